#!/usr/bin/env python
"""Headline benchmark: attribution images/sec (whole node), VGG16 Taylor; top-1 retained @ 50% pruned.

Launch (one process per GPU; the reference is single-device, attributions.py:16-22):
* ``python bench.py --gpus N`` spawns N rank processes itself (parallel/launch.py: the parent
  never touches the GPU, children get RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* and the parent exits
  with the worst child return code); under ``torchrun`` (WORLD_SIZE set) nothing is re-spawned.
  A rank that finds fewer GPUs on the node than ranks exits non-zero (``TORCHPRUNER_SHARE_GPU=1``
  + ``TORCHPRUNER_DIST_BACKEND=gloo`` rehearses N ranks on one GPU).
* The JSON reports ``dist_backend`` and ``world_size_seen`` (``dist.get_world_size()``).

A plain run (``python bench.py --gpus N --steps K --warmup W``) does only what the headline
needs: teacher, W warm-up steps, K timed steps, the JSON line (``ms_per_step``: one timed step;
``vs_baseline`` null). ``--dump-outputs DIR`` also writes the timed run's scores as ``.npy``.
``--full`` adds everything below that is not the headline: ``vs_baseline`` and
``generic_run_many_img_s``, the other BASELINE configs and the accuracy protocol.

Throughput (timed; BASELINE.json config #2, scaled to N GPUs):
* VGG16-BN / CIFAR-10 shape (reference experiments/models/cifar10.py:62-77), eval mode, fp32
  (the reference's precision), weights of a briefly trained teacher (untimed). Every rank
  trains the same deterministic teacher; the digests are all-gathered and rank 0's weights
  are broadcast before timing (``teacher_sync``).
* One step = Taylor attribution of one batch of B images for EVERY conv layer (the 13 units a
  50%-filter prune needs), evaluated after BN+ReLU (``find_best_evaluation_module``), through the
  public API ``TaylorAttributionMetric.run_many``.
* Data parallel: whole batches sharded per rank (each rank materialises only its own batches,
  HBM-resident before timing: no host->device copy in the timed region), scores all-reduced
  over RCCL at the end of ``run_many`` (inside the timed region). Weak scaling: B images per GPU
  per step; ``value`` = total img/s.
* ``vs_baseline``: the reference has no published number for this metric, so
  the comparison point is the reference algorithm run eagerly on the same GPU (one full pass
  per layer, activation clone + non-full backward hook, full backward, per-batch host numpy
  concatenation; ``bench/reference_semantics.py``), timed on rank 0 for a few batches.
  ``vs_baseline`` = per-GPU throughput / eager per-GPU throughput. ``generic_run_many_img_s``
  separates the algorithm from the kernels: the SAME one-pass ``run_many`` on the generic
  module/hook path with MIOpen / hipBLASLt convolutions (``TORCHPRUNER_ENGINES=0``,
  ``TORCHPRUNER_GENERIC_NATIVE=0``), sharded the same way.

Other BASELINE configs in the same run (``--full``; all ranks, sharded like the headline):
* ``resnet50_apoz_img_s`` / ``resnet50_taylor_img_s``: config #3, ResNet-50 224x224 B=256 per
  GPU, every prunable bottleneck conv in one ``run_many`` on the ResNet engine.
* ``vgg_taylor_b100_img_s``: the headline's fp32 Taylor run_many at the reference's attribution
  batch B=100 per GPU (200 timed steps; small batches replay HIP graphs, four in flight).
* ``shapley_vgg_img_evals_s``: config #4, Shapley sv_samples=5 over 1000 images (B=100, the
  nbVGG setup) at conv layers 0 / 6 / 12, downstream image-evaluations per second.

* ``resnet50_finetune_img_s``: config #5, the ResNet-50 training step of the prune -> finetune loop
  (224 px, B=128 per GPU, native kernels, PrunableDDP + SGD momentum, bucketed gradient
  all-reduce over RCCL) timed after one data-parallel Taylor prune of every prunable bottleneck
  conv + DDP rewrap; ``resnet50_prune_finetune``: one prune -> finetune round, Taylor vs Random,
  from one teacher (``bench/resnet_finetune.py``).

Accuracy (``--full``; untimed; ``bench/prune_quality.py``, rank 0 after the process group is torn down):
the teacher is pruned for real — ``Pruner.prune_model`` through ``get_vgg_pruning_graph`` on
every conv, 50% of the filters, in 4 increments per layer with a few SGD steps between
increments (Molchanov-style iterative pruning), Taylor scores vs Random scores under the same
finetune budget. ``top1_retained_at_50pct`` = top-1 of the Taylor-pruned network / top-1 of the
teacher, on held-out samples, averaged over ``--quality-seeds`` seeds (each seed its own
teacher and task draw); ``*_wd5e-4`` repeats it with the reference's weight decay.
``top1_layerwise_mask_50pct_*``: the reference's layerwise-robustness protocol at one point
(nbVGG:1233-1285: each layer alone, lowest half of its units zeroed after BN+ReLU).

Synthetic data of CIFAR-10 / ImageNet shape (no datasets in this environment).
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
METRIC = "attribution images/sec (whole node) VGG16 Taylor; top-1 retained @ 50% pruned"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one per GPU); self-spawned unless under torchrun")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("BENCH_BATCH", 2048)),
                    help="images per GPU per step (HBM-sized: small-spatial layers need >= 2k images to "
                         "fill 256 CUs; 4096 / 8192 measure 1-3%% more, but the MIOpen comparison extra "
                         "then re-tunes for a minute)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run everything else this file measures: the reference-semantics "
                         "eager timing (vs_baseline), the extras and the accuracy protocol (each can be switched "
                         "off again with --no-baseline / --no-extras / --extras / --no-prune). Without --full "
                         "only the headline is set up, warmed up, timed and reported")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the arrays the timed run_many returned (one float32 score "
                         "vector per conv layer, covering the timed steps up to the last) as DIR/<name>.npy")
    ap.add_argument("--no-baseline", action="store_true", help="skip the reference-semantics eager timing")
    ap.add_argument("--baseline-batches", type=int, default=2)
    ap.add_argument("--no-prune", action="store_true", help="skip the (untimed) accuracy protocol")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the generic-path / ResNet-50 / Shapley figures")
    ap.add_argument("--generic-steps", type=int, default=2)
    ap.add_argument("--resnet-steps", type=int, default=16)
    ap.add_argument("--resnet-batch", type=int, default=256, help="config #3 images per GPU per step")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quality-seeds", type=int, default=5,
                    help="accuracy protocol over seeds seed..seed+K-1 (each its own teacher); top-1 figures "
                         "are means over the seeds, per-seed values are listed")
    ap.add_argument("--teacher-steps", type=int, default=None)
    ap.add_argument("--extras", default="generic,bf16,b100,pruned,resnet,shapley,finetune,quality5",
                    help="comma-separated extras to run (with --no-extras: none)")
    ap.add_argument("--finetune-steps", type=int, default=10)
    ap.add_argument("--finetune-batch", type=int, default=128)
    ap.add_argument("--finetune-res", type=int, default=224)
    ap.add_argument("--q5-res", type=int, default=112, help="config #5 quality round: image size")
    ap.add_argument("--q5-max-steps", type=int, default=800, help="config #5 quality round: teacher step cap")
    return ap.parse_args()


def _launcher():
    """parallel/launch.py loaded by path: the spawning parent imports neither torch nor the package."""
    spec = importlib.util.spec_from_file_location(
        "_tp_launch", os.path.join(ROOT, "torchpruner_amd", "parallel", "launch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    args = parse()
    rc = _launcher().maybe_spawn(args.gpus, os.path.abspath(__file__), sys.argv[1:], cwd=ROOT)
    if rc is not None:
        sys.exit(rc)
    sys.exit(run(args))


def run(args) -> int:
    import numpy as np
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    from torchpruner_amd import TaylorAttributionMetric
    from torchpruner_amd.bench import prune_quality as pq
    from torchpruner_amd.data import ShardLoader
    from torchpruner_amd.parallel import dist as pdist
    from torchpruner_amd.utils import find_best_module_for_attributions

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env > 1 and os.environ.get("TORCHPRUNER_SHARE_GPU") != "1":
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world_env))
        ndev = torch.cuda.device_count()  # does not initialise the HIP runtime
        if ndev < local_world:
            print(f"[bench] rank {os.environ.get('RANK')}: {local_world} ranks on this node but only {ndev} GPU(s) "
                  "visible (set TORCHPRUNER_SHARE_GPU=1 with TORCHPRUNER_DIST_BACKEND=gloo to rehearse)",
                  file=sys.stderr, flush=True)
            return 3
    if world_env > 1:
        # the generic-path extra runs MIOpen: the ranks of this job share one user perf-db / kernel
        # cache, which rank 0 fills alone first (_generic): the other ranks then read the compiled
        # kernels instead of every rank JIT-compiling the same convolutions (85 s at 4 shared ranks
        # in round 4, VERDICT weak #9)
        tag = f"{os.environ.get('MASTER_ADDR', 'local').replace('.', '_')}_{os.environ.get('MASTER_PORT', '0')}"
        os.environ.setdefault("MIOPEN_USER_DB_PATH", f"/tmp/tp_miopen_db_{tag}")
        os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", f"/tmp/tp_miopen_cache_{tag}")
    ctx = pdist.init_distributed()
    dev = ctx.device
    world, rank = ctx.world_size, ctx.rank
    if dev.type != "cuda":
        print("[bench] needs a GPU", file=sys.stderr, flush=True)
        return 2
    if world != args.gpus and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but the launcher started {world} rank(s); reporting {world}",
              file=sys.stderr, flush=True)
    world_seen = torch.distributed.get_world_size() if pdist.is_dist() else 1
    backend_seen = torch.distributed.get_backend() if pdist.is_dist() else None

    def log(*a):
        if rank == 0:
            print(*a, file=sys.stderr, flush=True)

    def timed_run(metric, modules, **kw):
        pdist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = metric.run_many(modules, find_best_evaluation_module=True, **kw)
        torch.cuda.synchronize()
        pdist.barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            dt = pdist.all_max_float(dt)
        return scores, dt

    from torchpruner_amd.engine.fused_chain import TUNER, tuner_choices
    phase = {}  # wall seconds per phase (rank 0's clock): an over-budget run can be attributed
    t_run = time.perf_counter()
    cfg = dict(pq.DEFAULTS)
    if args.teacher_steps is not None:
        cfg["teacher_steps"] = args.teacher_steps
    t0 = time.perf_counter()
    model, task = pq.make_teacher(args.seed, dev, cfg)  # deterministic: identical on every rank ...
    sync = pdist.sync_module(model)  # ... checked (digests all-gathered) and made so (rank 0 broadcast)
    phase["teacher"] = time.perf_counter() - t0
    log(f"[bench] teacher: {cfg['teacher_steps']} SGD steps in {time.perf_counter() - t0:.1f}s (untimed); "
        f"ranks agreed before broadcast: {sync['agreed_before']}")
    convs = [m for m in model.features if isinstance(m, torch.nn.Conv2d)]
    B = args.batch

    def loader(n_steps, seed, bs=B):  # this rank's batches only (global batch i from seed i)
        return ShardLoader.build(lambda i: task.sample(bs, seed * 1_000_003 + i), max(n_steps, 1) * world, bs,
                                 rank, world)

    t0 = time.perf_counter()
    warm = TaylorAttributionMetric(model, loader(args.warmup, args.seed + 1), F.cross_entropy, dev)
    metric = TaylorAttributionMetric(model, loader(args.steps, args.seed + 2), F.cross_entropy, dev)
    timed_run(warm, convs)  # warmup (untimed): W steps + the collective
    scores, dt = timed_run(metric, convs)
    assert metric.last_path["path"] == "fused", metric.last_path
    del warm, metric
    phase["headline"] = time.perf_counter() - t0
    head_choices = tuner_choices()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, scores)
    value = args.steps * B * world / dt
    log(f"[bench] {world} GPU(s) x {args.steps} steps x B={B}: {dt * 1e3:.1f} ms -> {value:.0f} img/s "
        f"(fused path, backend {backend_seen}, world {world_seen})")

    result = {
        "metric": METRIC,
        "value": round(value, 1),
        "unit": "images/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp32",
        "data": f"synthetic (CIFAR-10-shaped prototype-mixture task, {cfg['modes']} modes/class, noise "
                f"{cfg['noise']}, {cfg['label_noise']:.0%} label noise; random-init VGG16-BN trained "
                f"{cfg['teacher_steps']} steps, untimed); each rank's batches are generated in HBM before timing "
                "(no host->device copy in the timed region)",
        "config": {
            "model": "VGG16-BN (CIFAR-10, reference classifier)",
            "global_batch": B * world,
            "per_gpu_batch": B,
            "seq_len": None,
            "parallelism": f"dp{world}",
            "method": "TaylorAttributionMetric.run_many over 13 conv layers, find_best_evaluation_module=True",
        },
        "dist_backend": backend_seen,
        "world_size_seen": world_seen,
        "launcher": "torchrun/external" if os.environ.get("TORCHELASTIC_RUN_ID") else
                    ("bench.py --gpus (self-spawned ranks)" if world > 1 else "single process"),
        "teacher_sync": {"agreed_before_broadcast": sync["agreed_before"], "digest": sync["digest"]},
        "tuner_choices": {"headline": head_choices},
        "phase_wall_s": phase,
    }

    if args.full and not args.no_extras:
        # the extras run after the timed headline: one that raises (on every rank alike) is reported in
        # the JSON line instead of costing the headline its line
        try:
            result.update(extras(args, model, task, convs, dev, world, rank, timed_run, log, value, phase, scores))
        except Exception as e:  # noqa: BLE001
            log(f"[bench] extras failed: {e!r}")
            result["extras_error"] = repr(e)[:800]
        if "b100_tuner_choices" in result:
            result["tuner_choices"]["b100"] = result.pop("b100_tuner_choices")

    if world > 1:  # everything below is single-rank: no rank may wait in a collective meanwhile
        pdist.barrier()
        torch.distributed.destroy_process_group()
    if rank != 0:
        return 0

    if args.full and not args.no_baseline:
        from torchpruner_amd.bench.reference_semantics import reference_taylor_all
        from torchpruner_amd.data import DeviceLoader
        nb = args.baseline_batches
        t_eager = time.perf_counter()
        xb, yb = task.sample(nb * B, args.seed + 5)
        bt = None
        try:
            with _env(TORCHPRUNER_BACKEND="torch"):
                ev = [find_best_module_for_attributions(model, c) for c in convs]
                reference_taylor_all(model, DeviceLoader(xb[:B], yb[:B], B), F.cross_entropy, dev, ev[:1])  # warm
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                reference_taylor_all(model, DeviceLoader(xb, yb, B), F.cross_entropy, dev, ev)
                torch.cuda.synchronize()
                bt = time.perf_counter() - t1
        except Exception as e:  # noqa: BLE001  (rank 0 only, after the timed region: vs_baseline stays null)
            log(f"[bench] reference-semantics eager run failed: {e!r}")
            result["eager_reference_error"] = repr(e)[:800]
        finally:
            model.zero_grad(set_to_none=True)
        if bt is not None:
            eager = nb * B / bt
            result["eager_reference_img_s_per_gpu"] = round(eager, 1)
            result["vs_baseline"] = round((value / world) / eager, 2)
            result["vs_baseline_definition"] = ("per-GPU img/s / reference-semantics eager img/s on the same GPU "
                                                "(BASELINE.md: the reference publishes no number for this metric)")
            log(f"[bench] reference-semantics eager: {eager:.0f} img/s per GPU -> vs_baseline {result['vs_baseline']}")
        phase["eager_reference"] = time.perf_counter() - t_eager

    if args.full and not args.no_prune:
        t0 = time.perf_counter()
        try:
            result.update(accuracy(args, model, task, convs, scores, cfg, dev, log))
        except Exception as e:  # noqa: BLE001  (rank 0 only, after the timed region)
            log(f"[bench] accuracy phase failed: {e!r}")
            result["accuracy_error"] = repr(e)[:800]
        phase["accuracy"] = time.perf_counter() - t0
    phase["total"] = time.perf_counter() - t_run
    result["phase_wall_s"] = {k: round(v, 1) for k, v in phase.items()}

    print(json.dumps(result), flush=True)
    return 0


def dump_outputs(out_dir, scores):
    """``--dump-outputs``: what the timed ``run_many`` returned to its caller, one array per conv
    layer in network order (``taylor_conv00.npy`` ...): each the layer's per-filter Taylor scores
    over every timed step, the last included (all-reduced over the ranks). The batches come from
    ``--seed`` alone, so two builds run with the same arguments score the same images."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for k, s in enumerate(scores):
        s = np.asarray(s)
        np.save(os.path.join(out_dir, f"taylor_conv{k:02d}.npy"),
                s if s.dtype in (np.float32, np.float64) else s.astype(np.float64))


def extras(args, model, task, convs, dev, world, rank, timed_run, log, value, phase, scores):
    """Same-algorithm library baseline + BASELINE configs #3 / #4 / #5 (all ranks, sharded)."""
    from torchpruner_amd.data import ShardLoader

    out = {}
    want = set(args.extras.split(","))

    def loader(n, seed, bs):
        return ShardLoader.build(lambda i: task.sample(bs, seed * 1_000_003 + i), n * world, bs, rank, world)

    def timed_phase(name, fn, *a):
        t0 = time.perf_counter()
        out.update(fn(*a))
        phase[name] = time.perf_counter() - t0

    # 1. the same one-pass run_many on the generic module/hook path, MIOpen/hipBLASLt convolutions
    if "generic" in want:
        timed_phase("generic", _generic, args, model, convs, dev, world, timed_run, log, value, loader)
    if "bf16" in want:
        timed_phase("bf16", _bf16, args, model, convs, dev, world, timed_run, log, value, loader)
    if "b100" in want:
        timed_phase("b100", _b100, args, model, task, convs, dev, world, rank, timed_run, log, loader)
    if "pruned" in want:
        timed_phase("pruned", _pruned, args, model, task, convs, scores, dev, world, timed_run, log, value, loader)
    if "resnet" in want:
        timed_phase("resnet", _resnet, args, dev, world, timed_run, log)
    if "shapley" in want:
        timed_phase("shapley", _shapley, args, model, task, convs, dev, world, log)
    if "finetune" in want or "quality5" in want:
        from torchpruner_amd.bench import resnet_finetune as rf
        if "finetune" in want:
            t0 = time.perf_counter()
            r = rf.finetune_throughput(dev, world, rank, steps=args.finetune_steps, batch=args.finetune_batch,
                                       res=args.finetune_res, seed=args.seed)
            out.update(r)
            phase["finetune"] = time.perf_counter() - t0
            log(f"[bench] config #5 ResNet-50 finetune step after a 20% prune + DDP rewrap, B={args.finetune_batch}: "
                f"{r['resnet50_finetune_img_s']:.0f} img/s (dense {r['resnet50_train_dense_img_s']:.0f}) "
                f"({time.perf_counter() - t0:.1f}s)")
        if "quality5" in want:
            t0 = time.perf_counter()
            q = rf.prune_finetune_quality(dev, world, rank, seed=args.seed,
                                          cfg={"res": args.q5_res, "teacher_max_steps": args.q5_max_steps})
            out["resnet50_prune_finetune"] = q
            phase["quality5"] = time.perf_counter() - t0
            log(f"[bench] config #5 one prune->finetune round (20%): teacher {q['teacher_top1']:.3f}; after prune "
                f"Taylor {q['taylor_after_prune']:.3f} / Random {q['random_after_prune']:.3f}; after finetune Taylor "
                f"{q['taylor_after_finetune']:.3f} / Random {q['random_after_finetune']:.3f} "
                f"({time.perf_counter() - t0:.1f}s)")
    return out


def _generic(args, model, convs, dev, world, timed_run, log, value, loader):
    import torch.nn.functional as F

    from torchpruner_amd import TaylorAttributionMetric
    out = {}
    B = args.batch
    t0 = time.perf_counter()
    with _env(TORCHPRUNER_ENGINES="0", TORCHPRUNER_GENERIC_NATIVE="0"):
        def warm():  # MIOpen kernel selection / compilation (untimed, no collective: shard_data=False)
            from torchpruner_amd.data import DeviceLoader
            xw, yw = next(iter(loader(1, args.seed + 11, B).batches.values()))  # this rank's batch
            TaylorAttributionMetric(model, DeviceLoader(xw, yw, B), F.cross_entropy, dev,
                                    shard_data=False).run_many(convs, find_best_evaluation_module=True)

        from torchpruner_amd.parallel import dist as pdist
        if world > 1 and pdist.get_rank() != 0:
            pdist.barrier()  # rank 0 has filled the shared MIOpen cache
            warm()
        else:
            warm()
            if world > 1:
                pdist.barrier()
        gm = TaylorAttributionMetric(model, loader(args.generic_steps, args.seed + 12, B), F.cross_entropy, dev)
        _, gdt = timed_run(gm, convs)
        assert gm.last_path["path"] == "generic", gm.last_path
    model.zero_grad(set_to_none=True)
    generic = args.generic_steps * B * world / gdt
    out["generic_run_many_img_s"] = round(generic, 1)
    out["engine_vs_generic_same_algorithm"] = round(value / generic, 2)
    log(f"[bench] generic path (MIOpen/hipBLASLt, same one-pass run_many): {generic:.0f} img/s -> engine "
        f"x{value / generic:.2f} ({time.perf_counter() - t0:.1f}s)")
    return out


def _bf16(args, model, convs, dev, world, timed_run, log, value, loader):
    import torch
    import torch.nn.functional as F

    from torchpruner_amd import TaylorAttributionMetric
    out = {}
    B = args.batch
    # 1b. opt-in bf16 operands on the same engine (never the headline): throughput, and per-layer
    # rank agreement of the bf16 scores with the exact fp32 ones on the same batches
    t0 = time.perf_counter()
    TaylorAttributionMetric(model, loader(1, args.seed + 13, B), F.cross_entropy, dev,
                            compute_dtype=torch.bfloat16).run_many(convs, find_best_evaluation_module=True)  # tune
    bm = TaylorAttributionMetric(model, loader(args.steps, args.seed + 14, B), F.cross_entropy, dev,
                                 compute_dtype=torch.bfloat16)
    s_bf, bdt = timed_run(bm, convs)
    assert bm.last_path["path"] == "fused", bm.last_path
    s_fp = TaylorAttributionMetric(model, loader(args.steps, args.seed + 14, B), F.cross_entropy, dev).run_many(
        convs, find_best_evaluation_module=True)
    from scipy.stats import spearmanr
    rho = [float(spearmanr(a, b).correlation) for a, b in zip(s_bf, s_fp)]
    out["vgg_taylor_bf16_img_s"] = round(args.steps * B * world / bdt, 1)
    out["bf16_vs_fp32_engine"] = round(out["vgg_taylor_bf16_img_s"] / value, 2)
    out["bf16_score_spearman_min"] = round(min(rho), 5)
    out["bf16_config"] = {"compute_dtype": "bfloat16 operands (3x3 convs), fp32 accumulation/activations, fp64 "
                                           "score accumulators", "spearman_per_layer": [round(r, 5) for r in rho]}
    log(f"[bench] opt-in bf16 engine: {out['vgg_taylor_bf16_img_s']:.0f} img/s (x{out['bf16_vs_fp32_engine']} "
        f"fp32), min per-layer Spearman vs fp32 {min(rho):.4f} ({time.perf_counter() - t0:.1f}s)")
    return out


def _b100(args, model, task, convs, dev, world, rank, timed_run, log, loader):
    import torch
    import torch.nn.functional as F

    from torchpruner_amd import TaylorAttributionMetric
    from torchpruner_amd.engine.fused_chain import TUNER, tuner_choices
    out = {}
    # 1c. the same fp32 Taylor run_many at the reference's attribution batch B=100 (nbVGG:193-196):
    # the engine coalesces 5 consecutive loader batches into one 500-image launch (each batch's
    # 1/B loss scaling kept: the same per-sample scores), pipelined over HIP streams with
    # per-slot HIP-graph replay; also measured with one engine launch per loader batch, and fed
    # by the reference's own loader shape (host tensors, torch DataLoader, 1 worker, pinned memory)
    t0 = time.perf_counter()
    sb, s_steps = 100, 200
    res = {}
    before = set(TUNER.cache)
    for coalesce in ("1", "0"):
        os.environ["TORCHPRUNER_COALESCE"] = coalesce
        try:
            TaylorAttributionMetric(model, loader(20, args.seed + 15, sb), F.cross_entropy, dev).run_many(
                convs, find_best_evaluation_module=True)  # tune + capture (untimed)
            sm = TaylorAttributionMetric(model, loader(s_steps, args.seed + 16, sb), F.cross_entropy, dev)
            _, sdt = timed_run(sm, convs)
        finally:
            os.environ.pop("TORCHPRUNER_COALESCE", None)
        assert sm.last_path["path"] == "fused", sm.last_path
        res[coalesce] = (round(s_steps * sb * world / sdt, 1), sm.last_coalesce)
    out["b100_tuner_choices"] = tuner_choices({k: v for k, v in TUNER.cache.items() if k not in before})
    # host loader: this rank's 200 batches as host tensors behind a reference-style DataLoader
    # (experiments/models/cifar10.py:136-161: num_workers=1, pin_memory=True); run_many pins and
    # copies each batch one ahead on a side HIP stream (data/prefetch.py) — H2D time included
    xs, ys = [], []
    for i in range(rank, s_steps * world, world):
        x, y = task.sample(sb, (args.seed + 17) * 1_000_003 + i)
        xs.append(x.cpu())
        ys.append(y.cpu())
    ds = torch.utils.data.TensorDataset(torch.cat(xs), torch.cat(ys))
    del xs, ys
    host = {}
    # "per_sample": the reference's loader verbatim (default collate: 100 __getitem__ + a stack per
    # batch in the worker; the worker is forked at every pass); "batched": the same DataLoader class
    # with a BatchSampler (one indexing op per batch) and a persistent worker, forked once during
    # the warm-up pass: forking this GPU process stalls it ~1.2 s (profiles/bench/b100_host_loader_r5.txt)
    for kind in ("batched", "per_sample"):
        if kind == "per_sample":
            dl = torch.utils.data.DataLoader(ds, batch_size=sb, shuffle=False, num_workers=1, pin_memory=True)
        else:
            bs = torch.utils.data.BatchSampler(torch.utils.data.SequentialSampler(ds), sb, drop_last=False)
            dl = torch.utils.data.DataLoader(ds, sampler=bs, batch_size=None, num_workers=1, pin_memory=True,
                                             persistent_workers=True)
        # the DataLoader already holds only this rank's batches (i = rank, rank + world, ...): no
        # second sharding inside run_many (shard_data=False: each rank scores its own loader, no
        # collective; with the default sharding each rank would process only 1/world of its loader)
        TaylorAttributionMetric(model, dl, F.cross_entropy, dev, shard_data=False).run_many(
            convs, find_best_evaluation_module=True)  # warm (and, persistent, the worker's fork)
        hm = TaylorAttributionMetric(model, dl, F.cross_entropy, dev, shard_data=False)
        _, hdt = timed_run(hm, convs)
        assert hm.last_path["path"] == "fused", hm.last_path
        host[kind] = (round(s_steps * sb * world / hdt, 1), hm.last_coalesce)
    out["vgg_taylor_b100_img_s"] = res["1"][0]
    out["vgg_taylor_b100_one_launch_per_batch_img_s"] = res["0"][0]
    out["vgg_taylor_b100_host_loader_img_s"] = host["batched"][0]
    out["vgg_taylor_b100_host_loader_per_sample_img_s"] = host["per_sample"][0]
    out["b100_config"] = {"per_gpu_batch": sb, "steps": s_steps, "dtype": "fp32",
                          "coalesced_loader_batches_per_launch": res["1"][1],
                          "pipeline": "coalesced launches in flight on HIP streams, per-slot HIP-graph replay "
                                      "(one launch per loader batch: 4 in flight)",
                          "host_loader": "torch DataLoader over a TensorDataset of host fp32 tensors, num_workers=1, "
                                         "pin_memory=True (experiments/models/cifar10.py:136-161); run_many pins and "
                                         "copies one batch ahead on a side HIP stream (data/prefetch.py). "
                                         "host_loader_img_s: BatchSampler (one indexing op per batch), persistent worker "
                                         "(forked once, in the untimed warm-up pass); host_loader_per_sample_img_s: the "
                                         "reference's default per-sample collate, worker forked per pass (a ~1.2 s stall "
                                         "of this GPU process per fork, profiles/bench/b100_host_loader_r5.txt); "
                                         f"coalescing {host['batched'][1]}"}
    log(f"[bench] B=100 (reference attribution batch): {out['vgg_taylor_b100_img_s']:.0f} img/s with "
        f"{res['1'][1]} loader batches per launch, {res['0'][0]:.0f} img/s one launch per batch, "
        f"{out['vgg_taylor_b100_host_loader_img_s']:.0f} img/s from a host DataLoader (per-sample collate "
        f"{out['vgg_taylor_b100_host_loader_per_sample_img_s']:.0f}) "
        f"({time.perf_counter() - t0:.1f}s)")
    return out


def _pruned(args, model, task, convs, scores, dev, world, timed_run, log, value, loader):
    """The headline workload on the network a 50 % prune produces: the teacher with the lowest
    half of EVERY conv's filters (by the headline's all-reduced Taylor scores) really pruned
    through ``Pruner.prune_model`` + ``get_vgg_pruning_graph`` (widths 32/64/128/256, ~1/4 of the
    conv MACs), then the same fp32 ``run_many`` over its 13 convs at the same batch — whether the
    engine turns the pruned FLOPs into speed on the attribution side (reference flow: the model
    pruner.py:21-57 produces, scored by taylor.py:31-49)."""
    import copy

    import numpy as np
    import torch
    import torch.nn.functional as F

    from torchpruner_amd import Pruner, TaylorAttributionMetric, get_vgg_pruning_graph
    from torchpruner_amd.engine.fused_chain import TUNER, tuner_choices
    out = {}

    def conv_macs(net):  # conv multiply-adds of one image (forward hooks, one eval forward)
        tot = []
        hs = [m.register_forward_hook(lambda m, i, o: tot.append(o[0].numel() * m.in_channels * m.kernel_size[0]
                                                                 * m.kernel_size[1]))
              for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
        with torch.no_grad():
            net.eval()(torch.zeros(1, 3, 32, 32, device=dev))
        for h in hs:
            h.remove()
        return sum(tot)

    t0 = time.perf_counter()
    pm = copy.deepcopy(model)
    graph = [(m, c) for m, c in get_vgg_pruning_graph(pm) if isinstance(m, torch.nn.Conv2d)]
    by_conv = {id(c): s for c, s in zip([m for m in pm.features if isinstance(m, torch.nn.Conv2d)], scores)}
    pruner = Pruner(pm, (3, 32, 32), dev, sync_indices=False)  # scores are identical on every rank
    for module, cascade in graph:
        s = by_conv[id(module)]
        pruner.prune_model(module, np.argsort(s, kind="stable")[: len(s) // 2], cascading_modules=cascade)
    pconvs = [m for m in pm.features if isinstance(m, torch.nn.Conv2d)]
    macs = conv_macs(pm) / conv_macs(model)
    B = args.batch
    before = set(TUNER.cache)
    TaylorAttributionMetric(pm, loader(1, args.seed + 31, B), F.cross_entropy, dev).run_many(
        pconvs, find_best_evaluation_module=True)  # autotune the new shapes (untimed)
    pmet = TaylorAttributionMetric(pm, loader(args.steps, args.seed + 32, B), F.cross_entropy, dev)
    _, pdt = timed_run(pmet, pconvs)
    assert pmet.last_path["path"] == "fused", pmet.last_path
    v = args.steps * B * world / pdt
    out["vgg_taylor_pruned50_img_s"] = round(v, 1)
    out["pruned50_vs_dense"] = round(v / value, 2)
    out["pruned50_config"] = {"widths": [c.out_channels for c in pconvs], "per_gpu_batch": B, "dtype": "fp32",
                              "conv_mac_fraction": round(macs, 4),
                              "params": sum(p.numel() for p in pm.parameters()),
                              "prune": "lowest 50% of every conv's filters by the headline's Taylor scores, "
                                       "Pruner.prune_model + get_vgg_pruning_graph cascade (one shot)",
                              "tuner_choices": tuner_choices({k: v for k, v in TUNER.cache.items()
                                                              if k not in before})}
    log(f"[bench] 50%-pruned VGG16 (conv MACs x{macs:.3f}): {v:.0f} img/s = x{v / value:.2f} the dense headline "
        f"({time.perf_counter() - t0:.1f}s)")
    del pm, pmet
    return out


def _resnet(args, dev, world, timed_run, log):
    import torch
    import torch.nn.functional as F

    from torchpruner_amd import APoZAttributionMetric, TaylorAttributionMetric, get_resnet_pruning_graph
    from torchpruner_amd.data import StreamLoader
    from torchpruner_amd.models import resnet50
    from torchpruner_amd.parallel import dist as pdist
    out = {}
    # 2. config #3: ResNet-50, ImageNet shape, B=256 per GPU, every prunable bottleneck conv
    t0 = time.perf_counter()
    torch.manual_seed(0)
    rn = resnet50().to(dev).eval().to(memory_format=torch.channels_last)
    rsync = pdist.sync_module(rn)
    mods = [m for m, _ in get_resnet_pruning_graph(rn)]
    rb = args.resnet_batch
    for name, M in (("apoz", APoZAttributionMetric), ("taylor", TaylorAttributionMetric)):
        M(rn, StreamLoader(2 * world, rb, (3, 224, 224), 1000, dev, seed=1, channels_last=True), F.cross_entropy,
          dev).run_many(mods, find_best_evaluation_module=True)  # autotune (untimed)
        m = M(rn, StreamLoader(args.resnet_steps * world, rb, (3, 224, 224), 1000, dev, seed=2, channels_last=True),
              F.cross_entropy, dev)
        _, rdt = timed_run(m, mods)
        assert m.last_path["path"] == "resnet", m.last_path
        out[f"resnet50_{name}_img_s"] = round(args.resnet_steps * rb * world / rdt, 1)
    out["resnet50_config"] = {"per_gpu_batch": rb, "image": [3, 224, 224], "steps": args.resnet_steps,
                              "modules_scored": len(mods), "path": "resnet engine", "dtype": "fp32",
                              "weights": "random init (seed 0), synced from rank 0",
                              "agreed_before_broadcast": rsync["agreed_before"]}
    log(f"[bench] ResNet-50 B={rb}: APoZ {out['resnet50_apoz_img_s']:.0f} img/s, Taylor "
        f"{out['resnet50_taylor_img_s']:.0f} img/s ({time.perf_counter() - t0:.1f}s)")
    del rn
    return out


def _shapley(args, model, task, convs, dev, world, log):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from torchpruner_amd import ShapleyAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    from torchpruner_amd.parallel import dist as pdist
    out = {}
    # 3. config #4: Shapley sv_samples=5, 1000 images at B=100 (nbVGG:185-196), layers 0 / 6 / 12
    t0 = time.perf_counter()
    xs, ys = task.sample(1000, args.seed + 21)
    S = 5
    rows, tot_evals, tot_s = [], 0, 0.0
    for li in (0, 6, 12):
        conv = convs[li]
        sm = ShapleyAttributionMetric(model, DeviceLoader(xs, ys, 100), F.cross_entropy, dev, sv_samples=S)
        np.random.seed(args.seed)
        sm.run(conv, find_best_evaluation_module=True, sv_samples=1)  # autotune / allocate (untimed)
        np.random.seed(args.seed)
        pdist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sv = sm.run(conv, find_best_evaluation_module=True)
        torch.cuda.synchronize()
        pdist.barrier()
        sdt = pdist.all_max_float(time.perf_counter() - t1) if world > 1 else time.perf_counter() - t1
        assert sm.last_path["path"] == "fused", sm.last_path
        evals = S * conv.out_channels * xs.shape[0]
        rows.append({"layer": li, "units": conv.out_channels, "seconds": round(sdt, 4),
                     "img_evals_per_s": round(evals / sdt, 1), "finite": bool(np.isfinite(sv).all())})
        tot_evals += evals
        tot_s += sdt
    out["shapley_vgg_img_evals_s"] = round(tot_evals / tot_s, 1)
    out["shapley_vgg_layers"] = rows
    out["shapley_vgg_config"] = {"sv_samples": S, "images": 1000, "batch": 100, "layers": [0, 6, 12],
                                 "unit": "downstream image-evaluations/s (whole node; reference study ~9.9k, "
                                         "BASELINE.md derived)"}
    log(f"[bench] Shapley S=5 layers 0/6/12: {out['shapley_vgg_img_evals_s']:.0f} img-evals/s "
        f"({time.perf_counter() - t0:.1f}s)")
    return out


def accuracy(args, model, task, convs, scores, cfg, dev, log):
    """Untimed accuracy protocol (rank 0, after the process group is gone)."""
    import copy

    import numpy as np

    from torchpruner_amd.bench import prune_quality as pq
    from torchpruner_amd.utils import find_best_module_for_attributions

    def layerwise_mask_top1(scores_, x, y, frac=0.5):
        """Reference layerwise-robustness protocol (nbVGG:1233-1285) at one point: for each conv
        layer alone, zero the ``frac`` lowest-scored channels after its BN+ReLU; mean top-1."""
        import torch
        accs = []
        with torch.no_grad():
            for conv, s in zip(convs, scores_):
                idx = torch.as_tensor(np.argsort(s, kind="stable")[: int(len(s) * frac)], device=x.device)
                ev = find_best_module_for_attributions(model, conv)
                h = ev.register_forward_hook(lambda m, i, o, idx=idx: o.index_fill(1, idx, 0.0))
                try:
                    accs.append(pq.top1(model, x, y))
                finally:
                    h.remove()
        return float(np.mean(accs))

    t1 = time.perf_counter()
    xv, yv = task.sample(cfg["val_imgs"], args.seed * 7 + 3)
    before = pq.top1(model, xv, yv)
    rng = np.random.RandomState(args.seed)
    lw_t = layerwise_mask_top1(scores, xv, yv)
    lw_r = float(np.mean([layerwise_mask_top1([rng.random_sample(c.out_channels) for c in convs], xv, yv)
                          for _ in range(3)]))
    runs = [{"seed": args.seed, "top1_before": before}]
    t2 = time.perf_counter()
    runs[0].update(pq.layerwise_auc(model, task, args.seed))
    log(f"[quality] seed {args.seed}: layerwise AUC Taylor {runs[0]['layerwise_auc_taylor']:.4f} / SV "
        f"{runs[0]['layerwise_auc_sv']:.4f} / Random {runs[0]['layerwise_auc_random']:.4f} "
        f"({time.perf_counter() - t2:.1f}s)")
    runs[0].update(pq.oneshot_top1(model, task, args.seed, cfg, xv, yv))
    params = None
    for method in ("taylor", "random"):
        m = pq.iterative_prune(copy.deepcopy(model), task, method, args.seed, cfg)
        runs[0][f"top1_pruned_{method}"] = pq.top1(m, xv, yv)
        params = sum(p.numel() for p in m.parameters())
    log(f"[quality] seed {args.seed}: one-shot + iterative prunes done ({time.perf_counter() - t1:.1f}s)")
    for s in range(args.seed + 1, args.seed + max(1, args.quality_seeds)):
        runs.append(pq.run_protocol(s, dev, log=log, **cfg))  # its own teacher, task and held-out set
    mean = {k: float(np.mean([r[k] for r in runs])) for k in ("top1_before", "top1_pruned_taylor",
                                                             "top1_pruned_random")}
    std = {k: float(np.std([r[k] for r in runs])) for k in ("top1_before", "top1_pruned_taylor",
                                                           "top1_pruned_random")}
    ret = {m: float(np.mean([r[f"top1_pruned_{m}"] / max(r["top1_before"], 1e-9) for r in runs]))
           for m in ("taylor", "random")}
    pruned = {m: mean[f"top1_pruned_{m}"] for m in ("taylor", "random")}
    diff = np.array([r["top1_pruned_taylor"] - r["top1_pruned_random"] for r in runs])
    out = {
        "top1_retained_at_50pct": round(ret["taylor"], 4),
        "top1_before": round(mean["top1_before"], 4),
        "top1_pruned_50pct_taylor": round(pruned["taylor"], 4),
        "top1_pruned_50pct_random": round(pruned["random"], 4),
        "top1_retained_at_50pct_random": round(ret["random"], 4),
        "quality_seeds": [r["seed"] for r in runs],
        "top1_pruned_50pct_taylor_per_seed": [round(r["top1_pruned_taylor"], 4) for r in runs],
        "top1_pruned_50pct_random_per_seed": [round(r["top1_pruned_random"], 4) for r in runs],
        "top1_before_per_seed": [round(r["top1_before"], 4) for r in runs],
        "top1_mean_std": {"before": [round(mean["top1_before"], 4), round(std["top1_before"], 4)],
                          "taylor": [round(mean["top1_pruned_taylor"], 4), round(std["top1_pruned_taylor"], 4)],
                          "random": [round(mean["top1_pruned_random"], 4), round(std["top1_pruned_random"], 4)]},
        "taylor_minus_random": {"per_seed": [round(float(d), 4) for d in diff], "mean": round(float(diff.mean()), 4),
                                "std": round(float(diff.std(ddof=1)) if len(diff) > 1 else 0.0, 4),
                                "taylor_wins": int((diff > 0).sum()), "seeds": int(len(diff)),
                                "kernel_choices": "TUNER.fixed() (untimed heuristic configs: bit-reproducible)"},
        "params_before_after": [sum(p.numel() for p in model.parameters()), params],
        "prune_protocol": {k: cfg[k] for k in ("frac", "increments", "ft_steps", "final_ft_steps", "recal_batches",
                                               "score_imgs", "val_imgs", "ft_lr", "noise", "teacher_wd", "label_noise")},
        "top1_layerwise_mask_50pct_taylor": round(lw_t, 4),
        "top1_layerwise_mask_50pct_random": round(lw_r, 4),
    }
    # one-shot prune of every conv, BN statistics re-estimated, NO finetuning (the reference's
    # notebooks never finetune after pruning): separates the rankings, which finetuning hides
    for frac in pq.ONESHOT_FRACS:
        pc = int(frac * 100)
        kt, kr = f"top1_pruned_{pc}pct_oneshot_taylor", f"top1_pruned_{pc}pct_oneshot_random"
        d1 = np.array([r[kt] - r[kr] for r in runs])
        out[kt] = round(float(np.mean([r[kt] for r in runs])), 4)
        out[kr] = round(float(np.mean([r[kr] for r in runs])), 4)
        out[f"oneshot_{pc}pct_taylor_minus_random"] = {
            "per_seed": [round(float(d), 4) for d in d1], "mean": round(float(d1.mean()), 4),
            "std": round(float(d1.std(ddof=1)) if len(d1) > 1 else 0.0, 4), "taylor_wins": int((d1 > 0).sum()),
            "seeds": int(len(d1))}
    # the reference's layerwise-robustness AUC (nbVGG:1233-1285, 1521-1527) per seed, paired
    for mth in ("taylor", "random", "sv"):
        out[f"layerwise_auc_{mth}"] = round(float(np.mean([r[f"layerwise_auc_{mth}"] for r in runs])), 4)
    for mth in ("taylor", "sv"):
        d2 = np.array([r[f"layerwise_auc_{mth}"] - r["layerwise_auc_random"] for r in runs])
        out[f"layerwise_auc_{mth}_minus_random"] = {
            "per_seed": [round(float(d), 4) for d in d2], "mean": round(float(d2.mean()), 4),
            "std": round(float(d2.std(ddof=1)) if len(d2) > 1 else 0.0, 4),
            f"{mth}_better": int((d2 < 0).sum()), "seeds": int(len(d2))}
    out["layerwise_auc_per_seed"] = {mth: [round(r[f"layerwise_auc_{mth}"], 4) for r in runs]
                                     for mth in ("taylor", "random", "sv")}
    out["layerwise_auc_per_layer_seed0"] = {mth: runs[0][f"layerwise_auc_{mth}_per_layer"]
                                            for mth in ("taylor", "random", "sv")}
    out["layerwise_auc_protocol"] = dict(pq.LAYERWISE, layers=13, unit="mean loss increase per removed unit "
                                         "(nbVGG:1521-1527), units removed in ascending-score order after BN+ReLU, "
                                         "lower is better", kernel_choices="TUNER.fixed()")
    log(f"[bench] layerwise AUC (nbVGG protocol, lower is better) over seeds {out['quality_seeds']}: Taylor "
        f"{out['layerwise_auc_taylor']:.4f}, SV {out['layerwise_auc_sv']:.4f}, Random {out['layerwise_auc_random']:.4f}"
        f"; Taylor better on {out['layerwise_auc_taylor_minus_random']['taylor_better']}/{len(runs)} seeds, SV on "
        f"{out['layerwise_auc_sv_minus_random']['sv_better']}/{len(runs)}")
    out["oneshot_protocol"] = {"fracs": list(pq.ONESHOT_FRACS), "bn_recal_batches": pq.ONESHOT_RECAL,
                               "finetune_steps": 0, "taylor_score_imgs": cfg["score_imgs"],
                               "kernel_choices": "TUNER.fixed()"}
    log("[bench] one-shot (no finetune) " + ", ".join(
        f"{int(f * 100)}%: Taylor {out[f'top1_pruned_{int(f * 100)}pct_oneshot_taylor']:.4f} / Random "
        f"{out[f'top1_pruned_{int(f * 100)}pct_oneshot_random']:.4f} (Taylor wins "
        f"{out[f'oneshot_{int(f * 100)}pct_taylor_minus_random']['taylor_wins']}/{len(runs)})" for f in pq.ONESHOT_FRACS))
    log(f"[bench] Taylor - Random per seed {out['taylor_minus_random']['per_seed']}: mean "
        f"{out['taylor_minus_random']['mean']:+.4f} +- {out['taylor_minus_random']['std']:.4f}, Taylor wins "
        f"{out['taylor_minus_random']['taylor_wins']}/{len(diff)}")
    log(f"[bench] seeds {out['quality_seeds']}: mean top-1 before {mean['top1_before']:.4f}; 50% of every conv "
        f"pruned (iterative, {cfg['increments']} increments/layer, {cfg['ft_steps']} SGD steps each, "
        f"+{cfg['final_ft_steps']}): Taylor {pruned['taylor']:.4f}, Random {pruned['random']:.4f}; layerwise mask "
        f"(nbVGG protocol): Taylor {lw_t:.4f}, Random {lw_r:.4f} ({time.perf_counter() - t1:.1f}s untimed)")
    # the same protocol with the reference's weight decay (cifar10.py:95-99), one seed: reported
    # alongside because the headline protocol's teacher_wd=5e-3 was chosen by a sweep
    t2 = time.perf_counter()
    r = pq.run_protocol(args.seed, dev, layerwise=False, **dict(cfg, teacher_wd=5e-4))
    out["top1_pruned_50pct_wd5e-4"] = {"seed": args.seed, "before": round(r["top1_before"], 4),
                                       "taylor": round(r["top1_pruned_taylor"], 4),
                                       "random": round(r["top1_pruned_random"], 4)}
    log(f"[bench] same protocol, teacher wd 5e-4 (reference), seed {args.seed}: before {r['top1_before']:.4f}, "
        f"Taylor {r['top1_pruned_taylor']:.4f}, Random {r['top1_pruned_random']:.4f} "
        f"({time.perf_counter() - t2:.1f}s)")
    return out


if __name__ == "__main__":
    main()
