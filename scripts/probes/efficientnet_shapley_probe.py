"""Probe: Shapley values on EfficientNets through the MobileNet engine (``mobilenet_engine="shapley"``).

Project stage of a Fused-MBConv block (``EfficientNetEngine.fused_prefix_out``) at the distinct fused project
shapes of ``efficientnet_v2_s`` at 224 px, cnt = the metric's chunk: ``ops.silu_prefix_project`` (kernel)
against the composed route it replaces (``F.silu(z)``, a masked base conv, ``ops.prefix_project``) and the
``TORCHPRUNER_PREFIX_DELTA=0`` route (the project conv on the cnt masked copies); every side runs once first,
then they alternate in one process, device events around the stage, median and spread = (max - min) / median.

End to end: ``sv_samples=2`` over every channel of one evaluation point per model (``efficientnet_v2_s`` and
``efficientnet_b0``, ``small_input=True``, 64 px), engine against the generic path of the same build,
image-evaluations/s from the median round (a report, no gate).

    python scripts/probes/efficientnet_shapley_probe.py [--out profiles/mobilenet/efficientnet_shapley.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mobilenet_v3_shapley_probe import alternate  # noqa: E402
from torchpruner_amd import ShapleyAttributionMetric, ops  # noqa: E402
from torchpruner_amd.data import DeviceLoader  # noqa: E402
from torchpruner_amd.engine import maybe_mobilenet_engine  # noqa: E402
from torchpruner_amd.engine.mobilenet_engine import build_efficientnet_plan  # noqa: E402
from torchpruner_amd.models import efficientnet_b0, efficientnet_v2_s  # noqa: E402


CALLS = 10  # calls per timed window


def project_stage(a, emit):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = efficientnet_v2_s(1000).to(dev).eval()
    x = torch.randn(a.stage_batch, 3, a.px, a.px, device=dev)
    eng = maybe_mobilenet_engine(model, [], dev, shapley="lower")
    T, zero = ops.require(), torch.zeros((), device=dev)
    emit(f"# project stage of a Fused-MBConv block (device events, {a.rounds} alternating rounds of {CALLS} calls), efficientnet_v2_s "
         f"{a.px}px B={a.stage_batch}, cnt = the metric's chunk (and 8x it: the chunk of B / 8 images)")
    seen = set()
    for bi, blk in enumerate(eng.plan.blocks):
        if blk.dw is not None or blk.project is None:
            continue
        with torch.no_grad():
            h, z = eng.forward_to(x, bi)
        B, H, W, C = z.shape
        q = eng._pack()["blocks"][bi]["project"]
        co = q["scale"].numel()
        if (C, co, H, blk.shortcut) in seen:
            continue
        seen.add((C, co, H, blk.shortcut))
        n = eng.real_width(blk.expand.act)
        chunk = max(1, min(n, (1 << 29) // (4 * B * eng.downstream_elems(bi, tuple(x.shape[1:])))))
        perm = torch.randperm(n)
        rank = torch.full((C,), n + 1)
        rank[perm] = torch.arange(n)
        perm, rank = perm.to(torch.int32).to(dev), rank.to(torch.int32).to(dev)
        res, fill0 = h if blk.shortcut else None, torch.zeros(C, device=dev)
        for cnt in sorted({chunk, min(n, 8 * chunk, ((1 << 31) - 1) // (4 * B * H * W * max(co, C)))}):
            p0 = (n - cnt) // 2

            def composed(cnt=cnt, p0=p0, z=z, res=res):
                with torch.no_grad():
                    act = F.silu(z)
                    base = eng._conv(T, q, torch.where(rank < p0, zero, act), False, res=res)
                    return ops.prefix_project(base.view(-1, co), act.view(-1, C), fill0, q["wt_pfx"], perm, p0, cnt)

            def kernel(cnt=cnt, p0=p0, z=z, res=res):
                return ops.silu_prefix_project(z.view(-1, C), q["wt_pfx"], q["shift"],
                                               None if res is None else res.view(-1, co), perm, rank, p0, cnt)

            def delta0(cnt=cnt, p0=p0, z=z, res=res):  # the body of fused_prefix_out(delta=False)
                with torch.no_grad():
                    lim = torch.arange(p0, p0 + cnt, device=dev, dtype=rank.dtype).view(cnt, 1, 1, 1, 1)
                    act = torch.where(rank.view(1, 1, 1, 1, C) < lim, zero, F.silu(z).unsqueeze(0))
                    rr = res.repeat(cnt, 1, 1, 1) if res is not None and cnt > 1 else res
                    return eng._conv(T, q, act.view(cnt * B, H, W, C), False, res=rr)
            with torch.no_grad():
                assert torch.equal(kernel().view(-1), eng.fused_prefix_out(bi, h, z, perm, rank, p0, cnt).view(-1))
                assert torch.equal(delta0(), eng.fused_prefix_out(bi, h, z, perm, rank, p0, cnt, False))
            diff = float((kernel().view(-1) - composed().view(-1)).abs().max() / composed().abs().max())
            # operands are fetched once: a timed window holds the launches of CALLS calls and no engine packing
            r = alternate({k: (lambda f=f: any(f() is None for _ in range(CALLS))) for k, f in
                           (("kernel", kernel), ("composed", composed), ("delta0", delta0))}, a.rounds)
            r = {k: (t / CALLS, s) for k, (t, s) in r.items()}
            (tk, sk), (tc, sc), (td, sd) = r["kernel"], r["composed"], r["delta0"]
            emit(f"block {bi:2d} hidden {C:4d} -> {co:3d} at {H:3d}x{W:<3d} res={int(blk.shortcut)} cnt={cnt:3d}:  kernel "
                 f"{tk * 1e3:7.3f} ms ({sk:4.1f}%)  composed {tc * 1e3:7.3f} ms ({sc:4.1f}%)  DELTA=0 {td * 1e3:7.3f} ms "
                 f"({sd:4.1f}%)  composed/kernel {tc / tk:5.2f}x  DELTA=0/kernel {td / tk:5.2f}x  max rel diff {diff:.1e}")
    del model, eng
    torch.cuda.empty_cache()


def end_to_end(a, emit):
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, 3, a.e2e_px, a.e2e_px, generator=gen).to(dev)
    y = torch.randint(0, 1000, (a.batch,), generator=gen).to(dev)
    emit(f"# end to end (sv_samples=2, one batch of {a.batch} at {a.e2e_px}px, small_input=True, {a.rounds} alternating "
         "rounds), image-evaluations/s = prefix evaluations x images / median time")
    for mname, make in (("efficientnet_v2_s", efficientnet_v2_s), ("efficientnet_b0", efficientnet_b0)):
        torch.manual_seed(0)
        model = make(1000, small_input=True).to(dev).eval()
        blocks = build_efficientnet_plan(model)[0].blocks
        fused = [b for b in blocks if b.dw is None and b.project is not None]
        mb = [b for b in blocks if b.dw is not None and b.expand is not None]
        points = ([("fused expand", fused[len(fused) // 2].expand.conv)] if fused else []) + \
            [("MBConv depthwise", mb[len(mb) // 2].dw.conv)]
        for name, conv in points:
            evals = {}

            def side(on, conv=conv, evals=evals):
                def run():
                    np.random.seed(11)
                    m = ShapleyAttributionMetric(model, DeviceLoader(x, y, a.batch), F.cross_entropy, dev, sv_samples=2,
                                                 mobilenet_engine=on)
                    m.run(conv, find_best_evaluation_module=True)
                    assert (m.last_path["path"] == "mobilenet") == (on == "shapley"), m.last_path
                    evals[on] = m.last_work["prefix_evals"]
                return run
            r = alternate({"engine": side("shapley"), "generic": side(False)}, a.rounds)
            (te, se), (th, sh) = r["engine"], r["generic"]
            emit(f"{mname} {name} n={conv.weight.shape[0]:4d}:  engine {evals['shapley'] / te:9.0f} eval/s (spread {se:4.1f}%)  "
                 f"generic {evals[False] / th:9.0f} eval/s (spread {sh:4.1f}%)  engine/generic {th / te:6.2f}x")
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--stage-batch", type=int, default=64)
    ap.add_argument("--px", type=int, default=224)
    ap.add_argument("--e2e-px", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stage-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "mobilenet", "efficientnet_shapley.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("efficientnet_shapley_probe needs a GPU: nothing is measured without one")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as out:
        def emit(line):
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        emit(f"# efficientnet_shapley_probe: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, fp32; kernel = "
             "ops.silu_prefix_project, composed = F.silu + masked base conv + ops.prefix_project, DELTA=0 = the project "
             "conv on the cnt masked copies of silu(z)")
        project_stage(a, emit)
        if not a.stage_only:
            end_to_end(a, emit)


if __name__ == "__main__":
    main()
