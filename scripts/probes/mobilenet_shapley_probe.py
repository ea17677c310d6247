"""Probe: Shapley values on MobileNetV2 through the MobileNet engine (``mobilenet_engine=True``: the
block's project conv by prefix scan, ``ops.prefix_project``) against the same engine with
``TORCHPRUNER_PREFIX_DELTA=0`` (masked copies of the hidden activation through the project conv) and
against the ``generic-hook`` path (K stacked copies of the input through the whole network: what the
same build runs with the engine off).

End to end, in one process: one permutation (``sv_samples=1``) over every channel of the first, a
middle and the last expanded block of ``mobilenet_v2(1000)`` at 224 px, at both evaluation points
(post-expand and post-depthwise ReLU6), one batch, dense and with every hidden width cut by
30 % + 1. Every side runs once first (kernel tuning, allocation), then in alternating rounds timed
with device events; image-evaluations/s (prefix evaluations x images) from the median round,
spread = (max - min) / median of a side's own rounds. A ratio counts as a lead only where it exceeds
both sides' spread. Throughput only: on this untrained 1000-class net one masked channel moves no
fp32 loss, so every path returns zeros; agreement is what tests/test_mobilenet_shapley_gpu.py checks.

Per kernel: ``tpamd.prefix_project`` at the three blocks' shapes and the chunk sizes the metric picks,
timed with device events; ``--trace-kernels`` runs only those launches (20 per shape) for a
``rocprofv3 --kernel-trace --stats`` run of its own. Bytes/s count the cnt output copies written, the
base copy read and the 4-byte deltas gathered, against the 6.29 TB/s measured copy rate.

    python scripts/probes/mobilenet_shapley_probe.py [--out profiles/mobilenet/shapley_engine_vs_hook.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/probes/mobilenet_shapley_probe.py --trace-kernels
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from torchpruner_amd import Pruner, ShapleyAttributionMetric, get_mobilenet_pruning_graph, ops  # noqa: E402
from torchpruner_amd.data import DeviceLoader  # noqa: E402
from torchpruner_amd.engine import maybe_mobilenet_engine  # noqa: E402
from torchpruner_amd.models import mobilenet_v2  # noqa: E402
from torchpruner_amd.utils import find_best_module_for_attributions  # noqa: E402

COPY_RATE = 6.29e12  # measured device copy rate, bytes/s
TRACE_ITERS = 20
SIDES = (("engine", True, "1", "mobilenet"), ("engine, masked copies", True, "0", "mobilenet"),
         ("generic-hook", False, "1", "generic-hook"))


def build_model(pruned, px):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = mobilenet_v2(1000).to(dev)
    if pruned:
        rng = np.random.RandomState(0)
        pruner = Pruner(model, (3, px, px), dev)
        for module, cascade in get_mobilenet_pruning_graph(model):
            n = module.weight.shape[0]
            pruner.prune_model(module, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    return model.eval()


def timed_run(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3  # s


def targets(model):
    """(name, conv whose evaluation module is scored) of the first, a middle and the last expanded
    block, post-expand and post-depthwise (the pruning graph lists the last block first)."""
    graph = get_mobilenet_pruning_graph(model)
    out = []
    for name, gi in (("first", len(graph) - 1), ("middle", len(graph) // 2), ("last", 0)):
        module, cascade = graph[gi]
        out += [(f"{name:6s} post-expand", module), (f"{name:6s} post-dw    ", cascade[1])]
    return out


def end_to_end(a, emit):
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, 3, a.px, a.px, generator=gen).to(dev)
    y = torch.randint(0, 1000, (a.batch,), generator=gen).to(dev)
    shapes = []
    for pruned in (False, True):
        model = build_model(pruned, a.px)
        for name, conv in targets(model):
            runs, evals = {}, {}
            for side, on, delta, want in SIDES:
                def run(side=side, on=on, delta=delta, want=want):
                    os.environ["TORCHPRUNER_PREFIX_DELTA"] = delta
                    try:
                        np.random.seed(11)
                        m = ShapleyAttributionMetric(model, DeviceLoader(x, y, a.batch), F.cross_entropy, dev,
                                                     sv_samples=1, mobilenet_engine=on)
                        m.run(conv, find_best_evaluation_module=True)
                    finally:
                        del os.environ["TORCHPRUNER_PREFIX_DELTA"]
                    assert m.last_path["path"] == want, m.last_path
                    evals[side] = m.last_work["prefix_evals"]
                runs[side] = run
                run()  # tuning, allocation, lazily packed operands
            t = {s: [] for s in runs}
            for _ in range(a.rounds):
                for s, run in runs.items():
                    t[s].append(timed_run(run))
            med = {s: float(np.median(v)) for s, v in t.items()}
            spread = {s: (max(v) - min(v)) / med[s] * 100 for s, v in t.items()}
            n = conv.weight.shape[0]
            line = f"{'pruned' if pruned else 'dense ':6s} {name} n={n:4d} B={a.batch} {a.px}px:"
            for s in runs:
                line += f"  {s} {evals[s] / med[s]:9.0f} eval/s (spread {spread[s]:4.1f}%)"
            e, c, h = med["engine"], med["engine, masked copies"], med["generic-hook"]
            lead = lambda r, s1, s2: "exceeds" if (r - 1) * 100 > max(spread[s1], spread[s2]) else "within"
            line += (f"  engine/hook {h / e:6.2f}x ({lead(h / e, 'engine', 'generic-hook')} the spreads)  "
                     f"engine/masked copies {c / e:5.2f}x ({lead(c / e, 'engine', 'engine, masked copies')} the spreads)")
            emit(line)
            if not pruned:
                ev = find_best_module_for_attributions(model, conv)
                eng = maybe_mobilenet_engine(model, [ev], dev)
                bi, _ = eng.locate(ev)
                shapes.append((name, eng, bi))
        if not pruned:
            per_kernel(a, emit, model, x, shapes[1::2])  # once per block
        shapes = []
        del model
        torch.cuda.empty_cache()


def kernel_cases(a, model, x, blocks):
    for name, eng, bi in blocks:
        with torch.no_grad():
            h, y = eng.forward_to(x, bi)
        e = eng._pack()["blocks"][bi]
        wt = eng._bwd_operands(e["project"])["wt"]
        B, Ho, Wo, C = y.shape
        N, Co = B * Ho * Wo, wt.shape[1]
        n = eng.plan.blocks[bi].dw.conv.weight.shape[0]
        cnt = max(1, min(n, (1 << 29) // (4 * B * eng.downstream_elems(bi, tuple(x.shape[1:])))))  # the metric's K
        base = torch.randn(N, Co, device=x.device)
        perm = torch.randperm(n, device=x.device).to(torch.int32)
        fill = eng.prefix_fill(bi, "expand")
        fn = lambda base=base, y=y, fill=fill, wt=wt, perm=perm, cnt=cnt, N=N, C=C: ops.prefix_project(
            base, y.view(N, C), fill, wt, perm, 0, cnt)
        yield (name.split()[0], N, C, Co, cnt), fn, 4 * (cnt * N * Co + N * Co + (cnt - 1) * N)


def per_kernel(a, emit, model, x, blocks):
    emit(f"# tpamd.prefix_project (device events, min of 3 windows), dense model, B={a.batch}, cnt = the metric's chunk")
    for (name, N, C, Co, cnt), fn, nbytes in kernel_cases(a, model, x, blocks):
        iters = max(3, min(50, int(2e9 / nbytes)))
        fn()

        def timed():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / iters * 1e-3
        t = min(timed() for _ in range(3))
        emit(f"{name:6s} block  N={N:6d} C={C:4d} Co={Co:4d} cnt={cnt:3d}  {t * 1e6:8.1f} us  {nbytes / 1e6:7.1f} MB  "
             f"{nbytes / t / 1e12:5.2f} TB/s = {nbytes / t / COPY_RATE * 100:5.1f}% of the copy rate")


def trace_kernels(a):
    """Only the launches: TRACE_ITERS per shape, first / middle / last block in that order."""
    dev = torch.device("cuda")
    model = build_model(False, a.px)
    x = torch.randn(a.batch, 3, a.px, a.px, device=dev)
    blocks = []
    for name, conv in targets(model)[1::2]:
        ev = find_best_module_for_attributions(model, conv)
        eng = maybe_mobilenet_engine(model, [ev], dev)
        blocks.append((name, eng, eng.locate(ev)[0]))
    for _, fn, _ in kernel_cases(a, model, x, blocks):
        for _ in range(TRACE_ITERS):
            fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--px", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "mobilenet", "shapley_engine_vs_hook.txt"))
    ap.add_argument("--trace-kernels", action="store_true", help="only the kernel launches (program of a rocprofv3 run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mobilenet_shapley_probe needs a GPU: nothing is measured without one")
    if a.trace_kernels:
        trace_kernels(a)
        return
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit(f"# mobilenet_shapley_probe: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, fp32, sv_samples=1; "
         f"engine = mobilenet_engine=True, masked copies = engine with TORCHPRUNER_PREFIX_DELTA=0, generic-hook = the "
         f"same build with the engine off (the default); device events, image-evaluations/s")
    end_to_end(a, emit)
    out.close()


if __name__ == "__main__":
    main()
