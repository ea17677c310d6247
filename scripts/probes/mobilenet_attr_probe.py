"""Probe: attribution on MobileNetV2 through the MobileNet engine (engine/mobilenet_engine.py,
``mobilenet_engine=True``) against the generic path (hooks on PyTorch modules, every conv on the
native kernels: what the same build runs with the engine off).

End to end, in one process: Taylor and APoZ ``run_many`` over every entry of the pruning graph
(evaluated after the expand conv's ReLU6) of ``mobilenet_v2(1000)`` at 224 px, B=128, 8 batches,
dense and with every hidden width cut by 30 % + 1. Both sides run once first (kernel tuning,
allocation), then in alternating rounds timed with device events; img/s from the median round,
spread = (max - min) / median of a side's own rounds.

Per kernel: ``tpamd.dwconv_act_fwd`` / ``dwconv_act_dgrad`` (with Taylor partials) at the depthwise
shapes of the README's depthwise table, at the channel-padded widths the engine runs them at, timed
with device events here; ``--trace-kernels`` runs only those launches (20 per kernel and shape, in
table order) for a ``rocprofv3 --kernel-trace --stats`` run of its own. Bytes/s are over the floor
of one read of the input and one write of the output (forward: x + y; dgrad: g + y + z + dz) against
the 6.29 TB/s measured copy rate.

    python scripts/probes/mobilenet_attr_probe.py [--out profiles/mobilenet/attr_engine_vs_generic.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/probes/mobilenet_attr_probe.py --trace-kernels
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from torchpruner_amd import (APoZAttributionMetric, Pruner, TaylorAttributionMetric,  # noqa: E402
                             get_mobilenet_pruning_graph, ops)
from torchpruner_amd.data import DeviceLoader  # noqa: E402
from torchpruner_amd.engine.fused_chain import cpad  # noqa: E402
from torchpruner_amd.models import mobilenet_v2  # noqa: E402

COPY_RATE = 6.29e12  # measured device copy rate, bytes/s
# (real C, input H = W, stride) of the README's depthwise table (3x3, pad 1)
SHAPES = [(32, 112, 1), (22, 112, 1), (96, 112, 2), (144, 56, 1), (99, 56, 2), (576, 14, 1), (671, 7, 1)]
TRACE_ITERS = 20


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


def end_to_end(a, emit):
    dev = torch.device("cuda")
    n = a.batch * a.batches
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(n, 3, a.px, a.px, generator=gen).to(dev)
    y = torch.randint(0, 1000, (n,), generator=gen).to(dev)
    for pruned in (False, True):
        model = build_model(pruned, a.px)
        mods = [m for m, _ in get_mobilenet_pruning_graph(model)]
        for name, cls in (("taylor", TaylorAttributionMetric), ("apoz", APoZAttributionMetric)):
            sides, scores = {}, {}
            for side, on in (("engine", True), ("generic", False)):
                def run(on=on, side=side):
                    m = cls(model, DeviceLoader(x, y, a.batch), F.cross_entropy, dev, mobilenet_engine=on)
                    scores[side] = m.run_many(mods, find_best_evaluation_module=True)
                    want = "mobilenet" if on else "generic"
                    assert m.last_path["path"] == want, m.last_path
                sides[side] = run
                run()  # tuning, allocation, lazily packed operands
            err = max(float(np.abs(e - g).max() / (np.abs(g).max() + 1e-30))
                      for e, g in zip(scores["engine"], scores["generic"]))
            t = {s: [] for s in sides}
            for _ in range(a.rounds):
                for s, run in sides.items():
                    t[s].append(timed_run(run))
            med = {s: float(np.median(v)) for s, v in t.items()}
            spread = {s: (max(v) - min(v)) / med[s] * 100 for s, v in t.items()}
            emit(f"{'pruned' if pruned else 'dense ':6s} MobileNetV2 {name:6s} {len(mods)} layers, {a.batches} x B={a.batch} "
                 f"{a.px}px, {a.rounds} alternating rounds: engine {n / med['engine']:8.0f} img/s (spread "
                 f"{spread['engine']:4.1f}%)  generic {n / med['generic']:8.0f} img/s (spread {spread['generic']:4.1f}%)  "
                 f"engine/generic {med['generic'] / med['engine']:.2f}x  max rel. score difference {err:.1e}")
        del model
        torch.cuda.empty_cache()


def kernel_cases(B):
    dev = torch.device("cuda")
    T = ops.require()
    for C0, H, s in SHAPES:
        C = cpad(C0)
        g = torch.Generator().manual_seed(C0)
        z = (torch.randn(B, H, H, C, generator=g) * 4 + 3).to(dev)
        w = torch.zeros(C, 1, 3, 3)
        w[:C0] = torch.randn(C0, 1, 3, 3, generator=g) * 0.4
        sc, sh = torch.zeros(C), torch.zeros(C)
        sc[:C0], sh[:C0] = torch.rand(C0, generator=g) + 0.5, torch.rand(C0, generator=g) * 3
        w, sc, sh = w.to(dev), sc.to(dev), sh.to(dev)
        Ho = (H + 2 - 3) // s + 1
        gr = torch.randn(B, Ho, Ho, C, device=dev)
        y = T.dwconv_act_fwd(z, w, sc, sh, s, 1, 2, 2)
        R = T.dwconv_act_tay_slots(H, H, C)
        tay = torch.zeros(R, B, C, device=dev)
        fwd = lambda z=z, w=w, sc=sc, sh=sh, s=s: T.dwconv_act_fwd(z, w, sc, sh, s, 1, 2, 2)
        bwd = lambda gr=gr, y=y, w=w, sc=sc, z=z, H=H, s=s, tay=tay: T.dwconv_act_dgrad(gr, y, w, sc, z, H, H, s, 1, 2,
                                                                                        2, tay, 0)
        yield (C0, C, H, s, R), fwd, (z.numel() + y.numel()) * 4, bwd, (2 * y.numel() + 2 * z.numel()) * 4


def per_kernel(a, emit):
    def timed(fn, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / iters * 1e-3

    emit(f"# per kernel (device events, min of 3 windows; in_act = out_act = ReLU6, dgrad with Taylor partials), B={a.batch}")
    for (C0, C, H, s, R), fwd, fb, bwd, bb in kernel_cases(a.batch):
        iters = max(3, min(50, int(2e9 / fb)))
        for fn in (fwd, bwd):
            fn()
        tf = min(timed(fwd, iters) for _ in range(3))
        tb = min(timed(bwd, iters) for _ in range(3))
        emit(f"C={C0:4d} (run at {C:4d}) {H:3d}x{H:<3d} s{s}  fwd {tf * 1e6:7.1f} us {fb / tf / COPY_RATE * 100:5.1f}%  "
             f"dgrad+tay {tb * 1e6:7.1f} us {bb / tb / COPY_RATE * 100:5.1f}%  (slab slots {R})")


def trace_kernels(a):
    """Only the launches: TRACE_ITERS x forward, then TRACE_ITERS x dgrad, shape by shape in table order."""
    for _, fwd, _, bwd, _ in kernel_cases(a.batch):
        for fn in (fwd, bwd):
            for _ in range(TRACE_ITERS):
                fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--px", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "mobilenet", "attr_engine_vs_generic.txt"))
    ap.add_argument("--trace-kernels", action="store_true", help="only the kernel launches (program of a rocprofv3 run)")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mobilenet_attr_probe needs a GPU: nothing is measured without one")
    if a.trace_kernels:
        trace_kernels(a)
        return
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit(f"# mobilenet_attr_probe: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, fp32; engine = "
         f"mobilenet_engine=True, generic = the same build with the engine off (the default); device events")
    if not a.kernels_only:
        end_to_end(a, emit)
    per_kernel(a, emit)
    out.close()


if __name__ == "__main__":
    main()
