"""Probe: the native depthwise-conv kernels (tpamd.dwconv_*) against the library path
(F.conv2d on channels_last, what TORCHPRUNER_NATIVE_DW=0 leaves a depthwise conv on), on
MobileNetV2's depthwise shapes at B=128 / 224 px, each also cut by 30 % to a width that is no
multiple of 4.

Per shape, in one process: the first call of each path (after a prune every width is new: the
JIT / solver search the library pays), then forward + backward (dgrad + wgrad) of the module on
both paths in alternating rounds timed with device events, and the three native kernels alone
with their achieved bytes/s over the floor of one read and one write of the activation
(forward: x + y, dgrad: g + dx, wgrad: g + x) against the 6.29 TB/s measured copy rate. The
spread is what the native side's own rounds show. Last, one whole training step of MobileNetV2,
dense and pruned, three ways in alternating rounds: the default (fused BN + ReLU6 tails, carried
hidden widths, the inverted-residual block forward), the same build with those fusions off
(TORCHPRUNER_FUSE_RELU6=0's path) and with the depthwise convs on the library path; those lines also
go to --step-out.

    python scripts/probes/dwconv_probe.py [--batch 128] [--out profiles/dwconv/dwconv_vs_library.txt]
    python scripts/probes/dwconv_probe.py --step-only [--no-library] [--step-out profiles/dwconv/mobilenet_step_fused.txt]
    python scripts/probes/dwconv_probe.py --trace-steps 3 --variant fused|unfused   (under rocprofv3 --kernel-trace)
"""
import argparse
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from torchpruner_amd import Pruner, get_mobilenet_pruning_graph, ops  # noqa: E402
from torchpruner_amd.engine import train  # noqa: E402
from torchpruner_amd.models import mobilenet_v2  # noqa: E402

COPY_RATE = 6.29e12  # measured device copy rate, bytes/s
# (C, input H = W, stride) of MobileNetV2's 3x3 depthwise layers at 224 px
SHAPES = [(32, 112, 1), (96, 112, 2), (144, 56, 1), (144, 56, 2), (192, 28, 1), (192, 28, 2), (384, 14, 1),
          (576, 14, 1), (576, 14, 2), (960, 7, 1)]


def cut(c):
    c = c - int(c * 0.3) - 1
    return c - 1 if c % 4 == 0 else c


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms


def first_call(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def probe_shape(C, H, s, B, rounds, emit):
    dev = torch.device("cuda")
    T = ops.require()
    conv = torch.nn.Conv2d(C, C, 3, s, 1, groups=C, bias=False).to(dev).to(memory_format=torch.channels_last)
    x = torch.randn(B, C, H, H, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    Ho = (H + 2 - 3) // s + 1
    g = torch.randn(B, C, Ho, Ho, device=dev).contiguous(memory_format=torch.channels_last)

    conv_nat = copy.deepcopy(conv)
    assert train.enable_native_convs(conv_nat) == [conv_nat], "depthwise conv not switched to the native kernels"

    def run(m):
        def f():
            x.grad = m.weight.grad = None
            m(x).backward(g)
        return f

    nat, lib = run(conv_nat), run(conv)
    first = {"native": first_call(nat), "library": first_call(lib)}
    for f in (nat, lib):
        for _ in range(2):
            f()
    iters = max(3, min(50, int(2e9 / (B * C * H * H * 4 * 6))))  # a timed window of tens of ms
    tn, tl = [], []
    for _ in range(rounds):
        tn.append(timed(nat, iters))
        tl.append(timed(lib, iters))
    xh, gh, w = x.detach().permute(0, 2, 3, 1), g.permute(0, 2, 3, 1), conv.weight.detach()
    dw = torch.empty_like(w)
    kern = {"fwd": (lambda: T.dwconv_fwd(xh, w, None, s, 1), x.numel() + g.numel()),
            "dgrad": (lambda: T.dwconv_dgrad(gh, w, H, H, s, 1), x.numel() + g.numel()),
            "wgrad": (lambda: T.dwconv_wgrad(gh, xh, 3, s, 1, dw, False), x.numel() + g.numel())}
    ks = []
    for name, (fn, elems) in kern.items():
        fn()
        ms = min(timed(fn, iters) for _ in range(3))
        ks.append(f"{name} {ms * 1e3:7.1f} us {elems * 4 / (ms * 1e-3) / COPY_RATE * 100:5.1f}%")
    mn, ml = float(np.median(tn)), float(np.median(tl))
    spread = (max(tn) - min(tn)) / mn
    emit(f"C={C:4d} {H:3d}x{H:<3d} s{s}  native {mn:8.3f} ms  library {ml:8.3f} ms  lib/nat {ml / mn:5.2f}x  "
         f"spread {spread * 100:4.1f}%  first call native {first['native']:8.1f} ms library {first['library']:9.1f} ms"
         f"  | {' | '.join(ks)}")
    return mn, ml, spread, first


def step_model(B, pruned):
    """MobileNetV2 (224 px), dense or with every hidden width cut by 30 % + 1, and one batch."""
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = mobilenet_v2(1000).to(dev)
    if pruned:
        rng = np.random.RandomState(0)
        pruner = Pruner(model, (3, 224, 224), dev)
        for module, cascade in get_mobilenet_pruning_graph(model):
            n = module.weight.shape[0]
            pruner.prune_model(module, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    model = model.to(memory_format=torch.channels_last).train()
    x = torch.randn(B, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (B,), device=dev)
    return model, x, y


# variant -> (_NATIVE_DW, _MB_FUSE) while enable_native_convs installs the forwards
VARIANTS = {"fused": (True, True), "unfused": (True, False), "library": (False, True)}


def make_step(model, x, y, variant):
    m = copy.deepcopy(model)
    keep = train._NATIVE_DW, train._MB_FUSE
    train._NATIVE_DW, train._MB_FUSE = VARIANTS[variant]
    train.enable_native_convs(m)
    train._NATIVE_DW, train._MB_FUSE = keep
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, fused=True)

    def step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(m(x), y).backward()
        opt.step()
    return step


def probe_step(B, rounds, emit, pruned=True, library=True):
    """One training step of MobileNetV2 (224 px), dense or with every hidden width cut by 30 % + 1,
    dense convs native on every side: the fused default, the fusions off (the path before them:
    native BN then ATen hardtanh, hidden widths sliced, depthwise convs at their real width) and
    the depthwise convs on the library path. Alternating rounds, device events; each side's spread
    is (max - min) / median over its own rounds."""
    model, x, y = step_model(B, pruned)
    steps = {v: make_step(model, x, y, v) for v in VARIANTS if library or v != "library"}
    first = {n: first_call(f) for n, f in steps.items()}
    for f in steps.values():
        f()
    t = {n: [] for n in steps}
    for _ in range(rounds):
        for n, f in steps.items():
            t[n].append(timed(f, 3))
    med = {n: float(np.median(v)) for n, v in t.items()}
    spread = {n: (max(v) - min(v)) / med[n] * 100 for n, v in t.items()}
    what = "pruned" if pruned else "dense"
    line = (f"{what} MobileNetV2 step B={B} 224px, {rounds} alternating rounds of 3 steps: "
            f"fused {med['fused']:.2f} ms (spread {spread['fused']:.1f}%)  "
            f"unfused {med['unfused']:.2f} ms (spread {spread['unfused']:.1f}%)  "
            f"unfused/fused {med['unfused'] / med['fused']:.3f}x")
    if "library" in steps:
        line += (f"  depthwise on the library path {med['library']:.2f} ms (spread {spread['library']:.1f}%)  "
                 f"library/fused {med['library'] / med['fused']:.2f}x")
    line += "  first step " + " ".join(f"{n} {first[n] / 1e3:.1f} s" for n in steps)
    emit(line)
    return med, spread


def trace_steps(B, variant, n):
    """A few pruned steps of one variant and nothing else: the program of a
    ``rocprofv3 --kernel-trace --stats`` run (tuning and warm-up steps are part of the trace; the
    per-kernel summary is taken over all of them)."""
    model, x, y = step_model(B, True)
    step = make_step(model, x, y, variant)
    for _ in range(n):
        step()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=900.0, help="seconds after which remaining shapes are skipped")
    ap.add_argument("--out", default=os.path.join("profiles", "dwconv", "dwconv_vs_library.txt"))
    ap.add_argument("--step-out", default=os.path.join("profiles", "dwconv", "mobilenet_step_fused.txt"))
    ap.add_argument("--step-only", action="store_true", help="only the whole-step comparison")
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-library", action="store_true", help="whole step: leave the library-path variant out")
    ap.add_argument("--trace-steps", type=int, default=0, help="run this many pruned steps of --variant and exit")
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="fused")
    a = ap.parse_args()
    if a.trace_steps:
        trace_steps(a.batch, a.variant, a.trace_steps)
        return
    os.makedirs(os.path.dirname(a.step_out) or ".", exist_ok=True)
    step_out = open(a.step_out, "w")

    def emit_step(line):
        print(line, flush=True)
        for f in (step_out,) if a.step_only else (out, step_out):
            f.write(line + "\n")
            f.flush()

    def steps():
        emit_step(f"# dwconv_probe whole step: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, fp32 "
                  f"channels_last, SGD momentum (fused optimizer); fused = the default path, unfused = "
                  f"TORCHPRUNER_FUSE_RELU6=0's path in the same process; median ms per step, device events")
        for pruned in (False, True):
            probe_step(a.batch, a.step_rounds, emit_step, pruned=pruned, library=not a.no_library)
            torch.cuda.empty_cache()
        step_out.close()

    if a.step_only:
        steps()
        return
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    t0 = time.perf_counter()
    emit(f"# dwconv_probe: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, B={a.batch}, fp32 NHWC, 3x3 pad 1; "
         f"module forward + backward (dgrad + wgrad), median of {a.rounds} alternating rounds; kernel % = bytes/s over "
         f"one read + one write of the activation against {COPY_RATE / 1e12:.2f} TB/s")
    tot_n = tot_l = 0.0
    worst_spread, loses = 0.0, []
    first_n = first_l = 0.0
    for C0, H, s in SHAPES:
        for C in (C0, cut(C0)):
            if time.perf_counter() - t0 > a.budget:
                emit(f"C={C} {H}x{H} s{s}: skipped (time budget)")
                continue
            mn, ml, spread, first = probe_shape(C, H, s, a.batch, a.rounds, emit)
            tot_n, tot_l, worst_spread = tot_n + mn, tot_l + ml, max(worst_spread, spread)
            first_n, first_l = first_n + first["native"], first_l + first["library"]
            if mn > ml * (1 + spread):
                loses.append((C, H, s, mn / ml))
            torch.cuda.empty_cache()
    emit(f"sum over shapes: native {tot_n:.2f} ms  library {tot_l:.2f} ms  lib/nat {tot_l / max(tot_n, 1e-9):.2f}x  "
         f"(largest spread of a native side {worst_spread * 100:.1f}%); first calls summed: native {first_n / 1e3:.2f} s  "
         f"library {first_l / 1e3:.2f} s")
    emit("shapes where native loses by more than its spread: " +
         (", ".join(f"C={c} {h}x{h} s{s} ({r:.2f}x)" for c, h, s, r in loses) or "none"))
    if time.perf_counter() - t0 < a.budget:
        steps()
    else:
        emit("whole step: skipped (time budget)")
    out.close()


if __name__ == "__main__":
    main()
