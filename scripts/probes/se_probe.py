"""Probe: the native squeeze-and-excitation gate (tpamd.se_*, engine.train._NativeSE) against the
module's own forward (ATen pool, 1x1 convs, ReLU, Hardsigmoid, broadcast multiply: what
TORCHPRUNER_NATIVE_SE=0 leaves a gate on), on every distinct gate shape of MobileNetV3 small and
large at B=128 / 224 px, each also with the width cut by 30 % + 1 (no multiple of 4).

Per shape, in one process: forward + backward of the gate (input, weight and bias gradients) on
both paths in alternating rounds timed with device events, and the native kernels alone with the
bytes/s of the activation passes (forward 3: pool read, scale read + write; backward 4:
product-reduce reads g and x, dx reads g and writes) against the 6.29 TB/s measured copy rate. The
spread is (max - min) / median over a side's own rounds. Last, one whole training step of
mobilenet_v3_large, default against gates on the library path, in alternating rounds.

    python scripts/probes/se_probe.py [--batch 128] [--out profiles/se/se_vs_library.txt]
    python scripts/probes/se_probe.py --step-only [--step-out profiles/se/mobilenet_v3_step.txt]
    python scripts/probes/se_probe.py --trace 3     (under rocprofv3 --kernel-trace --stats: native gates only)
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

from torchpruner_amd import ops  # noqa: E402
from torchpruner_amd.engine import train  # noqa: E402
from torchpruner_amd.models import mobilenet_v3_large  # noqa: E402
from torchpruner_amd.models.mobilenet import _make_divisible  # noqa: E402
from torchpruner_amd.models.mobilenet_v3 import SqueezeExcitation  # noqa: E402

COPY_RATE = 6.29e12  # measured device copy rate, bytes/s
# (C, H = W) of the gates of MobileNetV3 small and large at 224 px
SHAPES = [(16, 56), (72, 28), (120, 28), (96, 14), (120, 14), (144, 14), (240, 14), (480, 14), (672, 14), (288, 7),
          (576, 7), (672, 7), (960, 7)]


def cut(c):
    return c - int(c * 0.3) - 1


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms


def gate_pair(C, Cs, H, B):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    lib = SqueezeExcitation(C, Cs).to(dev)
    nat = copy.deepcopy(lib)
    assert nat in train.enable_native_convs(nat), "gate not switched to the native kernels"
    x = torch.randn(B, C, H, H, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    g = torch.randn(B, C, H, H, device=dev).contiguous(memory_format=torch.channels_last)

    def run(m):
        def f():
            x.grad = None
            for p in m.parameters():
                p.grad = None
            m(x).backward(g)
        return f
    return lib, nat, x, g, run


def probe_shape(C, Cs, H, B, rounds, emit):
    T = ops.require()
    lib_m, nat_m, x, g, run = gate_pair(C, Cs, H, B)
    nat, lib = run(nat_m), run(lib_m)
    before = train.SE_COUNTS["fwd"]
    for f in (nat, lib):
        for _ in range(3):
            f()
    assert train.SE_COUNTS["fwd"] - before == 3
    act = B * C * H * H * 4
    iters = max(3, min(50, int(2e9 / (act * 7))))  # a timed window of tens of ms
    tn, tl = [], []
    for _ in range(rounds):
        tn.append(timed(nat, iters))
        tl.append(timed(lib, iters))
    xh, gh = x.detach().permute(0, 2, 3, 1), g.permute(0, 2, 3, 1)
    w1, b1, w2, b2 = (t.detach() for t in (lib_m.fc1.weight, lib_m.fc1.bias, lib_m.fc2.weight, lib_m.fc2.bias))
    p = T.se_pool(xh)
    h, s = T.se_gate_fwd(p, w1, b1, w2, b2, 0)
    ds = T.se_bwd_reduce(gh, xh)
    dz2, dz1, dp = T.se_gate_bwd(ds, s, h, w1, w2, 0)
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    kern = {"pool": (lambda: T.se_pool(xh), 1), "gate_fwd": (lambda: T.se_gate_fwd(p, w1, b1, w2, b2, 0), 0),
            "scale": (lambda: T.se_scale(xh, s), 2), "bwd_reduce": (lambda: T.se_bwd_reduce(gh, xh), 2),
            "gate_bwd": (lambda: T.se_gate_bwd(ds, s, h, w1, w2, 0), 0), "bwd_dx": (lambda: T.se_bwd_dx(gh, s, dp), 2),
            "wgrad": (lambda: (T.se_wgrad(dz1, p, dw1, True), T.se_wgrad(dz2, h, dw2, True)), 0)}
    ks, tot = [], 0.0
    for name, (fn, passes) in kern.items():
        fn()
        ms = min(timed(fn, iters) for _ in range(3))
        tot += ms
        pct = f" {passes * act / (ms * 1e-3) / COPY_RATE * 100:5.1f}%" if passes else ""
        ks.append(f"{name} {ms * 1e3:6.1f} us{pct}")
    mn, ml = float(np.median(tn)), float(np.median(tl))
    sn, sl = (max(tn) - min(tn)) / mn, (max(tl) - min(tl)) / ml
    emit(f"C={C:4d} Cs={Cs:3d} {H:2d}x{H:<2d}  native {mn:7.3f} ms (spread {sn * 100:4.1f}%)  library {ml:7.3f} ms "
         f"(spread {sl * 100:4.1f}%)  lib/nat {ml / mn:5.2f}x  kernels {tot:6.3f} ms = {7 * act / (tot * 1e-3) / COPY_RATE * 100:4.1f}% "
         f"of 7 passes at the copy rate | {' | '.join(ks)}")
    return mn, ml, sn, sl


def probe_step(B, rounds, emit):
    """One training step of mobilenet_v3_large (224 px, SGD momentum), every other module native on
    both sides: gates on the native kernels (the default) against gates on the library path."""
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = mobilenet_v3_large(1000).to(dev).to(memory_format=torch.channels_last).train()
    x = torch.randn(B, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (B,), device=dev)
    steps = {}
    for name, flag in (("native", True), ("library", False)):
        m = copy.deepcopy(model)
        keep, train._NATIVE_SE = train._NATIVE_SE, flag
        train.enable_native_convs(m)
        train._NATIVE_SE = keep
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, fused=True)

        def step(m=m, opt=opt):
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(m(x), y).backward()
            opt.step()
        steps[name] = step
    for f in steps.values():
        for _ in range(2):
            f()
    t = {n: [] for n in steps}
    for _ in range(rounds):
        for n, f in steps.items():
            t[n].append(timed(f, 3))
    med = {n: float(np.median(v)) for n, v in t.items()}
    spread = {n: (max(v) - min(v)) / med[n] * 100 for n, v in t.items()}
    emit(f"mobilenet_v3_large step B={B} 224px, {rounds} alternating rounds of 3 steps: gates native "
         f"{med['native']:.2f} ms (spread {spread['native']:.1f}%)  gates on the library path {med['library']:.2f} ms "
         f"(spread {spread['library']:.1f}%)  library/native {med['library'] / med['native']:.3f}x")
    return med, spread


def trace(B, n):
    """Forward + backward of the native gate on every shape, n times each, and nothing else: the
    program of a ``rocprofv3 --kernel-trace --stats`` run."""
    for C0, H in SHAPES:
        for C in (C0, cut(C0)):
            _, nat_m, x, g, run = gate_pair(C, _make_divisible(C0 // 4, 8), H, B)
            f = run(nat_m)
            for _ in range(n):
                f()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=400.0, help="seconds after which remaining shapes are skipped")
    ap.add_argument("--out", default=os.path.join("profiles", "se", "se_vs_library.txt"))
    ap.add_argument("--step-out", default=os.path.join("profiles", "se", "mobilenet_v3_step.txt"))
    ap.add_argument("--step-only", action="store_true", help="only the whole-step comparison")
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0, help="run the native gates this many times per shape and exit")
    a = ap.parse_args()
    if a.trace:
        trace(a.batch, a.trace)
        return

    def writer(path):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        f = open(path, "w")

        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        return emit

    head = f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, B={a.batch}, fp32 channels_last"
    if not a.step_only:
        emit = writer(a.out)
        t0 = time.perf_counter()
        emit(f"# se_probe: {head}; SqueezeExcitation forward + backward (dx, dW, db), median of {a.rounds} alternating "
             f"rounds, device events; kernel % = bytes/s of the activation passes against {COPY_RATE / 1e12:.2f} TB/s")
        tot_n = tot_l = worst = 0.0
        loses = []
        for C0, H in SHAPES:
            for C in (C0, cut(C0)):
                if time.perf_counter() - t0 > a.budget:
                    emit(f"C={C} {H}x{H}: skipped (time budget)")
                    continue
                mn, ml, sn, sl = probe_shape(C, _make_divisible(C0 // 4, 8), H, a.batch, a.rounds, emit)
                tot_n, tot_l, worst = tot_n + mn, tot_l + ml, max(worst, sn)
                if mn > ml:
                    loses.append((C, H, mn / ml))
                torch.cuda.empty_cache()
        emit(f"sum over shapes: native {tot_n:.2f} ms  library {tot_l:.2f} ms  lib/nat {tot_l / max(tot_n, 1e-9):.2f}x  "
             f"(largest spread of a native side {worst * 100:.1f}%)")
        emit("shapes where native loses: " + (", ".join(f"C={c} {h}x{h} ({r:.2f}x)" for c, h, r in loses) or "none"))
    emit_step = writer(a.step_out)
    emit_step(f"# se_probe whole step: {head}, SGD momentum (fused optimizer); median ms per step, device events")
    probe_step(a.batch, a.step_rounds, emit_step)


if __name__ == "__main__":
    main()
