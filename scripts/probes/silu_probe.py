"""Probe: the fused BatchNorm + SiLU unit tails and the SiLU gates (engine.train.bn_silu, _NativeSE with a
SiLU inner activation) on EfficientNet, modelled on hswish_probe.py.

--kernels: the backward of tpamd.bn_silu_bwd on (128, 56, 56, 96) and (128, 7, 7, 1152) fp32, device
events: the statistics kernel + finalize (want_dx=False), the apply kernel (the full backward minus
that) and a same-size copy (y.copy_(x): one read, one write), each the median of alternating rounds
with its spread (max - min) / median.

--step (default): one whole training step of efficientnet(0.25, 0.34, small_input) at 32 px and of
efficientnet_b0 at 224 px, B=128, fp32 channels_last, fused SGD with momentum: fused (BN + SiLU tails,
native gates) against unfused (TORCHPRUNER_FUSE_SILU=0 TORCHPRUNER_NATIVE_SE=0: native BN, ATen silu,
the gate modules' own forwards), two copies of one model stepped in alternating rounds in one process.

    python scripts/probes/silu_probe.py [--batch 128] [--rounds 9] [--steps 10] [--out profiles/silu/efficientnet_step.txt]
    python scripts/probes/silu_probe.py --kernels [--out profiles/silu/silu_kernel_probe.txt]
"""
import argparse
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hswish_probe import timed  # noqa: E402

KERNEL_SHAPES = [(128, 56, 56, 96), (128, 7, 7, 1152)]


def med_spread(v):
    m = float(np.median(v))
    return m, (max(v) - min(v)) / m * 100


def probe_kernels(rounds, iters, emit):
    from torchpruner_amd import ops
    T = ops.require()
    dev = torch.device("cuda")
    for shape in KERNEL_SHAPES:
        torch.manual_seed(0)
        C = shape[-1]
        x, g = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        y, mean, invstd, ab = T.bn_silu_fwd(x, gamma, beta, None, None, 1e-3, 0.01)
        sides = {"copy": lambda: y.copy_(x),
                 "statistics": lambda: T.bn_silu_bwd(g, x, gamma, mean, invstd, ab, False),
                 "statistics+apply": lambda: T.bn_silu_bwd(g, x, gamma, mean, invstd, ab, True)}
        t = {k: [] for k in sides}
        for f in sides.values():
            timed(f, 3)
        for _ in range(rounds):
            for k, f in sides.items():
                t[k].append(timed(f, iters) * 1e3)  # us
        copy_us = med_spread(t["copy"])[0]
        emit(f"shape {shape} fp32, {4 * x.numel() / 1e6:.0f} MB per activation pass; median us of {rounds} alternating "
             f"rounds of {iters} calls (spread), against the copy (2 passes)")
        for k, v in t.items():
            m, s = med_spread(v)
            emit(f"  {k:28s} {m:9.1f} us ({s:4.1f}%)  {m / copy_us:5.2f} x copy")
        m, s = med_spread(list(np.array(t["statistics+apply"]) - np.array(t["statistics"])))
        emit(f"  {'apply (difference)':28s} {m:9.1f} us ({s:4.1f}%)  {m / copy_us:5.2f} x copy (3 passes)")


def probe_step(name, model, px, B, rounds, per, emit):
    from torchpruner_amd.engine import train
    dev = torch.device("cuda")
    base = model.to(dev).to(memory_format=torch.channels_last).train()
    x = torch.randn(B, 3, px, px, device=dev).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (B,), device=dev)
    steps, counts = {}, {}
    keep = (train._SILU_FUSE, train._NATIVE_SE)
    try:
        for side, flag in (("fused", True), ("unfused", False)):
            m = copy.deepcopy(base)
            train._NATIVE_SE = flag  # consulted when the forwards are installed
            train.enable_native_convs(m)
            opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, fused=True)

            def step(m=m, opt=opt, flag=flag):
                train._SILU_FUSE = flag  # consulted at every Sequential forward
                opt.zero_grad(set_to_none=True)
                F.cross_entropy(m(x), y).backward()
                opt.step()
            steps[side] = step
        for side, f in steps.items():
            before = train.FUSE_COUNTS["bn_silu"], train.SE_COUNTS["fwd"]
            for _ in range(3):
                f()
            counts[side] = ((train.FUSE_COUNTS["bn_silu"] - before[0]) // 3, (train.SE_COUNTS["fwd"] - before[1]) // 3)
        assert min(counts["fused"]) > 0 and counts["unfused"] == (0, 0), counts
        t = {n: [] for n in steps}
        for _ in range(rounds):
            for n, f in steps.items():
                t[n].append(timed(f, per))
    finally:
        train._SILU_FUSE, train._NATIVE_SE = keep
    (mf, sf), (mu, su) = med_spread(t["fused"]), med_spread(t["unfused"])
    gain = (mu / mf - 1) * 100
    emit(f"{name:34s} {px:3d} px  {counts['fused'][0]:2d} fused pairs, {counts['fused'][1]:2d} gates: fused {mf:7.2f} ms "
         f"(spread {sf:4.1f}%)  unfused {mu:7.2f} ms (spread {su:4.1f}%)  unfused/fused {mu / mf:.3f}x  ahead by "
         f"{gain:+.1f}% {'>' if gain > su else '<='} the unfused side's spread")
    del steps
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10, help="steps (--kernels: calls) per timed window")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join("profiles", "silu", "silu_kernel_probe.txt" if a.kernels else "efficientnet_step.txt")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    f = open(out, "w")

    def emit(line):
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    head = f"# silu_probe: {torch.cuda.get_device_name(0)}, torch {torch.__version__}"
    if a.kernels:
        emit(head + "; tpamd.bn_silu_bwd, device events")
        probe_kernels(a.rounds, a.steps, emit)
        return
    from torchpruner_amd.models import efficientnet, efficientnet_b0
    emit(head + f", B={a.batch}, fp32 channels_last, SGD momentum (fused optimizer); one training step, median ms of "
         f"{a.rounds} alternating rounds of {a.steps} steps, device events; fused = BN + SiLU pairs on tpamd.bn_silu_* "
         f"and SiLU gates on tpamd.se_*, unfused = TORCHPRUNER_FUSE_SILU=0 TORCHPRUNER_NATIVE_SE=0")
    torch.manual_seed(0)
    probe_step("efficientnet(0.25, 0.34, small_input)", efficientnet(0.25, 0.34, 10, True), 32, a.batch, a.rounds, a.steps, emit)
    probe_step("efficientnet_b0", efficientnet_b0(10), 224, a.batch, a.rounds, a.steps, emit)


if __name__ == "__main__":
    main()
