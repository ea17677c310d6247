"""Probe: the LDS-staged SiLU depthwise kernels (``tpamd.dwconv_silu_fwd`` / ``dwconv_silu_dgrad``,
csrc/kernels/dwconv_silu.hip) on EfficientNet-B0's depthwise layers (B=32 at 224 px, and the 14- and
7-pixel ones again at B=8), against the per-row-activating kernels of dwconv_act.hip run with
Hardswish on both sides (``dwconv_hs_fwd`` / ``dwconv_hs_dgrad``, codes (3, 3), ``pre`` and the score
slab): code that moves the same bytes, so it is the yardstick. Forwards write y and pre; the staged
forward also writes the pool partials (which saves the engine an ``se_pool`` pass the yardstick does
not pay here either).

Rate: the bytes one pass must move (forward x + y + pre, backward g + pre + z + dz) over the 6.29 TB/s
copy rate. The two kernels alternate round by round, timed with device events after a warm-up; a
timed window is as many launches as fill ``--window`` seconds (sized per shape from a first timing of
the staged kernel, the same count for both kernels: thousands of launches on the small maps); per
kernel the median over the rounds and the spread (max - min) / median.

    python scripts/probes/dwconv_silu_probe.py [--rounds 7] [--window 0.2] [--out profiles/silu/dwconv_silu_kernels.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY = 6.29e12
# (C padded to 32 as the engine carries it, input size, k, stride) of B0's depthwise layers at 224 px
B0_DW = [(32, 112, 3, 1), (96, 112, 3, 2), (160, 56, 3, 1), (160, 56, 5, 2), (256, 28, 5, 1), (256, 28, 3, 2),
         (480, 14, 3, 1), (480, 14, 5, 1), (672, 14, 5, 1), (672, 14, 5, 2), (1152, 7, 5, 1), (1152, 7, 3, 1)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e-3  # s


def probe(B, C, HW, k, s, rounds, window, emit):
    from torchpruner_amd import ops
    T = ops.require()
    dev, pad = torch.device("cuda"), k // 2
    g = torch.Generator().manual_seed(C + HW + k)
    z = (torch.randn(B, HW, HW, C, generator=g) * 2).to(dev)
    w = (torch.randn(C, 1, k, k, generator=g) / k).to(dev)
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    Ho = (HW + 2 * pad - k) // s + 1
    gr = torch.randn(B, Ho, Ho, C, generator=g).to(dev)
    pre, pre_h = torch.empty(B, Ho, Ho, C, device=dev), torch.empty(B, Ho, Ho, C, device=dev)
    pool = torch.zeros(T.dwconv_silu_pool_slots(Ho, Ho, C), B, C, device=dev)
    tay = torch.zeros(T.dwconv_silu_tay_slots(HW, HW, C), B, C, device=dev)
    tay_h = torch.zeros(T.dwconv_hs_tay_slots(HW, HW, C), B, C, device=dev)
    runs = {"fwd": (lambda: T.dwconv_silu_fwd(z, w, sc, sh, s, pad, 4, 4, None, pre, pool),
                    lambda: T.dwconv_hs_fwd(z, w, sc, sh, s, pad, 3, 3, None, pre_h)),
            "dgrad": (lambda: T.dwconv_silu_dgrad(gr, pre, w, sc, z, HW, HW, s, pad, 4, 4, tay, 0),
                      lambda: T.dwconv_hs_dgrad(gr, pre_h, w, sc, z, HW, HW, s, pad, 3, 3, tay_h, 0))}
    nbytes = {"fwd": 4 * (z.numel() + 2 * gr.numel()), "dgrad": 4 * (2 * gr.numel() + 2 * z.numel())}
    for name, pair in runs.items():
        for fn in pair:  # warm-up (and pre / pre_h for the dgrads)
            timed(fn, 20)
        iters = max(20, int(window / timed(pair[0], 50)))
        t = ([], [])
        for _ in range(rounds):
            for i, fn in enumerate(pair):  # alternate
                t[i].append(timed(fn, iters))
        med = [float(np.median(v)) for v in t]
        spread = [(max(v) - min(v)) / m for v, m in zip(t, med)]
        ratio = med[1] / med[0]
        noise = max(spread)
        verdict = "ahead" if ratio > 1 + noise else "behind" if ratio < 1 - noise else "level"
        emit(f"B={B:3d} C={C:5d} {HW:3d}x{HW:<3d} k{k} s{s} {name:5s}: staged {med[0] * 1e6:7.1f} us "
             f"{100 * nbytes[name] / med[0] / COPY:5.1f}% (spread {100 * spread[0]:4.1f}%)  per-row hs "
             f"{med[1] * 1e6:7.1f} us {100 * nbytes[name] / med[1] / COPY:5.1f}% (spread {100 * spread[1]:4.1f}%)  "
             f"hs / staged {ratio:4.2f}x  {verdict}  ({iters} launches)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of launches per timed window")
    ap.add_argument("--out", default="profiles/silu/dwconv_silu_kernels.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dwconv_silu_probe: needs a GPU (nothing is measured without one)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; kernels alternating, device events; {a.rounds} "
         f"rounds of {a.window:g} s windows per kernel after warm-up; median us, % of the 6.29 TB/s copy rate (fwd x + y + pre, "
         "dgrad g + pre + z + dz), spread = (max - min) / median; verdict: outside the larger spread or level")
    for C, HW, k, s in B0_DW:
        probe(32, C, HW, k, s, a.rounds, a.window, emit)
    for C, HW, k, s in B0_DW:
        if HW <= 14:
            probe(8, C, HW, k, s, a.rounds, a.window, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
