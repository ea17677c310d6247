"""Probe: the fused BatchNorm + Hardswish unit tails (engine.train.bn_hswish, tpamd.bn_hswish_fwd /
bn_hswish_bwd) against the unfused path (the native BN followed by ATen's hardswish: what
TORCHPRUNER_FUSE_HSWISH=0 leaves, the path before the fusion existed) on one whole training step of
mobilenet_v3_large and mobilenet_v3_small: B=128, 224 px, fp32 channels_last, fused SGD with momentum,
dense and with every hidden width cut by 30 % + 1.

One process, same build: the switch (train._HS_FUSE) is read at every Sequential forward, so the two
sides are two copies of one model stepped in alternating rounds, timed with device events after a
warm-up (the tuner's one-off timings included), each timed window 10 steps (0.1 s or more). Per side the median over the rounds and the spread
(max - min) / median of its own rounds. The rule for the default: the fusion is on by default only
if it is ahead by more than the other side's spread in every configuration.

    python scripts/probes/hswish_probe.py [--batch 128] [--rounds 9] [--steps 10] [--out profiles/hswish/mobilenet_v3_step.txt]
    python scripts/probes/hswish_probe.py --trace 20 [--trace-shape stem|wide]
                                (under rocprofv3 --kernel-trace --stats: the three new kernels on one shape, nothing else timed)
    python scripts/probes/hswish_probe.py --stats-csv DIR/..._kernel_stats.csv [--trace-shape ...] [--append]
                                [--stats-out profiles/hswish/hswish_kernel_stats.txt]
                                (that run's per-kernel times as bytes/s against the copy rate)
"""
import argparse
import copy
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

COPY_RATE = 6.29e12  # measured device copy rate, bytes/s
# the traced shapes (B, H, W, C), one per trace run (--trace-shape): the stem unit's tail of
# mobilenet_v3_large at B=128 / 224 px, the largest activation a fused pair sees (25.7 M elements, 103 MB, a
# quarter of the statistics kernels' column lanes busy at C = 16), and its widest 14-pixel unit
TRACE_SHAPES = {"stem": (128, 112, 112, 16), "wide": (128, 14, 14, 672)}
# activation passes of each new kernel (reads + writes of a (P, C) fp32 activation)
PASSES = {"bn_hswish_partial<": 2, "bn_hswish_apply<false>": 2, "bn_hswish_apply<true>": 3, "bn_partial<0": 1}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms


def build(name, pruned):
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    from torchpruner_amd import models
    torch.manual_seed(0)
    model = getattr(models, name)(1000)
    if pruned:
        rng = np.random.RandomState(0)
        pruner = Pruner(model, (3, 64, 64), "cpu")
        for module, cascade in get_mobilenet_pruning_graph(model):
            n = module.weight.shape[0]
            pruner.prune_model(module, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    return model


def probe_step(name, pruned, B, rounds, per, emit):
    from torchpruner_amd.engine import train
    dev = torch.device("cuda")
    base = build(name, pruned).to(dev).to(memory_format=torch.channels_last).train()
    x = torch.randn(B, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (B,), device=dev)
    steps, counts = {}, {}
    for side, flag in (("fused", True), ("unfused", False)):
        m = copy.deepcopy(base)
        train.enable_native_convs(m)
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, fused=True)

        def step(m=m, opt=opt, flag=flag):
            train._HS_FUSE = flag
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(m(x), y).backward()
            opt.step()
        steps[side] = step
    keep = train._HS_FUSE
    try:
        for side, f in steps.items():
            before = train.FUSE_COUNTS["bn_hswish"]
            for _ in range(3):
                f()
            counts[side] = (train.FUSE_COUNTS["bn_hswish"] - before) // 3
        assert counts["fused"] > 0 and counts["unfused"] == 0, counts
        t = {n: [] for n in steps}
        for _ in range(rounds):
            for n, f in steps.items():
                t[n].append(timed(f, per))
    finally:
        train._HS_FUSE = keep
    med = {n: float(np.median(v)) for n, v in t.items()}
    spread = {n: (max(v) - min(v)) / med[n] * 100 for n, v in t.items()}
    gain = (med["unfused"] / med["fused"] - 1) * 100
    ahead = gain > spread["unfused"]
    emit(f"{name} {'pruned 30%+1' if pruned else 'dense':12s} {counts['fused']:2d} fused pairs: fused {med['fused']:7.2f} ms "
         f"(spread {spread['fused']:4.1f}%)  unfused {med['unfused']:7.2f} ms (spread {spread['unfused']:4.1f}%)  "
         f"unfused/fused {med['unfused'] / med['fused']:.3f}x  ahead by {gain:+.1f}% "
         f"{'>' if ahead else '<='} the unfused side's spread")
    del steps
    torch.cuda.empty_cache()
    return ahead


def trace(n, shape):
    """The fused forward and backward on one shape, n times, and nothing else."""
    from torchpruner_amd import ops
    T = ops.require()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    C = shape[-1]
    x, g = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    for _ in range(n):
        y, mean, invstd, ab = T.bn_hswish_fwd(x, gamma, beta, None, None, 1e-3, 0.01)
        T.bn_hswish_bwd(g, x, gamma, mean, invstd, ab, True)
    torch.cuda.synchronize()


def summarise(path, shape, emit):
    rows = list(csv.DictReader(open(path)))
    act = 4 * int(np.prod(shape))
    emit(f"# rocprofv3 --kernel-trace --stats -- python scripts/probes/hswish_probe.py --trace N (a run of its own): "
         f"tpamd.bn_hswish_fwd + bn_hswish_bwd on {shape} fp32 ({act / 1e6:.0f} MB per activation pass), "
         f"bytes/s against the {COPY_RATE / 1e12:.2f} TB/s copy rate")
    emit(f"{'calls':>6} {'avg_us':>9} {'passes':>6} {'TB/s':>6} {'of copy':>8}  kernel")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"]
        if "tp::" not in name:
            continue
        avg = float(r["TotalDurationNs"]) / max(1, int(r["Calls"])) * 1e-9
        passes = next((p for k, p in PASSES.items() if k in name.replace(" ", "")), 0)
        short = name.split("(")[0][:70]
        if passes:
            rate = passes * act / avg
            emit(f"{r['Calls']:>6} {avg * 1e6:9.1f} {passes:6d} {rate / 1e12:6.2f} {rate / COPY_RATE * 100:7.1f}%  {short}")
        else:
            emit(f"{r['Calls']:>6} {avg * 1e6:9.1f} {'-':>6} {'-':>6} {'-':>8}  {short}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window (0.1 s or more of work)")
    ap.add_argument("--out", default=os.path.join("profiles", "hswish", "mobilenet_v3_step.txt"))
    ap.add_argument("--trace", type=int, default=0, help="run the fused kernels this many times on one shape and exit")
    ap.add_argument("--trace-shape", default="stem", choices=sorted(TRACE_SHAPES))
    ap.add_argument("--append", action="store_true", help="append to --stats-out instead of replacing it")
    ap.add_argument("--stats-csv", default=None, help="summarise this rocprofv3 kernel_stats.csv and exit")
    ap.add_argument("--stats-out", default=os.path.join("profiles", "hswish", "hswish_kernel_stats.txt"))
    a = ap.parse_args()
    if a.trace:
        trace(a.trace, TRACE_SHAPES[a.trace_shape])
        return

    def writer(path, mode="w"):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        f = open(path, mode)

        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        return emit

    if a.stats_csv:
        summarise(a.stats_csv, TRACE_SHAPES[a.trace_shape], writer(a.stats_out, "a" if a.append else "w"))
        return
    emit = writer(a.out)
    emit(f"# hswish_probe: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, B={a.batch}, 224 px, fp32 "
         f"channels_last, SGD momentum (fused optimizer); one training step, median ms of {a.rounds} alternating rounds "
         f"of {a.steps} steps, device events; fused = BN + Hardswish pairs on tpamd.bn_hswish_*, unfused = "
         f"TORCHPRUNER_FUSE_HSWISH=0 (native BN, ATen hardswish)")
    ahead = [probe_step(name, pruned, a.batch, a.rounds, a.steps, emit)
             for name in ("mobilenet_v3_large", "mobilenet_v3_small") for pruned in (False, True)]
    emit(f"fused ahead by more than the unfused side's spread in {sum(ahead)} of {len(ahead)} configurations: "
         f"default {'on' if all(ahead) else 'off'} by the project's rule")


if __name__ == "__main__":
    main()
