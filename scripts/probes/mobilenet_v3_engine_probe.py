"""Probe: APoZ and Taylor over all blocks of mobilenet_v3_small and mobilenet_v3_large on the MobileNet
attribution engine (``mobilenet_engine=True``: engine/mobilenet_engine.py, MobileNetV3Engine) against
the generic hook path (``mobilenet_engine=False``), same build, one GPU, one process: B=128, 224 px,
fp32, eval mode, one resident batch per run.

The two paths alternate round by round and are timed with device events after a warm-up of both (the
tuner's one-off timings and the first launches included). A timed window is ``--runs`` metric runs.
Per path the median over the rounds and the spread (max - min) / median of its own rounds. No target
is set; the engine stays opt-in whatever the result.

    python scripts/probes/mobilenet_v3_engine_probe.py [--batch 128] [--rounds 7] [--runs 3]
                                                       [--out profiles/mobilenet_v3/engine_vs_generic.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms


def live_model(name, dev):
    """The net in eval mode with BN statistics that keep every activation branch busy (weight ~
    U(0.75, 1.75), bias ~ U(0, 2), running_mean ~ N(0, 0.2), running_var ~ U(0.5, 1.5))."""
    from torchpruner_amd import models
    torch.manual_seed(0)
    model = getattr(models, name)(1000).eval()
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_(torch.rand(n, generator=gen) + 0.75)
                m.bias.copy_(torch.rand(n, generator=gen) * 2)
                m.running_mean.copy_(torch.randn(n, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(n, generator=gen) + 0.5)
    return model.to(dev)


def convs_of(model):
    from torchpruner_amd import get_mobilenet_pruning_graph
    expand = [m for m, _ in get_mobilenet_pruning_graph(model)]
    dw = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups != 1]
    return expand + [c for c in dw if not any(c is e for e in expand)]


def probe(name, B, rounds, runs, emit):
    from torchpruner_amd import APoZAttributionMetric, TaylorAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    dev = torch.device("cuda")
    model = live_model(name, dev)
    convs = convs_of(model)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, 1000, (B,), generator=g).to(dev)
    for label, cls in (("apoz", APoZAttributionMetric), ("taylor", TaylorAttributionMetric)):
        sides, results = {}, {}
        for side, flag in (("engine", True), ("generic", False)):
            metric = cls(model, DeviceLoader(x, y, B), F.cross_entropy, dev, mobilenet_engine=flag)

            def run(metric=metric, side=side):
                results[side] = metric.run_many(convs, find_best_evaluation_module=True)
            run()
            want = "mobilenet" if flag else "generic"
            assert metric.last_path["path"] == want, metric.last_path
            run()  # warm-up: the tuner has chosen, every code object is loaded
            sides[side] = run
        torch.cuda.synchronize()
        worst = max(float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
                    for a, b in zip(results["engine"], results["generic"]))
        times = {s: [] for s in sides}
        for _ in range(rounds):
            for s, fn in sides.items():  # alternate
                times[s].append(timed(fn, runs))
        med = {s: float(np.median(t)) for s, t in times.items()}
        spread = {s: (max(t) - min(t)) / med[s] for s, t in times.items()}
        emit(f"{name:20s} {label:7s} B={B} {len(convs)} layers: engine {med['engine']:8.2f} ms (spread "
             f"{100 * spread['engine']:4.1f} %), generic {med['generic']:8.2f} ms (spread {100 * spread['generic']:4.1f} %), "
             f"generic / engine {med['generic'] / med['engine']:5.2f}x; max |engine - generic| / max |generic| per layer "
             f"<= {worst:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--nets", default="mobilenet_v3_small,mobilenet_v3_large")
    ap.add_argument("--out", default="profiles/mobilenet_v3/engine_vs_generic.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mobilenet_v3_engine_probe: needs a GPU (nothing is measured without one)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; one process, paths alternating, device events; "
         f"{a.rounds} rounds of {a.runs} runs per path after warm-up; median (spread = (max - min) / median)")
    for name in a.nets.split(","):
        probe(name, a.batch, a.rounds, a.runs, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
