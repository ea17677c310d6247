"""Probe: Shapley values on MobileNetV3 through the MobileNet engine (``mobilenet_engine=True``: a gated
block's prefixes on the channel-scaled project GEMM, ``ops.scaled_project``).

Project stage: ``MobileNetV3Engine.prefix_project_out`` with ``TORCHPRUNER_PREFIX_GATED=1`` (the kernel)
against ``=0`` (``torch.where`` + ``se_pool`` / ``se_gate_fwd`` / ``se_scale`` + the project conv on the
stacked copies) at the gated project shapes of ``mobilenet_v3_large(1000)`` at 224 px, one block per
distinct (C, Co, map), cnt = the metric's chunk; both sides run once first, then alternate in one process,
device events around the stage, median and spread = (max - min) / median of each side's own rounds. The
kernel counts as ahead only where its median is below the composed one's by more than the composed
side's spread.

End to end: ``sv_samples=2`` over every channel of the first, a middle and the last gated block's
post-depthwise activation of ``mobilenet_v3_large`` and ``mobilenet_v3_small``, engine on against the
``generic-hook`` path of the same build, image-evaluations/s from the median round (a report, no gate).

    python scripts/probes/mobilenet_v3_shapley_probe.py [--out profiles/mobilenet_v3/shapley_engine_vs_hook.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from torchpruner_amd import ShapleyAttributionMetric  # noqa: E402
from torchpruner_amd.data import DeviceLoader  # noqa: E402
from torchpruner_amd.engine import build_mobilenet_v3_plan, maybe_mobilenet_engine  # noqa: E402
from torchpruner_amd.models import mobilenet_v3_large, mobilenet_v3_small  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3  # s


def alternate(sides, rounds):
    """{side: (median s, spread %)} of callables run once untimed, then in alternating timed rounds."""
    for fn in sides.values():
        fn()
    t = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            t[s].append(timed(fn))
    return {s: (float(np.median(v)), (max(v) - min(v)) / float(np.median(v)) * 100) for s, v in t.items()}


def project_stage(a, emit):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = mobilenet_v3_large(1000).to(dev).eval()
    x = torch.randn(a.stage_batch, 3, a.px, a.px, device=dev)
    eng = maybe_mobilenet_engine(model, [], dev, shapley=True)
    emit(f"# project stage (prefix_project_out, device events, {a.rounds} alternating rounds), mobilenet_v3_large "
         f"{a.px}px B={a.stage_batch}, post-depthwise evaluation point, cnt = the metric's chunk")
    seen = set()
    for bi, blk in enumerate(eng.plan.blocks):
        if blk.gate is None:
            continue
        with torch.no_grad():
            h, y = eng.forward_to(x, bi)
        B, Ho, Wo, C = y.shape
        co = eng._pack()["blocks"][bi]["project"]["scale"].numel()
        if (C, co, Ho) in seen:
            continue
        seen.add((C, co, Ho))
        n = eng.real_width(blk.dw.act)
        cnt = max(1, min(n, (1 << 29) // (4 * B * eng.downstream_elems(bi, tuple(x.shape[1:])))))
        rank = torch.cat([torch.randperm(n), torch.full((C - n,), n + 1)]).to(torch.int32).to(dev)
        p0 = (n - cnt) // 2

        def side(flag, bi=bi, h=h, y=y, rank=rank, p0=p0, cnt=cnt):
            def run():
                os.environ["TORCHPRUNER_PREFIX_GATED"] = flag
                try:
                    with torch.no_grad():
                        eng.prefix_project_out(bi, "dw", h, y, rank, p0, cnt)
                finally:
                    del os.environ["TORCHPRUNER_PREFIX_GATED"]
            return run
        r = alternate({"kernel": side("1"), "composed": side("0")}, a.rounds)
        (tk, sk), (tc, scp) = r["kernel"], r["composed"]
        ahead = "kernel ahead by more than the composed spread" if (tc - tk) / tc * 100 > scp else \
            ("kernel behind" if tk > tc else "within the composed spread")
        emit(f"block {bi:2d} C={C:4d} Co={co:4d} map {Ho:2d}x{Wo:<2d} cnt={cnt:3d}:  kernel {tk * 1e6:8.1f} us (spread "
             f"{sk:4.1f}%)  composed {tc * 1e6:8.1f} us (spread {scp:4.1f}%)  composed/kernel {tc / tk:5.2f}x  ({ahead})")
    del model, eng
    torch.cuda.empty_cache()


def end_to_end(a, emit):
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, 3, a.px, a.px, generator=gen).to(dev)
    y = torch.randint(0, 1000, (a.batch,), generator=gen).to(dev)
    emit(f"# end to end (sv_samples=2, one batch of {a.batch} at {a.px}px, {a.rounds} alternating rounds), "
         "image-evaluations/s = prefix evaluations x images / median time")
    for mname, make in (("mobilenet_v3_large", mobilenet_v3_large), ("mobilenet_v3_small", mobilenet_v3_small)):
        torch.manual_seed(0)
        model = make(1000).to(dev).eval()
        gated = [b for b in build_mobilenet_v3_plan(model)[0].blocks if b.gate is not None]
        for name, blk in (("first ", gated[0]), ("middle", gated[len(gated) // 2]), ("last  ", gated[-1])):
            conv, evals = blk.dw.conv, {}

            def side(on, want, conv=conv, evals=evals):
                def run():
                    np.random.seed(11)
                    m = ShapleyAttributionMetric(model, DeviceLoader(x, y, a.batch), F.cross_entropy, dev, sv_samples=2,
                                                 mobilenet_engine=on)
                    m.run(conv, find_best_evaluation_module=True)
                    assert m.last_path["path"] == want, m.last_path
                    evals[want] = m.last_work["prefix_evals"]
                return run
            r = alternate({"engine": side(True, "mobilenet"), "generic-hook": side(False, "generic-hook")}, a.rounds)
            (te, se), (th, sh) = r["engine"], r["generic-hook"]
            lead = "exceeds" if (th / te - 1) * 100 > max(se, sh) else "within"
            emit(f"{mname} {name} gated block post-dw n={conv.weight.shape[0]:4d}:  engine {evals['mobilenet'] / te:9.0f} "
                 f"eval/s (spread {se:4.1f}%)  generic-hook {evals['generic-hook'] / th:9.0f} eval/s (spread {sh:4.1f}%)  "
                 f"engine/hook {th / te:6.2f}x ({lead} the spreads)")
        del model
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--stage-batch", type=int, default=32)
    ap.add_argument("--px", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "mobilenet_v3", "shapley_engine_vs_hook.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mobilenet_v3_shapley_probe needs a GPU: nothing is measured without one")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit(f"# mobilenet_v3_shapley_probe: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, fp32; kernel = "
         "TORCHPRUNER_PREFIX_GATED=1 (ops.scaled_project), composed = TORCHPRUNER_PREFIX_GATED=0, generic-hook = the "
         "same build with the engine off (the default)")
    project_stage(a, emit)
    end_to_end(a, emit)
    out.close()


if __name__ == "__main__":
    main()
