"""Shapley values on the MobileNetV3 engine: the stacked prefix logits of every evaluation module against
the float64 module forward with a masking hook (scaled project GEMM and composed path), and the metric
end to end against the float64 hook path. The model is the pruned live-BN MobileNetV3-small of
test_mobilenet_v3_engine.py (9 gated and 2 gate-free blocks), its first 6 images.
Measured figures: profiles/numerics/mobilenet_v3_shapley_engine.txt."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_SETUP = {}


@pytest.fixture
def setup(cuda):
    if not _SETUP:
        from test_mobilenet_v3_engine import live_bn_v3, pruned_v3
        from torchpruner_amd.engine import MobileNetV3Engine, maybe_mobilenet_engine
        model, x, y = live_bn_v3(pruned_v3())
        m64 = copy.deepcopy(model).double()
        model = model.to(cuda)
        why = []
        eng = maybe_mobilenet_engine(model, [], cuda, why=why, shapley=True)
        assert isinstance(eng, MobileNetV3Engine), why
        _SETUP.update(model=model, m64=m64, x=x[:6].to(cuda), y=y[:6].to(cuda), eng=eng, ref={})
    return _SETUP


def _hooked_logits(s, idx, rank, p0, cnt):
    """float64 CPU logits (cnt * B, classes) of the module forward with evaluation module ``idx``'s
    output channels of rank < p0 + j zeroed in copy j."""
    from torchpruner_amd.engine.mobilenet_engine import MobileNetV3Engine, build_mobilenet_v3_plan
    m64 = s["m64"]
    mod = MobileNetV3Engine(m64, build_mobilenet_v3_plan(m64)[0]).eval_modules()[idx]
    x = s["x"].double().cpu()
    outs = []
    for j in range(cnt):
        keep = (rank >= p0 + j).view(1, -1, 1, 1)
        h = mod.register_forward_hook(lambda _m, _i, o, keep=keep: torch.where(keep, o, torch.zeros((), dtype=o.dtype)))
        try:
            with torch.no_grad():
                outs.append(m64(x))
        finally:
            h.remove()
    return torch.cat(outs, 0)


@pytest.mark.parametrize("gated", ["1", "0"], ids=["scaled_project", "composed"])
def test_prefix_logits_match_the_hooked_module(setup, monkeypatch, gated):
    """Every evaluation module, one chunk of 5 prefixes from the middle of a seeded permutation:
    rtol = atol = 2e-3 (the bound of the MobileNetV2 test) against the float64 module forward with a
    masking hook, on the scaled project GEMM and with TORCHPRUNER_PREFIX_GATED=0."""
    s = setup
    eng = s["eng"]
    monkeypatch.setenv("TORCHPRUNER_PREFIX_GATED", gated)
    mods = eng.eval_modules()
    kinds = [eng.locate(m) for m in mods]
    blocks = eng.plan.blocks
    assert {k for bi, k in kinds if blocks[bi].gate is not None} == {"dw", "expand"}
    assert any(blocks[bi].gate is None for bi, _ in kinds)
    assert any(k == "expand" and type(blocks[bi].dw.act) is nn.Hardswish and blocks[bi].gate is not None
               and bool(eng.prefix_fill(bi, k).any()) for bi, k in kinds)
    assert any(blocks[bi].shortcut for bi, _ in kinds) and any(blocks[bi].dw.conv.stride[0] == 2 for bi, _ in kinds)
    cnt, worst = 5, 0.0
    for idx, (m, (bi, kind)) in enumerate(zip(mods, kinds)):
        n = eng.real_width(m)
        perm = torch.from_numpy(np.random.RandomState(idx).permutation(n))
        rank = torch.empty(n, dtype=torch.long)
        rank[perm] = torch.arange(n)
        p0 = n // 2 - 2
        if idx not in s["ref"]:
            s["ref"][idx] = _hooked_logits(s, idx, rank, p0, cnt)
        ref = s["ref"][idx]
        with torch.no_grad():
            h, y = eng.forward_to(s["x"], bi)
            rank_p = torch.cat([rank, torch.full((y.shape[3] - n,), n + 1)]).to(torch.int32).to(y.device)
            got = eng.prefix_logits(bi, kind, h, y, perm.to(torch.int32).to(y.device), rank_p, p0, cnt)
        assert got.shape == ref.shape == (cnt * 6, 10)
        worst = max(worst, float((got.double().cpu() - ref).abs().max()))
        torch.testing.assert_close(got.double().cpu(), ref, rtol=2e-3, atol=2e-3, msg=lambda t: f"{idx} {kind}: {t}")
        assert not torch.equal(ref[:6], ref[-6:])
    print(f"V3 prefix logits (TORCHPRUNER_PREFIX_GATED={gated}): worst abs error {worst:.3e}")


def _shapley(model, module, x, y, device, backend, **kw):
    from torchpruner_amd import ShapleyAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    os.environ["TORCHPRUNER_BACKEND"] = backend
    try:
        np.random.seed(7)
        metric = ShapleyAttributionMetric(model, DeviceLoader(x, y, 6), F.cross_entropy, device, sv_samples=1,
                                          reduction="none", **kw)
        return metric.run(module, find_best_evaluation_module=True), metric
    finally:
        del os.environ["TORCHPRUNER_BACKEND"]


def _targets(model):
    """(name, conv whose evaluation module is scored): the last gated block's depthwise conv and the
    second-to-last gated block's expand conv (the float32 hook path of either stays within 1e-4 of
    the float64 one, far inside the bound)."""
    from torchpruner_amd.engine.mobilenet_engine import build_mobilenet_v3_plan
    gated = [b for b in build_mobilenet_v3_plan(model)[0].blocks if b.gate is not None and b.expand is not None]
    return [("last gated depthwise", gated[-1].dw.conv), ("gated expand", gated[-2].expand.conv)]


@pytest.mark.parametrize("ti", [0, 1], ids=["depthwise", "expand"])
def test_shapley_matches_the_fp64_hook_path(setup, cuda, ti):
    """sv_samples=1, reduction="none", np.random.seed(7): max abs error / max |ref| < 2e-2 (the bound of
    the MobileNetV2 and ResNet Shapley tests) against the float64 CPU hook path, served by the engine."""
    s = setup
    name, module = _targets(s["model"])[ti]
    got, metric = _shapley(s["model"], module, s["x"], s["y"], cuda, "hip", mobilenet_engine=True)
    assert metric.last_path["path"] == "mobilenet", metric.last_path
    ref, _ = _shapley(s["m64"], _targets(s["m64"])[ti][1], s["x"].double().cpu(), s["y"].cpu(), "cpu", "torch")
    assert got.shape == ref.shape == (6, module.weight.shape[0])
    err = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))
    print(f"V3 shapley {name}: max abs error / max |ref| = {err:.3e} (max |ref| {np.abs(ref).max():.3e})")
    assert err < 2e-2, (name, err)
