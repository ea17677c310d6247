"""EfficientNet engine (engine/mobilenet_engine.py) on ``efficientnet(0.25, 0.34, 10, small_input=True)``
with 30 % + 1 of every hidden width pruned (widths that are no multiples of 4), random BN statistics and
gate biases, one batch of 8 at 32 px: logits against the module forward, APoZ against the generic
path, Taylor / signed Taylor / Sensitivity against the generic path on a float64 CPU copy (SiLU is
smooth: no branch decisions to replay), the Shapley rejection, and repacking after a prune.

The measured worst per-layer errors are in profiles/numerics/efficientnet_engine.txt (bound 1e-4)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_SETUP = {}


def _build():
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    from torchpruner_amd.models import efficientnet
    torch.manual_seed(0)
    model = efficientnet(0.25, 0.34, 10, small_input=True)
    rng = np.random.RandomState(0)
    pruner = Pruner(model, (3, 32, 32), "cpu")
    for module, cascade in get_mobilenet_pruning_graph(model):
        n = module.weight.shape[0]
        pruner.prune_model(module, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    gen = torch.Generator().manual_seed(3)
    model.eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_(torch.rand(n, generator=gen) + 0.75)
                m.bias.copy_(torch.rand(n, generator=gen) * 2 - 1)
                m.running_mean.copy_(torch.randn(n, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(n, generator=gen) + 0.5)
            elif isinstance(m, nn.Conv2d) and m.bias is not None:  # the gates' fcs
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.5)
    return model, torch.randn(8, 3, 32, 32, generator=gen), torch.randint(0, 10, (8,), generator=gen)


@pytest.fixture
def setup(cuda):
    if not _SETUP:
        from torchpruner_amd import get_mobilenet_pruning_graph
        model, x, y = _build()
        ref = copy.deepcopy(model).double()
        expand = [m for m, _ in get_mobilenet_pruning_graph(model)]
        dw = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups != 1]
        names = {id(m): n for n, m in model.named_modules()}
        convs = expand + [c for c in dw if not any(c is e for e in expand)]
        refs = dict(ref.named_modules())
        _SETUP.update(model=model.to(cuda), x=x.to(cuda), y=y.to(cuda), convs=convs, ref=ref, x64=x.double(), y64=y,
                      ref_convs=[refs[names[id(c)]] for c in convs])
    return _SETUP


def _metric(which, model, x, y, **kw):
    from torchpruner_amd import APoZAttributionMetric, SensitivityAttributionMetric, TaylorAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    cls = {"apoz": APoZAttributionMetric, "sensitivity": SensitivityAttributionMetric}.get(which, TaylorAttributionMetric)
    if which == "taylor_signed":
        kw["signed"] = True
    return cls(model, DeviceLoader(x, y, 8), F.cross_entropy, x.device, **kw)


def test_logits_apoz_and_shapley_rejection(setup, cuda):
    from torchpruner_amd import ShapleyAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    from torchpruner_amd.engine import EfficientNetEngine, maybe_mobilenet_engine
    s = setup
    why = []
    eng = maybe_mobilenet_engine(s["model"], [], cuda, why=why)
    assert isinstance(eng, EfficientNetEngine), why
    assert any(eng.real_width(m) % 4 for m in eng.eval_modules()) and not eng._stem_fused()
    with torch.no_grad():
        torch.testing.assert_close(eng.forward(s["x"]), s["model"](s["x"]), rtol=2e-3, atol=2e-3)
    on = _metric("apoz", s["model"], s["x"], s["y"], mobilenet_engine=True)
    got = on.run_many(s["convs"], find_best_evaluation_module=True)
    assert on.last_path["path"] == "mobilenet", on.last_path
    off = _metric("apoz", s["model"], s["x"], s["y"])
    ref = off.run_many(s["convs"], find_best_evaluation_module=True)
    assert off.last_path["path"] == "generic", off.last_path
    for c, a, b in zip(s["convs"], got, ref):
        assert a.shape == b.shape == (c.weight.shape[0],)
        np.testing.assert_allclose(a, b, atol=0.5)
    why = []
    assert maybe_mobilenet_engine(s["model"], [], cuda, why=why, shapley=True) is None and "Shapley" in why[0]
    sv = ShapleyAttributionMetric(s["model"], DeviceLoader(s["x"], s["y"], 8), F.cross_entropy, cuda, sv_samples=1,
                                  mobilenet_engine=True)
    sv.run(min(s["convs"], key=lambda c: c.weight.shape[0]), find_best_evaluation_module=True)
    assert sv.last_path["path"].startswith("generic") and any("Shapley" in r for r in sv.last_path["reasons"])


@pytest.mark.parametrize("mode", ["taylor", "taylor_signed", "sensitivity"])
def test_gradient_scores_match_the_fp64_generic_path(setup, mode):
    s = setup
    m = _metric(mode, s["model"], s["x"], s["y"], mobilenet_engine=True, reduction="none")
    got = m.run_many(s["convs"], find_best_evaluation_module=True)
    assert m.last_path["path"] == "mobilenet", m.last_path
    if mode not in s:
        s[mode] = _metric(mode, s["ref"], s["x64"], s["y64"], reduction="none").run_many(
            s["ref_convs"], find_best_evaluation_module=True)
    worst = 0.0
    for c, a, ref in zip(s["convs"], got, s[mode]):
        assert a.shape == ref.shape == (8, c.weight.shape[0])
        worst = max(worst, float(np.abs(a - ref).max() / np.abs(ref).max()))
    print(f"efficientnet engine {mode}: worst per-layer max abs error / max |ref| = {worst:.3e} (bound 1e-4)")
    assert worst <= 1e-4, worst


def test_engine_repacks_after_a_prune(setup, cuda):
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    from torchpruner_amd.engine import maybe_mobilenet_engine
    from torchpruner_amd.utils import find_best_module_for_attributions
    model = copy.deepcopy(setup["model"])
    module, cascade = get_mobilenet_pruning_graph(model)[2]
    n = module.weight.shape[0]
    names = {id(m): k for k, m in model.named_modules()}
    Pruner(model, (3, 32, 32), cuda).prune_model(module, np.arange(0, n, 3), cascade)
    dw = next(c for c in cascade if isinstance(c, nn.Conv2d) and c.groups != 1)
    convs = [module, dw]
    ev = [find_best_module_for_attributions(model, c) for c in convs]
    eng = maybe_mobilenet_engine(model, ev, cuda, grad=True)
    assert eng is not None and eng.real_width(ev[0]) == module.weight.shape[0] == n - len(range(0, n, 3))
    got = _metric("taylor_signed", model, setup["x"], setup["y"], mobilenet_engine=True, reduction="none").run_many(
        convs, find_best_evaluation_module=True)
    ref_model = copy.deepcopy(model).cpu().double()
    refs = dict(ref_model.named_modules())
    ref = _metric("taylor_signed", ref_model, setup["x64"], setup["y64"], reduction="none").run_many(
        [refs[names[id(c)]] for c in convs], find_best_evaluation_module=True)
    for a, b in zip(got, ref):
        assert a.shape == b.shape == (8, module.weight.shape[0])
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max()
