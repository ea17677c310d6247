"""MobileNet engine (engine/mobilenet_engine.py) on a pruned MobileNetV2 (hidden widths that are no
multiples of 4) whose BN statistics make both ReLU6 kinks live: logits against the module forward,
APoZ against the generic path, Taylor / signed Taylor / Sensitivity against the fp64 oracle that
replays the engine's ReLU6 decisions, the metric's reductions and criteria, the opt-in default, and
repacking after a prune.

Measured on an MI355X (profiles/numerics/mobilenet_engine_vs_oracle.txt): worst per-layer max abs
error / max |ref| 6.4e-7 for Taylor and signed Taylor, 4.7e-7 for Sensitivity (bound 1e-4), and 0
flipped ReLU6 decisions in 11.9 M against fp64."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _live_bn_model(pruned):
    """(eval-mode copy of ``pruned`` with non-trivial BN statistics, x (8, 3, 32, 32), y) from
    torch.Generator().manual_seed(3): per BN, in module order, weight ~ U(0.75, 1.75), bias ~ U(0, 2),
    running_mean ~ N(0, 0.2), running_var ~ U(0.5, 1.5); then x, then y. From the second block on the
    post-expand ReLU6 inputs then hold a quarter to a half <= 0 and 1.5-21 % >= 6, the post-depthwise
    ones 4-14 % <= 0 and nothing >= 6 (test_mobilenet_engine.py checks both)."""
    gen = torch.Generator().manual_seed(3)
    model = copy.deepcopy(pruned).eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_(torch.rand(n, generator=gen) + 0.75)
                m.bias.copy_(torch.rand(n, generator=gen) * 2)
                m.running_mean.copy_(torch.randn(n, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(n, generator=gen) + 0.5)
    x = torch.randn(8, 3, 32, 32, generator=gen)
    y = torch.randint(0, 10, (8,), generator=gen)
    return model, x, y


def _mse_one_hot(out, y, reduction="mean"):
    return F.mse_loss(out, F.one_hot(y, out.shape[1]).to(out.dtype), reduction=reduction)


_SETUP = {}


@pytest.fixture
def setup(cuda):
    """Model, data, engine and the oracle's results, built once for the module."""
    if not _SETUP:
        _SETUP.update(_build_setup(cuda))
    return _SETUP


def _build_setup(cuda):
    from test_mobilenet_gpu import _pruned_mobilenet
    from torchpruner_amd import get_mobilenet_pruning_graph
    from torchpruner_amd.engine import maybe_mobilenet_engine
    model, x, y = _live_bn_model(_pruned_mobilenet())
    model = model.to(cuda)
    graph = get_mobilenet_pruning_graph(model)
    expand = [m for m, _ in graph]
    dw = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d) and m.groups != 1]
    assert len(expand) == 16 and len(dw) == 17
    eng = maybe_mobilenet_engine(model, [], cuda)
    assert eng is not None
    return {"model": model, "x": x.to(cuda), "y": y.to(cuda), "convs": expand + dw, "eng": eng, "oracle": {}}


def _metric(which, s, **kw):
    from torchpruner_amd import APoZAttributionMetric, SensitivityAttributionMetric, TaylorAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    x, y = kw.pop("x", s["x"]), kw.pop("y", s["y"])
    crit = kw.pop("criterion", F.cross_entropy)
    cls = {"apoz": APoZAttributionMetric, "sensitivity": SensitivityAttributionMetric}.get(which, TaylorAttributionMetric)
    if which == "taylor_signed":
        kw["signed"] = True
    return cls(s["model"], DeviceLoader(x, y, 8), crit, x.device, **kw)


def _oracle(s, mode):
    """fp64 scores with the engine's ReLU6 decisions replayed, computed once per mode."""
    from torchpruner_amd.engine.oracle import mobilenet_scores_fp64
    if mode not in s["oracle"]:
        s["oracle"][mode] = mobilenet_scores_fp64(s["eng"], s["model"], s["x"], s["y"], mode, conditioned=True)
    return s["oracle"][mode]


def _eval_modules(s):
    from torchpruner_amd.utils import find_best_module_for_attributions
    return [find_best_module_for_attributions(s["model"], c) for c in s["convs"]]


def test_forward_logits_match_the_module(setup):
    s = setup
    with torch.no_grad():
        ref = s["model"](s["x"])
        torch.testing.assert_close(s["eng"].forward(s["x"]), ref, rtol=2e-3, atol=2e-3)
    assert set(map(id, _eval_modules(s))) == set(map(id, s["eng"].eval_modules()))
    assert any(s["eng"].real_width(m) % 4 for m in s["eng"].eval_modules())


def test_apoz_matches_the_generic_path(setup):
    s = setup
    on = _metric("apoz", s, mobilenet_engine=True)
    got = on.run_many(s["convs"], find_best_evaluation_module=True)
    assert on.last_path["path"] == "mobilenet", on.last_path
    off = _metric("apoz", s)
    ref = off.run_many(s["convs"], find_best_evaluation_module=True)
    assert off.last_path["path"] == "generic", off.last_path
    for c, a, b in zip(s["convs"], got, ref):
        assert a.shape == b.shape == (c.weight.shape[0],)
        np.testing.assert_allclose(a, b, atol=0.5)  # mean counts: only values within rounding of 0 may flip
    assert max(float(b.max()) for b in ref) > 10


@pytest.mark.parametrize("mode", ["taylor", "taylor_signed", "sensitivity"])
def test_gradient_scores_match_the_conditioned_oracle(setup, mode):
    """Per-sample scores of all 16 post-expand and 17 post-depthwise ReLU6s, one batch of 8: max abs
    error / max |ref| per layer <= 1e-4 (the bound of the generic MobileNet test) against the fp64
    pass that replays the engine's own ReLU6 decisions, and those decisions flip against fp64 no
    more often than rounding ties allow."""
    from torchpruner_amd.engine.oracle import flip_violations
    s = setup
    m = _metric(mode, s, mobilenet_engine=True, reduction="none")
    got = m.run_many(s["convs"], find_best_evaluation_module=True)
    assert m.last_path["path"] == "mobilenet", m.last_path
    scores, flips, totals = _oracle(s, mode)
    assert len(flips) == 35  # every ReLU6 of the net: stem, 16 + 17 in the blocks, head
    worst = 0.0
    for c, ev, a in zip(s["convs"], _eval_modules(s), got):
        ref = scores[ev].numpy()
        assert a.shape == ref.shape == (8, c.weight.shape[0])
        err = np.abs(a - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= 1e-4, (c, err)
    print(f"{mode}: worst per-layer max abs error / max |ref| = {worst:.3e}; "
          f"decision flips {sum(flips.values())} of {sum(totals.values())}")
    assert not flip_violations(flips, totals), flip_violations(flips, totals)


@pytest.mark.parametrize("criterion", [F.cross_entropy, _mse_one_hot], ids=["cross_entropy", "mse"])
def test_mean_reduction_any_criterion_and_determinism(setup, cuda, criterion):
    s = setup
    g = torch.Generator().manual_seed(4)
    x = torch.cat([s["x"], torch.randn(8, 3, 32, 32, generator=g).to(cuda)])
    y = torch.cat([s["y"], torch.randint(0, 10, (8,), generator=g).to(cuda)])
    kw = dict(x=x, y=y, criterion=criterion, mobilenet_engine=True)
    per = _metric("taylor", s, reduction="none", **kw).run_many(s["convs"], find_best_evaluation_module=True)
    m = _metric("taylor", s, **kw)
    mean = m.run_many(s["convs"], find_best_evaluation_module=True)
    assert m.last_path["path"] == "mobilenet", m.last_path
    for a, p in zip(mean, per):
        assert p.shape[0] == 16
        np.testing.assert_allclose(a, p.astype(np.float64).mean(0), rtol=1e-5, atol=1e-5 * np.abs(p).mean(0).max())
    again = _metric("taylor", s, **kw).run_many(s["convs"], find_best_evaluation_module=True)
    for a, b in zip(mean, again):
        np.testing.assert_array_equal(a, b)
    if criterion is F.cross_entropy:  # (c) on the first batch is what the two-batch run saw there
        scores = _oracle(s, "taylor")[0]
        for ev, p in zip(_eval_modules(s), per):
            ref = scores[ev].numpy()
            assert np.abs(p[:8] - ref).max() <= 1e-4 * np.abs(ref).max()


def test_engine_is_opt_in(setup, monkeypatch):
    s = setup
    monkeypatch.delenv("TORCHPRUNER_MOBILENET_ENGINE", raising=False)
    m = _metric("taylor", s)
    m.run_many(s["convs"][:2], find_best_evaluation_module=True)
    assert m.last_path["path"] == "generic", m.last_path
    monkeypatch.setenv("TORCHPRUNER_MOBILENET_ENGINE", "1")
    m = _metric("taylor", s)
    m.run_many(s["convs"][:2], find_best_evaluation_module=True)
    assert m.last_path["path"] == "mobilenet", m.last_path
    m = _metric("taylor", s, mobilenet_engine=False)
    m.run_many(s["convs"][:2], find_best_evaluation_module=True)
    assert m.last_path["path"] == "generic", m.last_path


def test_engine_repacks_after_a_prune(setup, cuda):
    """After Pruner.prune_model on one graph entry the engine serves the new widths, and the scores
    of that block still match the conditioned oracle."""
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    from torchpruner_amd.engine import maybe_mobilenet_engine
    from torchpruner_amd.engine.oracle import flip_violations, mobilenet_scores_fp64
    from torchpruner_amd.utils import find_best_module_for_attributions
    s = dict(setup, model=copy.deepcopy(setup["model"]))
    model = s["model"]
    module, cascade = get_mobilenet_pruning_graph(model)[5]
    n = module.weight.shape[0]
    Pruner(model, (3, 32, 32), cuda).prune_model(module, np.arange(0, n, 3), cascade)
    assert module.weight.shape[0] == n - len(range(0, n, 3))
    dw = cascade[1]
    convs = [module, dw]
    ev = [find_best_module_for_attributions(model, c) for c in convs]
    eng = maybe_mobilenet_engine(model, ev, cuda, grad=True)
    assert eng is not None and eng.real_width(ev[0]) == module.weight.shape[0]
    s["convs"] = convs
    for mode in ("taylor_signed", "sensitivity"):
        got = _metric(mode, s, mobilenet_engine=True, reduction="none").run_many(convs, find_best_evaluation_module=True)
        scores, flips, totals = mobilenet_scores_fp64(eng, model, s["x"], s["y"], mode, conditioned=True)
        assert not flip_violations(flips, totals)
        for e, a in zip(ev, got):
            ref = scores[e].numpy()
            assert a.shape == ref.shape == (8, module.weight.shape[0])
            assert np.abs(a - ref).max() <= 1e-4 * np.abs(ref).max()
