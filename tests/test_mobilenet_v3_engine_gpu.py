"""MobileNetV3 engine (engine/mobilenet_engine.py) on the pruned ``mobilenet_v3_small(10,
width_mult=0.5, small_input=True)`` of test_mobilenet_v3_engine.py (hidden widths that are no
multiples of 4; BN statistics that put inputs on both sides of every ReLU and, after the bias shift
``live_bn_v3`` describes, on all three branches of every post-depthwise Hardswish; random gate
biases), one batch of 8 at 32 px: logits against the module forward, APoZ against the generic path,
Taylor / signed Taylor / Sensitivity against the fp64 oracle that replays the engine's branch
decisions, the metric's reductions and criteria, repacking after a prune, and single blocks.

Measured on an MI355X (profiles/numerics/mobilenet_v3_engine_vs_oracle.txt): worst per-layer max abs
error / max |ref| 8.8e-7 for Taylor and signed Taylor, 1.4e-6 for Sensitivity (bound 1e-4), and 0
flipped branch decisions in 3.35 M against fp64."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


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
    from test_mobilenet_v3_engine import _convs, branch_census, live_bn_v3, pruned_v3
    from torchpruner_amd.engine import MobileNetV3Engine, maybe_mobilenet_engine
    model, x, y = live_bn_v3(pruned_v3())
    # the preconditions, on the CPU, before anything runs on the GPU
    census, plan = branch_census(model, x)
    names = dict(model.named_modules())
    skip = {id(plan.blocks[0].dw.act)}
    for name, fr in census.items():
        if id(names[name]) not in skip:
            assert sum(f > 0 for f in fr) >= 2, (name, fr)
    model = model.to(cuda)
    convs = _convs(model)
    assert len(convs) == 10 + 11
    why = []
    eng = maybe_mobilenet_engine(model, [], cuda, why=why)
    assert isinstance(eng, MobileNetV3Engine), why
    return {"model": model, "x": x.to(cuda), "y": y.to(cuda), "convs": convs, "eng": eng, "oracle": {}}


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
    from torchpruner_amd.engine.oracle import mobilenet_v3_scores_fp64
    if mode not in s["oracle"]:
        s["oracle"][mode] = mobilenet_v3_scores_fp64(s["eng"], s["model"], s["x"], s["y"], mode, conditioned=True)
    return s["oracle"][mode]


def _eval_modules(s, convs=None):
    from torchpruner_amd.utils import find_best_module_for_attributions
    return [find_best_module_for_attributions(s["model"], c) for c in (convs or s["convs"])]


def test_forward_logits_match_the_module(setup):
    s = setup
    with torch.no_grad():
        ref = s["model"](s["x"])
        torch.testing.assert_close(s["eng"].forward(s["x"]), ref, rtol=2e-3, atol=2e-3)
    assert set(map(id, _eval_modules(s))) == set(map(id, s["eng"].eval_modules()))
    assert any(s["eng"].real_width(m) % 4 for m in s["eng"].eval_modules())
    assert s["eng"].max_batch((3, 32, 32)) >= 8


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
    """Per-sample scores of all 10 post-expand and 11 post-depthwise activations, one batch of 8: max
    abs error / max |ref| per layer <= 1e-4 (the MobileNetV2 engine's bound) against the fp64 pass
    that replays the engine's own branch decisions, and those decisions flip against fp64 no more
    often than rounding ties allow."""
    from torchpruner_amd.engine.oracle import flip_violations
    s = setup
    m = _metric(mode, s, mobilenet_engine=True, reduction="none")
    got = m.run_many(s["convs"], find_best_evaluation_module=True)
    assert m.last_path["path"] == "mobilenet", m.last_path
    scores, flips, totals = _oracle(s, mode)
    # stem, 10 + 11 in the blocks, 9 gates x (ReLU, Hardsigmoid), head, classifier
    assert len(flips) == 1 + 21 + 18 + 2
    worst = 0.0
    for c, ev, a in zip(s["convs"], _eval_modules(s), got):
        ref = scores[ev].numpy()
        assert a.shape == ref.shape == (8, c.weight.shape[0])
        err = np.abs(a - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        print(f"{mode}: {tuple(ref.shape)} err {err:.3e}")
    print(f"{mode}: worst per-layer max abs error / max |ref| = {worst:.3e}; "
          f"decision flips {sum(flips.values())} of {sum(totals.values())}")
    assert worst <= 1e-4, worst
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
    if criterion is _mse_one_hot:  # another criterion against the oracle, first batch
        from torchpruner_amd.engine.oracle import mobilenet_v3_scores_fp64
        scores = mobilenet_v3_scores_fp64(s["eng"], s["model"], s["x"], s["y"], "taylor", True, _mse_one_hot)[0]
        one = _metric("taylor", s, criterion=criterion, mobilenet_engine=True, reduction="none").run_many(
            s["convs"], find_best_evaluation_module=True)
        for ev, p in zip(_eval_modules(s), one):
            ref = scores[ev].numpy()
            assert np.abs(p - ref).max() <= 1e-4 * np.abs(ref).max()


def test_single_blocks_gated_and_ungated(setup):
    """One gated and one ungated block scored alone: the backward stops at the earliest wanted
    block, and the scores are those of the all-blocks run's oracle."""
    s = setup
    plan = s["eng"].plan
    gated = next(i for i, b in enumerate(plan.blocks) if b.gate is not None and b.expand is not None and i > 3)
    ungated = next(i for i, b in enumerate(plan.blocks) if b.gate is None and b.expand is not None)
    scores = _oracle(s, "taylor_signed")[0]
    for bi in (gated, ungated):
        b = plan.blocks[bi]
        convs = [b.expand.conv, b.dw.conv]
        got = _metric("taylor_signed", s, mobilenet_engine=True, reduction="none").run_many(
            convs, find_best_evaluation_module=True)
        for ev, a in zip(_eval_modules(s, convs), got):
            ref = scores[ev].numpy()
            assert a.shape == ref.shape and np.abs(a - ref).max() <= 1e-4 * np.abs(ref).max()
        # post-depthwise alone: no depthwise dgrad is needed for it
        out = s["eng"].grad_scores(s["x"], s["y"], {b.dw.act}, "taylor_signed")
        assert set(out) == {b.dw.act}
        ref = scores[b.dw.act].numpy()
        a = out[b.dw.act][:, :ref.shape[1]].cpu().numpy()
        assert np.abs(a - ref).max() <= 1e-4 * np.abs(ref).max()


def test_engine_repacks_after_a_prune(setup, cuda):
    """After Pruner.prune_model on one graph entry (a gated block) the engine serves the new widths,
    and the scores of that block still match the conditioned oracle."""
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    from torchpruner_amd.engine import maybe_mobilenet_engine
    from torchpruner_amd.engine.oracle import flip_violations, mobilenet_v3_scores_fp64
    from torchpruner_amd.utils import find_best_module_for_attributions
    s = dict(setup, model=copy.deepcopy(setup["model"]))
    model = s["model"]
    module, cascade = get_mobilenet_pruning_graph(model)[3]
    n = module.weight.shape[0]
    Pruner(model, (3, 32, 32), cuda).prune_model(module, np.arange(0, n, 3), cascade)
    assert module.weight.shape[0] == n - len(range(0, n, 3))
    dw = next(c for c in cascade if isinstance(c, torch.nn.Conv2d) and c.groups != 1)
    convs = [module, dw]
    ev = [find_best_module_for_attributions(model, c) for c in convs]
    eng = maybe_mobilenet_engine(model, ev, cuda, grad=True)
    assert eng is not None and eng.real_width(ev[0]) == module.weight.shape[0]
    s["convs"] = convs
    for mode in ("taylor_signed", "sensitivity"):
        got = _metric(mode, s, mobilenet_engine=True, reduction="none").run_many(convs, find_best_evaluation_module=True)
        scores, flips, totals = mobilenet_v3_scores_fp64(eng, model, s["x"], s["y"], mode, conditioned=True)
        assert not flip_violations(flips, totals)
        for e, a in zip(ev, got):
            ref = scores[e].numpy()
            assert a.shape == ref.shape == (8, module.weight.shape[0])
            assert np.abs(a - ref).max() <= 1e-4 * np.abs(ref).max()


def test_fused_stem_layout(cuda):
    """The 224-px layout (stride-2 stem, first block without expand conv and shortcut): the first
    depthwise conv applies the stem's Hardswish itself (codes (3, 1)). Unpruned
    ``mobilenet_v3_small(10, width_mult=0.5)`` at 64 px, batch 4: logits, and signed Taylor of every
    layer against the conditioned oracle."""
    from test_mobilenet_v3_engine import _convs, live_bn_v3
    from torchpruner_amd.engine import maybe_mobilenet_engine
    from torchpruner_amd.engine.oracle import flip_violations, mobilenet_v3_scores_fp64
    from torchpruner_amd.models import mobilenet_v3_small
    torch.manual_seed(0)
    model, _, _ = live_bn_v3(mobilenet_v3_small(10, width_mult=0.5))
    model = model.to(cuda)
    g = torch.Generator().manual_seed(6)
    x, y = torch.randn(4, 3, 64, 64, generator=g).to(cuda), torch.randint(0, 10, (4,), generator=g).to(cuda)
    eng = maybe_mobilenet_engine(model, [], cuda)
    assert eng is not None and eng._stem_fused()
    with torch.no_grad():
        torch.testing.assert_close(eng.forward(x), model(x), rtol=2e-3, atol=2e-3)
    s = {"model": model, "x": x, "y": y, "convs": _convs(model)}
    m = _metric("taylor_signed", s, mobilenet_engine=True, reduction="none")
    got = m.run_many(s["convs"], find_best_evaluation_module=True)
    assert m.last_path["path"] == "mobilenet", m.last_path
    scores, flips, totals = mobilenet_v3_scores_fp64(eng, model, x, y, "taylor_signed", conditioned=True)
    assert not flip_violations(flips, totals)
    for ev, a in zip(_eval_modules(s), got):
        ref = scores[ev].numpy()
        assert a.shape == ref.shape and np.abs(a - ref).max() <= 1e-4 * np.abs(ref).max()
