"""CPU side of the MobileNetV3 attribution engine (engine/mobilenet_engine.py): the structural plan,
its rejections, the fp64 oracle without an engine against the generic metric, the path a metric
reports on the CPU, Shapley's reason, and the preconditions of tests/test_mobilenet_v3_engine_gpu.py
(every piecewise activation of its model has inputs on more than one branch)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from torchpruner_amd.engine import build_mobilenet_plan, build_mobilenet_v3_plan
from torchpruner_amd.models import mobilenet_v2, mobilenet_v3_large, mobilenet_v3_small


def pruned_v3():
    """``mobilenet_v3_small(10, width_mult=0.5, small_input=True)`` cut as ``_v3_pruned`` of
    test_mobilenet_v3_hswish_gpu.py cuts it (30 % + 1 of every hidden width, random gate biases)."""
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    torch.manual_seed(0)
    model = mobilenet_v3_small(10, width_mult=0.5, small_input=True)
    rng = np.random.RandomState(0)
    pruner = Pruner(model, (3, 32, 32), "cpu")
    for module, cascade in get_mobilenet_pruning_graph(model):
        n = module.weight.shape[0]
        pruner.prune_model(module, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    gen = torch.Generator().manual_seed(5)
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        elif isinstance(m, nn.Conv2d) and m.bias is not None:  # the gates' fcs: no symmetric start
            with torch.no_grad():
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.5)
    return model


def live_bn_v3(pruned):
    """(eval-mode copy of ``pruned``, x (8, 3, 32, 32), y) with the BN recipe of ``_live_bn_model`` in
    test_mobilenet_engine_gpu.py, from torch.Generator().manual_seed(3): per BN, in module order,
    weight ~ U(0.75, 1.75), bias ~ U(0, 2), running_mean ~ N(0, 0.2), running_var ~ U(0.5, 1.5); then
    x, then y.

    That recipe leaves the inputs of the post-depthwise Hardswishes on the middle branch alone (a
    depthwise conv's output is small: 94-100 % of them in [-3, 3]). So the BN bias of every depthwise
    unit that ends in a Hardswish is shifted afterwards: + 2.5 on its even channels, - 4.5 on its odd
    ones (centres near 3.5 and - 3.5), which puts inputs on all three branches of each
    (test_gpu_test_preconditions prints the census)."""
    gen = torch.Generator().manual_seed(3)
    model = copy.deepcopy(pruned).eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_(torch.rand(n, generator=gen) + 0.75)
                m.bias.copy_(torch.rand(n, generator=gen) * 2)
                m.running_mean.copy_(torch.randn(n, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(n, generator=gen) + 0.5)
        for m in model.modules():
            if isinstance(m, nn.Sequential) and len(m) == 3 and isinstance(m[0], nn.Conv2d) and m[0].groups != 1 \
                    and isinstance(m[2], nn.Hardswish):
                m[1].bias[0::2] += 2.5
                m[1].bias[1::2] -= 4.5
    x = torch.randn(8, 3, 32, 32, generator=gen)
    y = torch.randint(0, 10, (8,), generator=gen)
    return model, x, y


def branch_census(model, x):
    """{module name: fractions of its inputs per branch} for the block activations of the plan:
    ReLU (<= 0, > 0), Hardswish (< -3, middle, > 3)."""
    plan, why = build_mobilenet_v3_plan(model)
    assert plan is not None, why
    names = {id(m): n for n, m in model.named_modules()}
    acts = [a for b in plan.blocks for a in (([b.expand.act] if b.expand is not None else []) + [b.dw.act])]
    out = {}

    def hook(mod, inp):
        z = inp[0].detach()
        if type(mod) is nn.ReLU:
            out[names[id(mod)]] = ((z <= 0).float().mean().item(), (z > 0).float().mean().item())
        else:
            out[names[id(mod)]] = ((z < -3).float().mean().item(), ((z >= -3) & (z <= 3)).float().mean().item(),
                                   (z > 3).float().mean().item())
    handles = [a.register_forward_pre_hook(hook) for a in acts]
    with torch.no_grad():
        model(x)
    for h in handles:
        h.remove()
    return out, plan


@pytest.fixture(scope="module")
def pruned():
    return pruned_v3()


def _codes(plan):
    code = {nn.ReLU: 1, nn.Hardswish: 3}
    return [(code[type(b.expand.act)] if b.expand is not None else None, code[type(b.dw.act)]) for b in plan.blocks]


@pytest.mark.parametrize("make,table", [(mobilenet_v3_small, "SMALL"), (mobilenet_v3_large, "LARGE")])
def test_plan_lowers_the_v3_nets(make, table):
    from torchpruner_amd.models import mobilenet_v3
    rows = getattr(mobilenet_v3, table)
    model = make(10, small_input=True)
    plan, why = build_mobilenet_v3_plan(model)
    assert plan is not None, why
    assert len(plan.blocks) == len(rows)
    blocks = list(model.features)[1:-1]
    assert [b.shortcut for b in plan.blocks] == [b.use_res_connect for b in blocks]
    assert [b.gate is not None for b in plan.blocks] == [bool(r[3]) for r in rows]
    want = [(None if len(b.block) == (3 if r[3] else 2) else (3 if r[4] else 1), 3 if r[4] else 1)
            for b, r in zip(blocks, rows)]
    assert _codes(plan) == want
    assert plan.blocks[0].expand is None and plan.blocks[0].shortcut  # small_input: stride 1, equal widths
    assert type(plan.stem.act) is nn.Hardswish and type(plan.head.act) is nn.Hardswish
    assert plan.fc1 is model.classifier[0] and plan.fc is model.classifier[-1]
    # the V2 planner keeps rejecting these nets
    assert build_mobilenet_plan(model)[0] is None
    # stride-2 stem and first block (224-px layout): no shortcut on the first block, the stem is fused
    plan2, why = build_mobilenet_v3_plan(make(10))
    assert plan2 is not None, why
    if table == "SMALL":
        assert not plan2.blocks[0].shortcut and plan2.blocks[0].expand is None


def test_plan_lowers_a_pruned_net(pruned):
    plan, why = build_mobilenet_v3_plan(pruned)
    assert plan is not None, why
    widths = [b.dw.conv.weight.shape[0] for b in plan.blocks]
    assert any(w % 4 for w in widths), widths
    for b in plan.blocks:
        if b.gate is not None:
            assert b.gate.fc1.weight.shape[1] == b.dw.conv.weight.shape[0] == b.gate.fc2.weight.shape[0]
    assert sum(b.gate is not None for b in plan.blocks) == 9


def test_plan_rejects_with_a_reason_naming_the_module():
    plan, why = build_mobilenet_v3_plan(mobilenet_v2(10))
    assert plan is None and "MobileNetV3" in why
    m = mobilenet_v3_small(10, small_input=True)
    m.features[4].block[0][2] = nn.SiLU()
    plan, why = build_mobilenet_v3_plan(m)
    assert plan is None and "features.4.block.0" in why and "SiLU" in why
    m = mobilenet_v3_small(10, small_input=True)
    m.features[4].block[2].activation = nn.SiLU()
    plan, why = build_mobilenet_v3_plan(m)
    assert plan is None and "features.4.block.2" in why and "SiLU" in why
    m = mobilenet_v3_small(10, small_input=True)
    dw = m.features[2].block[1][0]
    dw.dilation, dw.padding = (2, 2), (2, 2)
    plan, why = build_mobilenet_v3_plan(m)
    assert plan is None and "features.2.block.1" in why and "dilation" in why
    m = mobilenet_v3_small(10, small_input=True)
    m.classifier = nn.Sequential(nn.Dropout(0.2), nn.Linear(m.classifier[0].in_features, 10))
    plan, why = build_mobilenet_v3_plan(m)
    assert plan is None and "classifier" in why
    m = mobilenet_v3_small(10, small_input=True)
    m.classifier[1] = nn.ReLU()
    plan, why = build_mobilenet_v3_plan(m)
    assert plan is None and "classifier" in why


def _convs(model):
    from torchpruner_amd import get_mobilenet_pruning_graph
    expand = [m for m, _ in get_mobilenet_pruning_graph(model)]
    dw = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups != 1]
    return expand + [c for c in dw if not any(c is e for e in expand)]


def test_gpu_test_preconditions(pruned):
    """The model of test_mobilenet_v3_engine_gpu.py: from the second block on every ReLU has inputs on
    both sides of 0 and every block Hardswish inputs on more than one branch."""
    model, x, _ = live_bn_v3(pruned)
    census, plan = branch_census(model, x)
    for name, fr in census.items():
        print(name, ["%.3f" % f for f in fr])
    first = {id(a) for a in ([plan.blocks[0].dw.act] + ([plan.blocks[0].expand.act] if plan.blocks[0].expand else []))}
    names = {n: m for n, m in model.named_modules()}
    for name, fr in census.items():
        if id(names[name]) in first:
            continue
        assert sum(f > 0 for f in fr) >= 2, (name, fr)


@pytest.mark.parametrize("mode", ["taylor", "taylor_signed", "sensitivity"])
def test_unconditioned_oracle_equals_the_generic_metric(pruned, mode):
    from torchpruner_amd import SensitivityAttributionMetric, TaylorAttributionMetric
    from torchpruner_amd.engine.oracle import mobilenet_v3_scores_fp64
    from torchpruner_amd.utils import find_best_module_for_attributions
    model, x, y = live_bn_v3(pruned)
    model = model.double()
    x = x.double()
    scores, flips, totals = mobilenet_v3_scores_fp64(None, model, x, y, mode, conditioned=False)
    assert not flips and not totals
    convs = _convs(model)
    plan = build_mobilenet_v3_plan(model)[0]
    assert len(scores) == len(convs) == sum(1 + (b.expand is not None) for b in plan.blocks)
    cls = SensitivityAttributionMetric if mode == "sensitivity" else TaylorAttributionMetric
    kw = {"signed": True} if mode == "taylor_signed" else {}
    metric = cls(model, [(x, y)], F.cross_entropy, "cpu", reduction="none", **kw)
    got = metric.run_many(convs, find_best_evaluation_module=True)
    for c, a in zip(convs, got):
        ref = scores[find_best_module_for_attributions(model, c)].numpy()
        assert a.shape == ref.shape == (8, c.weight.shape[0])
        # the generic path hands the criterion float32 logits, so dL/dlogits carries float32 rounding even
        # in a float64 model; the scores are linear in it: 1e-6 of the layer's largest score, the bound
        # of the MobileNetV2 counterpart (test_mobilenet_engine.py)
        np.testing.assert_allclose(a, ref, rtol=0, atol=1e-6 * np.abs(ref).max())


def test_cpu_metric_reports_generic_with_the_engine_reason(pruned):
    from torchpruner_amd import APoZAttributionMetric
    model, x, y = live_bn_v3(pruned)
    convs = _convs(model)[:2]
    m = APoZAttributionMetric(model, [(x, y)], F.cross_entropy, "cpu", mobilenet_engine=True)
    m.run_many(convs, find_best_evaluation_module=True)
    assert m.last_path["path"] == "generic", m.last_path
    assert any(r.startswith("mobilenet engine:") for r in m.last_path["reasons"]), m.last_path


def test_shapley_on_v3_reports_its_reason(pruned):
    from torchpruner_amd import ShapleyAttributionMetric
    from torchpruner_amd.engine.mobilenet_engine import V3_SHAPLEY_REASON
    from torchpruner_amd.utils import find_best_module_for_attributions
    model, x, y = live_bn_v3(pruned)
    conv = _convs(model)[0]
    m = ShapleyAttributionMetric(model, [(x[:2], y[:2])], F.cross_entropy, "cpu", sv_samples=1, mobilenet_engine=True)
    out = m.run(conv, find_best_evaluation_module=True)
    assert out.shape == (conv.weight.shape[0],)
    assert m.last_path["path"].startswith("generic"), m.last_path
    assert V3_SHAPLEY_REASON in m.last_path["reasons"] and "Shapley" in V3_SHAPLEY_REASON
    off = ShapleyAttributionMetric(model, [(x[:2], y[:2])], F.cross_entropy, "cpu", sv_samples=1)
    off.run(conv, find_best_evaluation_module=True)
    assert not any("mobilenet" in r for r in off.last_path["reasons"])
