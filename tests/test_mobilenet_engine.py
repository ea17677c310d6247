"""MobileNet engine, the parts that need no GPU: the plan builder (what it accepts, what it rejects
and why), the opt-in dispatch falling back to the generic path with the engine's reason, the fp64
oracle against the generic metric, and the GPU test's model actually exercising both ReLU6 kinks."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_mobilenet_engine_gpu import _live_bn_model
from test_mobilenet_gpu import _pruned_mobilenet


@pytest.fixture(scope="module")
def pruned():
    return _pruned_mobilenet()


def test_plan_accepts_dense_and_pruned(pruned):
    from torchpruner_amd.engine import build_mobilenet_plan
    from torchpruner_amd.models import mobilenet_v2
    dense = mobilenet_v2(10, 0.5, small_input=True)
    for model in (dense, pruned, mobilenet_v2(1000)):
        plan, why = build_mobilenet_plan(model)
        assert plan is not None, why
        assert len(plan.blocks) == 17 and plan.blocks[0].expand is None
        assert [b.shortcut for b in plan.blocks] == [m.use_res_connect for m in list(model.features)[1:-1]]
    # widths come from the tensors: the pruned hidden widths are no multiples of 4
    hidden = [b.dw.conv.weight.shape[0] for b in build_mobilenet_plan(pruned)[0].blocks]
    assert any(h % 4 for h in hidden) and hidden != [b.dw.conv.weight.shape[0]
                                                      for b in build_mobilenet_plan(dense)[0].blocks]
    # the shortcut is inferred (stride 1, equal widths) where the attribute is absent
    bare = copy.deepcopy(dense)
    want = [m.use_res_connect for m in list(bare.features)[1:-1]]
    for m in list(bare.features)[1:-1]:
        del m.use_res_connect
    assert [b.shortcut for b in build_mobilenet_plan(bare)[0].blocks] == want


def test_plan_rejects_with_a_reason():
    from torchpruner_amd.engine import build_mobilenet_plan
    from torchpruner_amd.models import mobilenet_v2, resnet18
    plan, why = build_mobilenet_plan(resnet18(10))
    assert plan is None and "MobileNetV2" in why
    base = mobilenet_v2(10, 0.5, small_input=True)
    m = copy.deepcopy(base)
    m.features[3].conv[0][2] = torch.nn.Hardswish()
    plan, why = build_mobilenet_plan(m)
    assert plan is None and "Hardswish" in why and "features.3" in why
    m = copy.deepcopy(base)
    dw = m.features[4].conv[1][0]
    dw.dilation, dw.padding = (2, 2), (2, 2)
    plan, why = build_mobilenet_plan(m)
    assert plan is None and "dilation" in why
    m = copy.deepcopy(base)  # depth multiplier 2
    old = m.features[2].conv[1][0]
    m.features[2].conv[1][0] = torch.nn.Conv2d(old.in_channels, 2 * old.in_channels, 3, 1, 1, groups=old.in_channels,
                                               bias=False)
    plan, why = build_mobilenet_plan(m)
    assert plan is None and "depth multiplier" in why
    m = copy.deepcopy(base)  # another grouped conv
    old = m.features[2].conv[0][0]
    m.features[2].conv[0][0] = torch.nn.Conv2d(old.in_channels, old.out_channels, 1, groups=2, bias=False)
    plan, why = build_mobilenet_plan(m)
    assert plan is None and "grouped" in why


def test_metric_on_cpu_reports_generic_with_the_engines_reason(pruned):
    from torchpruner_amd import TaylorAttributionMetric, get_mobilenet_pruning_graph
    from torchpruner_amd.data import DeviceLoader
    model = copy.deepcopy(pruned).eval()
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 10, (4,), generator=g)
    mods = [get_mobilenet_pruning_graph(model)[0][0]]
    m = TaylorAttributionMetric(model, DeviceLoader(x, y, 4), F.cross_entropy, "cpu", mobilenet_engine=True)
    m.run_many(mods, find_best_evaluation_module=True)
    assert m.last_path["path"] == "generic"
    assert any(r.startswith("mobilenet engine:") for r in m.last_path["reasons"]), m.last_path
    # off (the default): the engine is not even consulted
    m = TaylorAttributionMetric(model, DeviceLoader(x, y, 4), F.cross_entropy, "cpu")
    m.run_many(mods, find_best_evaluation_module=True)
    assert m.last_path["path"] == "generic"
    assert not any("mobilenet" in r for r in m.last_path["reasons"]), m.last_path


@pytest.mark.parametrize("mode", ["taylor", "taylor_signed", "sensitivity"])
def test_unconditioned_oracle_equals_the_generic_metric_in_fp64(pruned, mode):
    from torchpruner_amd import SensitivityAttributionMetric, TaylorAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    from torchpruner_amd.engine import build_mobilenet_plan
    from torchpruner_amd.engine.oracle import mobilenet_scores_fp64
    model, x, y = _live_bn_model(pruned)
    m64 = copy.deepcopy(model).double()
    plan = build_mobilenet_plan(m64)[0]
    ev = [a for b in plan.blocks for a in (([b.expand.act] if b.expand is not None else []) + [b.dw.act])]
    convs = [c for b in plan.blocks for c in (([b.expand.conv] if b.expand is not None else []) + [b.dw.conv])]
    assert len(ev) == 33
    if mode == "sensitivity":
        metric = SensitivityAttributionMetric(m64, DeviceLoader(x.double(), y, 8), F.cross_entropy, "cpu",
                                              reduction="none")
    else:
        metric = TaylorAttributionMetric(m64, DeviceLoader(x.double(), y, 8), F.cross_entropy, "cpu", reduction="none",
                                         signed=mode == "taylor_signed")
    got = metric.run_many(convs, find_best_evaluation_module=True)
    scores, flips, totals = mobilenet_scores_fp64(None, m64, x, y, mode, conditioned=False)
    assert flips == {} and totals == {}
    for mod, a in zip(ev, got):
        ref = scores[mod].numpy()
        assert a.shape == ref.shape
        # the generic path hands the criterion float32 logits (base.py: criterion(out.float(), y)), so
        # dL/dlogits carries float32 rounding (2^-24 per logit, a few ulp through the softmax) even
        # in a float64 model; the scores are linear in it: 1e-6 of the layer's largest score
        np.testing.assert_allclose(a, ref, rtol=0, atol=1e-6 * np.abs(ref).max())


def test_gpu_test_model_exercises_both_kinks(pruned):
    """With the BN statistics of the GPU test both ReLU6 kinks are live at the post-expand ReLU6 of
    every block from the second on (the default initialisation saturates nothing, and the upper
    kink would go untested)."""
    model, x, _ = _live_bn_model(pruned)
    sat = {}
    hooks = [m.register_forward_hook(lambda mod, inp, out, n=n: sat.__setitem__(n, (
        float((inp[0] <= 0).float().mean()), float((inp[0] >= 6).float().mean()))))
        for n, m in model.named_modules() if isinstance(m, torch.nn.ReLU6)]
    for m in model.modules():
        if isinstance(m, torch.nn.ReLU6):
            m.inplace = False
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    blocks = {n: v for n, v in sat.items() if n.startswith("features.") and 2 <= int(n.split(".")[1]) <= 17}
    expand = [v for n, v in blocks.items() if n.endswith("conv.0.2")]
    dw = [v for n, v in blocks.items() if n.endswith("conv.1.2")]
    assert len(expand) == len(dw) == 16
    # post-expand (the input of the depthwise kernels): a quarter to a half <= 0, 1.5 - 21 % >= 6
    assert all(lo > 0.15 and hi > 0.01 and 1 - lo - hi > 0.25 for lo, hi in expand), expand
    # post-depthwise: the lower kink only (4 - 14 % <= 0, nothing saturates); the upper kink of the
    # kernels' output mask is covered by test_dwconv_act_gpu.py, where exact 6.0 outputs are planted
    assert all(lo > 0.03 for lo, _ in dw), dw
    default = _pruned_mobilenet().eval()
    hi = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: hi.append(float((inp[0] >= 6).float().mean())))
             for m in default.modules() if isinstance(m, torch.nn.ReLU6)]
    with torch.no_grad():
        default(x)
    assert max(hi) == 0.0
