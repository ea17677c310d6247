"""EfficientNetV2 on the EfficientNet engine (Fused-MBConv blocks on the silu_project kernels), by the protocol
of tests/test_efficientnet_engine_gpu.py: ``efficientnet_v2(0.25, 0.34, 10, small_input=True)`` with 30 % + 1 of
every hidden width pruned (the fused blocks' too), random BN statistics and gate biases, one batch of 8 at
32 px. Measured worst per-layer errors: profiles/numerics/efficientnet_engine.txt (bound 1e-4)."""
import copy

import numpy as np
import pytest
import torch

from test_efficientnet_engine_gpu import _metric

pytestmark = pytest.mark.gpu

_SETUP = {}


@pytest.fixture
def setup(cuda):
    if not _SETUP:
        import torch.nn as nn
        from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
        from torchpruner_amd.models import efficientnet_v2
        torch.manual_seed(0)
        model = efficientnet_v2(0.25, 0.34, 10, small_input=True)
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
        x, y = torch.randn(8, 3, 32, 32, generator=gen), torch.randint(0, 10, (8,), generator=gen)
        ref = copy.deepcopy(model).double()
        convs = [m for m, _ in get_mobilenet_pruning_graph(model)]
        convs += [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups != 1]
        names = {id(m): n for n, m in model.named_modules()}
        refs = dict(ref.named_modules())
        _SETUP.update(model=model.to(cuda), x=x.to(cuda), y=y.to(cuda), convs=convs, ref=ref, x64=x.double(), y64=y,
                      ref_convs=[refs[names[id(c)]] for c in convs])
    return _SETUP


def test_logits_and_apoz(setup, cuda):
    from torchpruner_amd.engine import EfficientNetEngine, maybe_mobilenet_engine
    s = setup
    why = []
    eng = maybe_mobilenet_engine(s["model"], [], cuda, why=why)
    assert isinstance(eng, EfficientNetEngine), why
    fused = [b for b in eng.plan.blocks if b.dw is None and b.project is not None]
    assert len(fused) == 4 and any(eng.real_width(b.expand.act) % 4 for b in fused)
    with torch.no_grad():
        torch.testing.assert_close(eng.forward(s["x"]), s["model"](s["x"]), rtol=2e-3, atol=2e-3)
    on = _metric("apoz", s["model"], s["x"], s["y"], mobilenet_engine=True)
    got = on.run_many(s["convs"], find_best_evaluation_module=True)
    assert on.last_path["path"] == "mobilenet", on.last_path
    ref = _metric("apoz", s["model"], s["x"], s["y"]).run_many(s["convs"], find_best_evaluation_module=True)
    for c, a, b in zip(s["convs"], got, ref):
        assert a.shape == b.shape == (c.weight.shape[0],)
        np.testing.assert_allclose(a, b, atol=0.5)


@pytest.mark.parametrize("mode", ["taylor", "taylor_signed", "sensitivity"])
def test_gradient_scores_match_the_fp64_generic_path(setup, mode):
    s = setup
    m = _metric(mode, s["model"], s["x"], s["y"], mobilenet_engine=True, reduction="none")
    got = m.run_many(s["convs"], find_best_evaluation_module=True)
    assert m.last_path["path"] == "mobilenet", m.last_path
    ref = _metric(mode, s["ref"], s["x64"], s["y64"], reduction="none").run_many(
        s["ref_convs"], find_best_evaluation_module=True)
    worst = 0.0
    for c, a, r in zip(s["convs"], got, ref):
        assert a.shape == r.shape == (8, c.weight.shape[0])
        worst = max(worst, float(np.abs(a - r).max() / np.abs(r).max()))
    print(f"efficientnet_v2 engine {mode}: worst per-layer max abs error / max |ref| = {worst:.3e} (bound 1e-4)")
    assert worst <= 1e-4, worst
