"""A pruned MobileNetV2 (odd hidden widths, C % 4 != 0) on the native kernels, depthwise layers
included: one training step against plain autograd, Taylor attribution on the generic path
against an fp64 CPU run, and the TORCHPRUNER_NATIVE_DW=0 switch in a fresh process."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pruned_mobilenet():
    """mobilenet_v2(10, width_mult=0.5, small_input=True) with every hidden width cut by
    30 % + 1 random units (built on the CPU; dropout off: the native Philox dropout draws other
    masks than ATen's)."""
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    from torchpruner_amd.models import mobilenet_v2
    torch.manual_seed(0)
    model = mobilenet_v2(10, width_mult=0.5, small_input=True)
    rng = np.random.RandomState(0)
    pruner = Pruner(model, (3, 32, 32), "cpu")
    for module, cascade in get_mobilenet_pruning_graph(model):
        n = module.weight.shape[0]
        pruner.prune_model(module, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


@pytest.fixture(scope="module")
def pruned():
    return _pruned_mobilenet()


def _depthwise(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.Conv2d) and m.groups != 1]


def _step(model, x, y, native):
    from torchpruner_amd.engine.train import native_convs
    model.zero_grad(set_to_none=True)
    with native_convs(model, enable=native):
        loss = F.cross_entropy(model(x), y)
        loss.backward()
    return float(loss.detach()), [p.grad.detach().double().cpu().clone() for p in model.parameters()]


def _mid_range_bn(model, gen):
    """BN scale in (0.5, 1), shift 3: the pre-activations of every ReLU6 (range 0..6) sit
    mid-range, 3 to 6 standard deviations from either kink.

    Why: two fp32 implementations round differently, and a pre-activation within rounding of a
    kink gets another ReLU6 decision, which switches one whole term of a weight-gradient sum
    on or off. With B = 4 at 32 px the late layers sum only 256 terms per channel, so ONE
    flipped decision moves a gradient entry by percents. At the default initialisation (shift
    0: the density of the pre-activations peaks at the kink, ~6 M activations per step) plain
    fp32 autograd itself misses the bounds below against fp64 autograd on the CPU by 6x - 38x
    on 8 of 8 data seeds (measured, MI355X), and the native step misses them against plain fp32
    autograd, the comparison asked for, by 7x - 77x on the same 8 seeds (14.6x on seed 5; with
    the depthwise kernels off, dense kernels only, by 6x - 28x) while agreeing with it in the
    loss to 1e-6: the comparison would measure flipped decisions, not kernels. With these BN
    parameters it is at 0.014 - 0.022 of the bounds on the 6 of 8 seeds where the library path
    itself has no flip against fp64. 3 standard deviations out, the density at a kink is ~90x lower or less."""
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) * 0.5 + 0.5)
                m.bias.fill_(3.0)


def _compare_step(base, dev, mid_range=True):
    """One training step (B = 4, 32 px, channels_last) on the native kernels vs plain autograd,
    with the bounds of test_native_conv_training_matches_autograd. Returns the DW_COUNTS deltas.
    Seed 5 (BN scales and data): plain fp32 autograd is at 0.02 of these bounds against fp64
    autograd on the CPU (measured; on 2 of 8 seeds tried the library path itself still flips a
    decision against fp64, which the native path on those seeds does not).
    ``mid_range=False``: the default initialisation; the gradients are then only required to be
    finite (see :func:`_mid_range_bn` for what they measure there), the loss and the running
    statistics, which a flipped decision moves by one rounding error, keep their bounds."""
    from torchpruner_amd.engine.train import DW_COUNTS
    gen = torch.Generator().manual_seed(5)
    model = copy.deepcopy(base)
    if mid_range:
        _mid_range_bn(model, gen)
    model = model.to(dev).to(memory_format=torch.channels_last).train()
    assert any(m.weight.shape[0] % 4 for m in _depthwise(model))
    x = torch.randn(4, 3, 32, 32, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (4,), generator=gen).to(dev)
    ref_model = copy.deepcopy(model)
    before = dict(DW_COUNTS)
    l_nat, g_nat = _step(model, x, y, True)
    delta = {k: DW_COUNTS[k] - before[k] for k in before}
    l_ref, g_ref = _step(ref_model, x, y, False)
    print(f"loss native {l_nat:.7f} autograd {l_ref:.7f}")
    assert abs(l_nat - l_ref) < 1e-4 * max(1.0, abs(l_ref))
    worst = 0.0
    for (name, _), a, b in zip(model.named_parameters(), g_nat, g_ref):
        err, lim = (a - b).abs().max().item(), 2e-3 * b.abs().max().item() + 1e-6
        worst = max(worst, err / lim)
        assert torch.isfinite(a).all(), name
        assert err <= lim or not mid_range, (name, err, lim)
    print(f"worst gradient error / bound: {worst:.3f}")
    for (n1, b1), (_, b2) in zip(model.named_buffers(), ref_model.named_buffers()):
        torch.testing.assert_close(b1.float(), b2.float(), rtol=1e-4, atol=1e-5, msg=n1)
    return delta, len(_depthwise(model))


def test_pruned_mobilenet_training_step_matches_autograd(cuda, pruned):
    delta, n_dw = _compare_step(pruned, cuda)
    assert n_dw == 17
    assert delta == {"fwd": n_dw, "dgrad": n_dw, "wgrad": n_dw}, delta


def test_pruned_mobilenet_default_init_step(cuda, pruned):
    """The same step at the default initialisation (BN shift 0: ReLU6 clamps half of every
    pre-activation): loss and BN running statistics against plain autograd within the issue's
    bounds, every depthwise kernel launched, gradients finite."""
    delta, n_dw = _compare_step(pruned, cuda, mid_range=False)
    assert delta == {"fwd": n_dw, "dgrad": n_dw, "wgrad": n_dw}, delta


def test_pruned_mobilenet_taylor_on_generic_path(cuda, pruned):
    """Taylor scores of three expand convs, evaluated after their ReLU6, on the generic path with
    every conv (dense and depthwise) on the native kernels, vs the same metric in fp64 on the CPU
    (bound and oracle as test_fmnist_generic_attribution_on_native_convs). Data seed 11: the
    library path (TORCHPRUNER_GENERIC_NATIVE=0) meets the same bound on it (checked once: 1.4e-7,
    5.3e-6, 3.4e-6 for the three layers; native 1.6e-7, 2.1e-5, 2.0e-5), so no ReLU6 decision
    flipped by fp32 rounding is what this measures (seed 14 misses it on both paths alike)."""
    from torchpruner_amd import TaylorAttributionMetric, get_mobilenet_pruning_graph
    from torchpruner_amd.data import DeviceLoader
    from torchpruner_amd.engine.train import dw_eligible, eligible
    model = copy.deepcopy(pruned).to(cuda).eval()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(16, 3, 32, 32, generator=gen).to(cuda)
    y = torch.randint(0, 10, (16,), generator=gen).to(cuda)
    pick = (0, 7, 15)
    graph = get_mobilenet_pruning_graph(model)
    mods = [graph[i][0] for i in pick]
    m = TaylorAttributionMetric(model, DeviceLoader(x, y, 8), F.cross_entropy, cuda)
    got = m.run_many(mods, find_best_evaluation_module=True)
    n_native = sum(eligible(c) or dw_eligible(c) for c in model.modules())
    assert n_native == sum(isinstance(c, torch.nn.Conv2d) for c in model.modules()) == 52
    assert m.last_path["path"] == "generic" and m.last_path["native_convs"] == n_native, m.last_path
    m64 = copy.deepcopy(model).double().cpu()
    mods64 = [get_mobilenet_pruning_graph(m64)[i][0] for i in pick]
    os.environ["TORCHPRUNER_BACKEND"] = "torch"
    try:
        ref = TaylorAttributionMetric(m64, DeviceLoader(x.double().cpu(), y.cpu(), 8), F.cross_entropy, "cpu").run_many(
            mods64, find_best_evaluation_module=True)
    finally:
        del os.environ["TORCHPRUNER_BACKEND"]
    for mod, a, e in zip(mods, got, ref):
        assert a.shape == e.shape == (mod.out_channels,)
        err = np.abs(a - e).max() / (np.abs(e).max() + 1e-30)
        print(f"{mod.out_channels} channels: rel. error {err:.3e}")
        assert err < 1e-4


def _ab_child():
    """(child process, TORCHPRUNER_NATIVE_DW=0) the step still matches and no depthwise kernel ran."""
    from torchpruner_amd import ops
    from torchpruner_amd.engine import train
    ops.require()
    assert not train._NATIVE_DW
    delta, n_dw = _compare_step(_pruned_mobilenet(), torch.device("cuda"))
    assert n_dw == 17 and delta == {"fwd": 0, "dgrad": 0, "wgrad": 0}, delta
    assert train.DW_COUNTS == {"fwd": 0, "dgrad": 0, "wgrad": 0}
    print("dw switch off ok")


def test_native_dw_switch_off_keeps_library_path(cuda):
    env = dict(os.environ, TORCHPRUNER_NATIVE_DW="0")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            "import test_mobilenet_gpu as t; t._ab_child()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dw switch off ok" in r.stdout
