"""CPU checks of Shapley on the MobileNet engine: the algebra of ``ops.prefix_project`` (its PyTorch
body in float64 is the kernel's oracle), the fill value a masked post-expand channel leaves in the
post-depthwise output, and the hook path that still serves a machine without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from torchpruner_amd import ops


def _operands(N, C, Co, n, zero_fill, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(N, C, generator=g, dtype=torch.float64) * 6
    fill = torch.zeros(C, dtype=torch.float64) if zero_fill else torch.rand(C, generator=g, dtype=torch.float64) * 6
    wt = torch.randn(C, Co, generator=g, dtype=torch.float64)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    rank = torch.full((C,), n + 1, dtype=torch.int64)  # the padded tail ranks after every real channel
    rank[perm.long()] = torch.arange(n)
    shortcut = torch.randn(N, Co, generator=g, dtype=torch.float64)
    return a, fill, wt, perm, rank, shortcut


@pytest.mark.parametrize("zero_fill", [True, False], ids=["fill0", "fill"])
@pytest.mark.parametrize("C,n", [(24, 24), (24, 17)], ids=["full", "padded_tail"])
@pytest.mark.parametrize("cnt", [1, 2, 7])
def test_prefix_project_is_the_masked_project_conv(zero_fill, C, n, cnt):
    N, Co = 10, 8
    a, fill, wt, perm, rank, shortcut = _operands(N, C, Co, n, zero_fill)

    def filled(p):
        return torch.where((rank < p).view(1, C), fill.view(1, C), a)

    for p0 in (0, 1, n - cnt + 1):
        base = filled(p0) @ wt + shortcut
        out = ops.prefix_project(base, a, fill, wt, perm, p0, cnt)
        assert out.shape == (cnt, N, Co) and out.dtype == torch.float64
        assert torch.equal(out[0], base)
        for j in range(cnt):
            want = filled(p0 + j) @ wt + (base - filled(p0) @ wt)
            assert (out[j] - want).abs().max() <= 1e-12 * want.abs().max(), (p0, j)
            if n < C:  # no prefix touches the padded tail
                assert torch.equal(filled(p0 + j)[:, rank > n], a[:, rank > n])


def test_prefix_project_rejects_bad_arguments():
    a, fill, wt, perm, _, sc = _operands(10, 24, 8, 17, False)
    for p0, cnt in ((0, 0), (-1, 2), (17, 2), (0, 19)):
        with pytest.raises(ValueError):
            ops.prefix_project(sc, a, fill, wt, perm, p0, cnt)
    with pytest.raises(ValueError):
        ops.prefix_project(sc[:, :6].contiguous(), a, fill, wt[:, :6].contiguous(), perm, 0, 2)  # Co % 4
    with pytest.raises(ValueError):
        ops.prefix_project(sc, a[:, :12].contiguous(), fill[:12], wt[:12], perm, 0, 2)  # n > C


@pytest.mark.parametrize("stride", [1, 2])
def test_masked_expand_channel_becomes_the_clamped_shift(stride):
    """Zeroing post-expand channels S leaves the post-depthwise output at clamp(shift_c, 0, 6) on S
    (zero padding included) and untouched elsewhere, exactly."""
    g = torch.Generator().manual_seed(5)
    C = 12
    expand = nn.Sequential(nn.Conv2d(5, C, 1, bias=False), nn.BatchNorm2d(C), nn.ReLU6())
    dw = nn.Sequential(nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False), nn.BatchNorm2d(C), nn.ReLU6())
    net = nn.Sequential(expand, dw).double().eval()
    with torch.no_grad():
        for seq in (expand, dw):
            seq[1].weight.copy_(torch.rand(C, generator=g) + 0.75)
            seq[1].running_mean.copy_(torch.randn(C, generator=g) * 0.2)
            seq[1].running_var.copy_(torch.rand(C, generator=g) + 0.5)
        expand[1].bias.copy_(torch.rand(C, generator=g) * 2)
        dw[1].bias.copy_(torch.linspace(-3.0, 9.0, C).double())  # folded shift below 0, inside (0, 6), above 6
        bn = dw[1]
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale
        assert (shift < 0).any() and ((shift > 0) & (shift < 6)).any() and (shift > 6).any()
        x = torch.randn(3, 5, 7, 7, generator=g, dtype=torch.float64)
        z = expand(x)
        y0 = dw(z)
        S = torch.tensor([0, 3, 4, 7, 11])
        assert (shift[S] < 0).any() and ((shift[S] > 0) & (shift[S] < 6)).any() and (shift[S] > 6).any()
        zm = z.clone()
        zm[:, S] = 0.0
        got = dw(zm)
        # the BN module's own arithmetic at a zero input: (0 - mean) / sqrt(var + eps) * weight + bias
        fill = F.batch_norm(torch.zeros(1, C, 1, 1, dtype=torch.float64), bn.running_mean, bn.running_var, bn.weight,
                            bn.bias, False, 0.0, bn.eps).clamp(0.0, 6.0)
        torch.testing.assert_close(fill.view(C), shift.clamp(0.0, 6.0), rtol=1e-14, atol=1e-14)
        in_s = torch.zeros(C, dtype=torch.bool)
        in_s[S] = True
        want = torch.where(in_s.view(1, C, 1, 1), fill, y0)
        assert torch.equal(got, want)
        assert not torch.equal(got, y0)


def test_engine_switched_on_without_a_gpu_takes_the_hook_path():
    from torchpruner_amd import ShapleyAttributionMetric, get_mobilenet_pruning_graph
    from torchpruner_amd.models import mobilenet_v2
    torch.manual_seed(0)
    model = mobilenet_v2(10, width_mult=0.5, small_input=True).eval()
    data = [(torch.randn(2, 3, 32, 32), torch.randint(0, 10, (2,)))]
    module = get_mobilenet_pruning_graph(model)[-1][0]
    runs = []
    for on in (True, None):
        metric = ShapleyAttributionMetric(model, data, F.cross_entropy, "cpu", sv_samples=1, mobilenet_engine=on)
        np.random.seed(3)
        runs.append(metric.run(module, find_best_evaluation_module=True))
        assert metric.last_path["path"] == "generic-hook", metric.last_path
        assert any(r.startswith("mobilenet engine:") for r in metric.last_path["reasons"]) == bool(on)
    np.testing.assert_array_equal(runs[0], runs[1])
    assert runs[0].shape == (48,) and np.abs(runs[0]).max() > 0


def test_engine_locates_its_evaluation_modules():
    from torchpruner_amd.engine.mobilenet_engine import MobileNetEngine, build_mobilenet_plan
    from torchpruner_amd.models import mobilenet_v2
    model = mobilenet_v2(10, width_mult=0.5, small_input=True).eval()
    plan, why = build_mobilenet_plan(model)
    assert plan is not None, why
    eng = MobileNetEngine(model, plan)
    kinds = [eng.locate(m) for m in eng.eval_modules()]
    assert kinds[0] == (0, "dw") and kinds[1:3] == [(1, "expand"), (1, "dw")] and len(kinds) == 33
    with pytest.raises(KeyError):
        eng.locate(model.features[0][2])
    # the largest activation downstream of a block's output, in padded elements per sample
    last = len(plan.blocks) - 1
    with torch.no_grad():
        _, c, H, W = model.features[:-1](torch.zeros(1, 3, 32, 32)).shape  # the last block's output
    head = plan.head.conv.weight.shape[0]
    assert head % 32 == 0 and head > c
    assert eng.downstream_elems(last, (3, 32, 32)) == H * W * head
    assert eng.downstream_elems(0, (3, 32, 32)) >= eng.downstream_elems(last, (3, 32, 32))
