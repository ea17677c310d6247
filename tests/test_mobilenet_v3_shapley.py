"""The identity behind Shapley prefixes on a gated MobileNetV3 block, in float64 on the CPU: the scales
and biases of ``_gated_operands`` pushed through ``ops.scaled_project``'s torch body equal masking,
pooling, gating, scaling and multiplying the explicit copies."""
import pytest
import torch


@pytest.mark.parametrize("code", [0, 1], ids=["hardsigmoid", "sigmoid"])
@pytest.mark.parametrize("zero_fill", [True, False], ids=["fill0", "fill"])
def test_gated_operands_equal_explicit_copies(zero_fill, code):
    from torchpruner_amd import ops
    from torchpruner_amd.engine.mobilenet_engine import _gated_operands
    g = torch.Generator().manual_seed(11 + code)
    B, HW, C, Cs, Co, n, p0, cnt = 3, 5, 24, 8, 12, 21, 7, 6  # channels n .. C-1 are padding: never masked
    f64 = dict(dtype=torch.float64, generator=g)
    y = torch.rand(B, HW, C, **f64) * 6
    y[:, :, n:] = 0
    fill = torch.zeros(C, dtype=torch.float64) if zero_fill else torch.rand(C, **f64) * 2
    fill[n:] = 0
    q = {"w1": torch.randn(Cs, C, **f64), "b1": torch.randn(Cs, **f64), "w2": torch.randn(C, Cs, **f64),
         "b2": torch.randn(C, **f64), "code": code}
    wt, shift, h = torch.randn(C, Co, **f64), torch.randn(Co, **f64), torch.randn(B * HW, Co, **f64)
    perm = torch.randperm(n, generator=g)
    rank = torch.full((C,), n + 1)
    rank[perm] = torch.arange(n)
    sc, bias = _gated_operands(rank, p0, cnt, y.mean(1), fill, q, wt, shift)
    got = ops.scaled_project(y.reshape(B * HW, C), sc, wt, bias, h, hw=HW)
    for j in range(cnt):
        yj = torch.where((rank < p0 + j).view(1, 1, C), fill, y)
        _, s = ops.se_gate_fwd(yj.mean(1), q["w1"], q["b1"], q["w2"], q["b2"], code)
        ref = (yj * s.unsqueeze(1)).reshape(B * HW, C) @ wt + shift + h
        assert (got[j] - ref).abs().max() <= 1e-12 * ref.abs().max()
    assert not torch.equal(got[0], got[-1])
