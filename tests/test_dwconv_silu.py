"""The float64 PyTorch bodies of ops.dwconv_silu_* (the oracle of test_dwconv_silu_gpu.py) against
autograd through F.conv2d -> affine -> F.silu, and their operand validation."""
import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops


@pytest.mark.parametrize("in_act", [0, 4])
@pytest.mark.parametrize("shape,k,s,pad", [((2, 7, 9, 8), 3, 1, 1), ((2, 6, 5, 4), 5, 2, 2), ((1, 1, 1, 4), 3, 1, 1)])
def test_bodies_match_autograd(shape, k, s, pad, in_act):
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(k * 10 + s + in_act)
    z = (torch.randn(shape, dtype=torch.float64, generator=gen) * 2).requires_grad_()
    a = F.silu(z) if in_act else z
    a.retain_grad()
    w = torch.randn(C, 1, k, k, dtype=torch.float64, generator=gen)
    scale, shift = torch.rand(C, dtype=torch.float64, generator=gen) + 0.5, torch.randn(C, dtype=torch.float64, generator=gen)
    v_ref = F.conv2d(a.permute(0, 3, 1, 2), w, None, s, pad, 1, C).permute(0, 2, 3, 1) * scale + shift
    y_ref = F.silu(v_ref)
    g = torch.randn(y_ref.shape, dtype=torch.float64, generator=gen)
    (y_ref * g).sum().backward()

    Ho, Wo = y_ref.shape[1:3]
    apoz, pre = torch.zeros(B, C, dtype=torch.float64), torch.empty_like(y_ref)
    pool = torch.zeros(ops.dwconv_silu_pool_slots(Ho, Wo, C), B, C, dtype=torch.float64)
    zd = z.detach()
    y = ops.dwconv_silu_fwd(zd, w, scale, shift, s, pad, in_act, 4, apoz, pre, pool)
    torch.testing.assert_close(y, y_ref.detach())
    torch.testing.assert_close(pre, v_ref.detach())
    torch.testing.assert_close(pool.sum(0), y_ref.detach().sum((1, 2)))
    assert torch.equal(apoz, (y_ref > 0).sum((1, 2)).double())
    for mode, term in ((0, -(a.grad * a.detach())), (1, a.grad.abs())):
        tay = torch.zeros(ops.dwconv_silu_tay_slots(H, W, C), B, C, dtype=torch.float64)
        dz = ops.dwconv_silu_dgrad(g, pre, w, scale, zd, H, W, s, pad, in_act, 4, tay, mode)
        torch.testing.assert_close(dz, z.grad)
        torch.testing.assert_close(tay.sum(0), term.sum((1, 2)))


def test_slot_counts():
    assert ops.dwconv_silu_tay_slots(7, 7, 32) == 2 and ops.dwconv_silu_pool_slots(112, 112, 32) == 28 * 4
    assert ops.dwconv_silu_tay_slots(1, 1, 4) == 1 and ops.dwconv_silu_tay_slots(5, 33, 8) == 2
    assert ops.dwconv_silu_tay_slots(7, 7, 6) == 0 and ops.dwconv_silu_pool_slots(0, 7, 8) == 0


def test_bad_operands_raise():
    z, w, v = torch.zeros(1, 4, 4, 8), torch.zeros(8, 1, 3, 3), torch.zeros(8)
    for in_act, out_act in [(3, 4), (1, 4), (4, 0), (0, 3)]:
        with pytest.raises(ValueError, match="activation codes"):
            ops.dwconv_silu_fwd(z, w, v, v, 1, 1, in_act, out_act)
        with pytest.raises(ValueError, match="activation codes"):
            ops.dwconv_silu_dgrad(z, z, w, v, z, 4, 4, 1, 1, in_act, out_act)
    with pytest.raises(ValueError, match="slab"):
        ops.dwconv_silu_fwd(z, w, v, v, 1, 1, 4, 4, pool=torch.zeros(2, 1, 8))
    with pytest.raises(ValueError, match="slab"):
        ops.dwconv_silu_dgrad(z, z, w, v, z, 4, 4, 1, 1, 4, 4, torch.zeros(1, 2, 8))
    with pytest.raises(ValueError, match="tay_mode"):
        ops.dwconv_silu_dgrad(z, z, w, v, z, 4, 4, 1, 1, 4, 4, torch.zeros(1, 1, 8), 2)
    with pytest.raises(ValueError, match="pre must"):
        ops.dwconv_silu_fwd(z, w, v, v, 1, 1, 4, 4, pre=torch.zeros(1, 4, 4, 4))
