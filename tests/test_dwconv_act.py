"""The PyTorch references of dwconv_act_fwd / dwconv_act_dgrad (torchpruner_amd/ops/dwconv_act.py) in
fp64 against autograd through hardtanh(affine(conv2d(hardtanh(z)))): they are the oracle of the GPU
kernel tests, so they are validated here, on the CPU, with exact 0.0 / 6.0 planted in z and in the
pre-activation of the output (hardtanh_backward: zero gradient at both ends)."""
import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops


def _case(k, s, pad, shape, seed):
    """z, w, scale, shift (fp64, NHWC z) with exact 0 / 6 in z and in the output's pre-activation:
    a channel whose centre tap is the only non-zero weight, with scale 1 and shift 0, copies the
    clamped input, planted values included."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 4 + 3
    w = torch.randn(C, 1, k, k, generator=g, dtype=torch.float64) * (1.5 / k)
    scale = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(C, generator=g, dtype=torch.float64) + 2
    w[0].zero_()
    w[0, 0, k // 2, k // 2] = 1.0
    scale[0], shift[0] = 1.0, 0.0
    flat = z.view(-1, C)
    flat[0::7, :] = 0.0
    flat[3::7, :] = 6.0
    return z, w, scale, shift


def _act(code, t):
    return t if code == 0 else F.relu(t) if code == 1 else F.hardtanh(t, 0.0, 6.0)


@pytest.mark.parametrize("k,s,pad", [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2), (3, 2, 0), (5, 1, 4)])
@pytest.mark.parametrize("in_act,out_act", [(0, 0), (0, 2), (2, 0), (2, 2), (2, 1), (1, 2)])
def test_reference_matches_autograd(k, s, pad, in_act, out_act):
    shape = (2, 7, 9, 8)
    z, w, scale, shift = _case(k, s, pad, shape, k * 10 + s)
    B, H, W, C = shape
    zl = z.clone().requires_grad_(True)
    a = _act(in_act, zl)
    a.retain_grad()
    pre = F.conv2d(a.permute(0, 3, 1, 2), w, None, s, pad, 1, C).permute(0, 2, 3, 1) * scale + shift
    y_ref = _act(out_act, pre)
    if in_act == 2 and out_act == 2 and pad == k // 2 and s == 1:  # the planted values reach the output's kinks
        assert (pre[..., 0] == 0).any() and (pre[..., 0] == 6).any()
    g = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    y_ref.backward(g)

    apoz = torch.zeros(B, C, dtype=torch.float64)
    y = ops.dwconv_act_fwd(z, w, scale, shift, s, pad, in_act, out_act, apoz)
    torch.testing.assert_close(y, y_ref.detach(), rtol=1e-10, atol=1e-12)
    assert torch.equal(apoz, (y_ref > 0).sum((1, 2)).double())
    R = ops.dwconv_act_tay_slots(H, W, C)
    assert R == H * 1
    for tay_mode in (0, 1):
        tay = torch.zeros(R, B, C, dtype=torch.float64)
        dz = ops.dwconv_act_dgrad(g, y, w, scale, z, H, W, s, pad, in_act, out_act, tay, tay_mode)
        torch.testing.assert_close(dz, zl.grad, rtol=1e-10, atol=1e-12)
        if in_act != 0:
            dead = (z <= 0) | (z >= 6) if in_act == 2 else z <= 0
            assert (dz[dead] == 0).all() and dead.any()
        term = a.grad.abs() if tay_mode else -(a.grad * a.detach())
        torch.testing.assert_close(tay.sum(0), term.sum((1, 2)), rtol=1e-10, atol=1e-12)
    assert ops.dwconv_act_dgrad(g, y, w, scale, z, H, W, s, pad, in_act, out_act).equal(dz)


def test_saturated_units_score_although_their_gradient_stops():
    """a == 6: Taylor takes 6 * dA and Sensitivity |dA| from the unmasked gradient, dz is zero."""
    z = torch.full((1, 3, 3, 4), 7.0, dtype=torch.float64)
    w = torch.zeros(4, 1, 3, 3, dtype=torch.float64)
    w[:, 0, 1, 1] = 1.0
    one, zero = torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    y = ops.dwconv_act_fwd(z, w, one * 0.5, zero, 1, 1, 2, 2)
    assert (y == 3).all()
    g = torch.ones_like(y)
    for mode, want in ((0, -6 * 0.5 * 9), (1, 0.5 * 9)):
        tay = torch.zeros(ops.dwconv_act_tay_slots(3, 3, 4), 1, 4, dtype=torch.float64)
        dz = ops.dwconv_act_dgrad(g, y, w, one * 0.5, z, 3, 3, 1, 1, 2, 2, tay, mode)
        assert (dz == 0).all() and torch.allclose(tay.sum(0), torch.full((1, 4), want, dtype=torch.float64))


def test_slot_helper_and_argument_checks():
    assert ops.dwconv_act_tay_slots(5, 36, 128) == 5 * 2 and ops.dwconv_act_tay_slots(7, 9, 32) == 7
    assert ops.dwconv_act_tay_slots(112, 112, 96) == 112 * 3
    assert ops.dwconv_act_tay_slots(4, 4, 6) == 0 and ops.dwconv_act_tay_slots(0, 4, 8) == 0
    z = torch.zeros(1, 4, 4, 8)
    w, v = torch.zeros(8, 1, 3, 3), torch.zeros(8)
    with pytest.raises(ValueError):
        ops.dwconv_act_fwd(z, w, v, v, 1, 1, 3, 0)
    with pytest.raises(ValueError):
        ops.dwconv_act_dgrad(z, z, w, v, z, 4, 4, 1, 1, 2, 2, torch.zeros(3, 1, 8), 0)
    with pytest.raises(ValueError):
        ops.dwconv_act_dgrad(z, z, w, v, z, 4, 4, 1, 1, 2, 2, torch.zeros(4, 1, 8), 2)
    x = torch.zeros(1, 4, 4, 8)
    x[0, 1, 1, 3] = float("nan")
    w[:, 0, 1, 1] = 1.0
    y = ops.dwconv_act_fwd(x, w, v + 1, v, 1, 1, 2, 2)
    nan = torch.isnan(y)  # every window that covers the pixel (0 * NaN is NaN), that channel only
    assert nan[0, :3, :3, 3].all() and nan.sum() == 9
