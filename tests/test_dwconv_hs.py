"""The PyTorch references of dwconv_hs_fwd / dwconv_hs_dgrad (torchpruner_amd/ops/dwconv_hs.py) in
fp64 against autograd through act(affine(conv2d(act(z)))) with F.hardswish / F.relu / F.relu6: they
are the oracle of the GPU kernel tests, so they are validated here, on the CPU. Exact 0.0 (the ReLU
kink) is planted in z and, through a copy channel, in the output's pre-activation. At exactly -3 and
3 the derivative is the middle branch's (0 if v < -3; v / 3 + 0.5 if v <= 3; else 1, the order of
ATen's hardswish_backward on the GPU and of ops.bn_hswish_bwd); ATen's vectorised CPU kernel takes
the outer branches there (0 and 1), so those two points are checked against the formula in a test
of their own and kept out of the autograd comparison (random fp64 values never hit them)."""
import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops

PAIRS = [(3, 3), (3, 1), (1, 3), (0, 3), (3, 0)]


def _case(k, s, pad, shape, seed):
    """z, w, scale, shift (fp64, NHWC z) with exact 0 in z; channel 0 (centre tap 1, affine (1, 0))
    copies the activated input into the output's pre-activation."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 4
    w = torch.randn(C, 1, k, k, generator=g, dtype=torch.float64) * (1.5 / k)
    scale = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(C, generator=g, dtype=torch.float64)
    w[0].zero_()
    w[0, 0, k // 2, k // 2] = 1.0
    scale[0], shift[0] = 1.0, 0.0
    flat = z.view(-1, C)
    flat[0::7, :] = 0.0
    return z, w, scale, shift


def _act(code, t):
    return t if code == 0 else F.relu(t) if code == 1 else F.relu6(t) if code == 2 else F.hardswish(t)


@pytest.mark.parametrize("k,s,pad", [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2), (3, 2, 0), (5, 1, 4)])
@pytest.mark.parametrize("in_act,out_act", PAIRS)
def test_reference_matches_autograd(k, s, pad, in_act, out_act):
    shape = (2, 7, 9, 8)
    z, w, scale, shift = _case(k, s, pad, shape, k * 10 + s)
    B, H, W, C = shape
    zl = z.clone().requires_grad_(True)
    a = _act(in_act, zl)
    a.retain_grad()
    pre_ref = F.conv2d(a.permute(0, 3, 1, 2), w, None, s, pad, 1, C).permute(0, 2, 3, 1) * scale + shift
    y_ref = _act(out_act, pre_ref)
    if pad == k // 2 and s == 1:  # the planted zeros reach the output's pre-activation (act(0) == 0)
        assert (pre_ref[..., 0] == 0).any()
    assert not ((zl.abs() == 3).any() or (pre_ref.abs() == 3).any())
    g = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    y_ref.backward(g)

    apoz = torch.zeros(B, C, dtype=torch.float64)
    pre = torch.full_like(y_ref, float("nan"))
    y = ops.dwconv_hs_fwd(z, w, scale, shift, s, pad, in_act, out_act, apoz, pre)
    torch.testing.assert_close(y, y_ref.detach(), rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(pre, pre_ref.detach(), rtol=1e-10, atol=1e-12)
    assert torch.equal(apoz, (y_ref > 0).sum((1, 2)).double())
    assert torch.equal(ops.dwconv_hs_fwd(z, w, scale, shift, s, pad, in_act, out_act), y)
    R = ops.dwconv_hs_tay_slots(H, W, C)
    assert R == H * 1 == ops.dwconv_act_tay_slots(H, W, C)
    saved = pre if out_act == 3 else y  # what the dgrad reads the output's derivative from
    for tay_mode in (0, 1):
        tay = torch.zeros(R, B, C, dtype=torch.float64)
        dz = ops.dwconv_hs_dgrad(g, saved, w, scale, z, H, W, s, pad, in_act, out_act, tay, tay_mode)
        torch.testing.assert_close(dz, zl.grad, rtol=1e-10, atol=1e-12)
        if in_act == 3:
            assert (dz[z < -3] == 0).all() and (z < -3).any()
        if in_act == 1:
            assert (dz[z <= 0] == 0).all()
        term = a.grad.abs() if tay_mode else -(a.grad * a.detach())
        torch.testing.assert_close(tay.sum(0), term.sum((1, 2)), rtol=1e-10, atol=1e-12)
        assert (tay[1:] == 0).all()  # the reference puts the whole sum into slot 0
    assert ops.dwconv_hs_dgrad(g, saved, w, scale, z, H, W, s, pad, in_act, out_act).equal(dz)


def test_derivative_at_the_kinks_follows_atens_branch_order():
    """v = -3 and v = 3 take the middle branch: d(-3) = -0.5 (not 0), d(3) = 1.5 (not 1); just
    outside they take 0 and 1. Checked on the input side (dz / dA) and on the output side."""
    v = torch.tensor([-3.0, 3.0, -3.0 - 1e-9, 3.0 + 1e-9, 0.0], dtype=torch.float64)
    want = torch.tensor([-0.5, 1.5, 0.0, 1.0, 0.5], dtype=torch.float64)
    z = v.view(1, 1, 5, 1).repeat(1, 1, 1, 4).contiguous()
    w = torch.zeros(4, 1, 3, 3, dtype=torch.float64)
    w[:, 0, 1, 1] = 1.0
    one, zero = torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    g = torch.ones(1, 1, 5, 4, dtype=torch.float64)
    # input side: identity conv, no output activation: dA = 1, dz = d(z)
    dz = ops.dwconv_hs_dgrad(g, g, w, one, z, 1, 5, 1, 1, 3, 0)
    assert torch.equal(dz[0, 0, :, 0], want)
    # output side: identity conv of the raw input: pre == z, dz = d(pre)
    pre = torch.empty_like(z)
    y = ops.dwconv_hs_fwd(z, w, one, zero, 1, 1, 0, 3, None, pre)
    assert torch.equal(pre, z)
    torch.testing.assert_close(y, F.hardswish(z), rtol=1e-12, atol=1e-14)
    dz = ops.dwconv_hs_dgrad(g, pre, w, one, z, 1, 5, 1, 1, 0, 3)
    assert torch.equal(dz[0, 0, :, 0], want)
    # away from the two points ATen's CPU kernel agrees
    zl = z.clone().requires_grad_(True)
    F.hardswish(zl).backward(g)
    assert torch.equal(zl.grad[0, 0, 2:, 0], want[2:])


@pytest.mark.parametrize("in_act,out_act", [(0, 0), (0, 2), (2, 0), (2, 2), (2, 1), (1, 2)])
@pytest.mark.parametrize("k,s,pad", [(3, 1, 1), (5, 2, 2)])
def test_codes_0_to_2_equal_dwconv_act_exactly(k, s, pad, in_act, out_act):
    B, H, W, C = shape = (2, 7, 9, 8)
    z, w, scale, shift = _case(k, s, pad, shape, 7)
    z = z + 3  # populate the ReLU6 regions
    z.view(-1, C)[1::7, :] = 6.0
    a1, a2 = torch.zeros(B, C, dtype=torch.float64), torch.zeros(B, C, dtype=torch.float64)
    y1 = ops.dwconv_act_fwd(z, w, scale, shift, s, pad, in_act, out_act, a1)
    pre = torch.empty_like(y1)
    y2 = ops.dwconv_hs_fwd(z, w, scale, shift, s, pad, in_act, out_act, a2, pre)
    assert torch.equal(y1, y2) and torch.equal(a1, a2)
    assert torch.equal(pre, ops.dwconv_act_fwd(z, w, scale, shift, s, pad, in_act, 0))
    g = torch.randn(y1.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    R = ops.dwconv_act_tay_slots(H, W, C)
    for mode in (0, 1):
        t1, t2 = torch.zeros(R, B, C, dtype=torch.float64), torch.zeros(R, B, C, dtype=torch.float64)
        d1 = ops.dwconv_act_dgrad(g, y1, w, scale, z, H, W, s, pad, in_act, out_act, t1, mode)
        d2 = ops.dwconv_hs_dgrad(g, y2, w, scale, z, H, W, s, pad, in_act, out_act, t2, mode)
        assert torch.equal(d1, d2) and torch.equal(t1, t2)


def test_argument_checks_and_nan():
    z = torch.zeros(1, 4, 4, 8)
    w, v = torch.zeros(8, 1, 3, 3), torch.zeros(8)
    for ia, oa in ((4, 0), (0, 4), (-1, 3)):
        with pytest.raises(ValueError):
            ops.dwconv_hs_fwd(z, w, v, v, 1, 1, ia, oa)
        with pytest.raises(ValueError):
            ops.dwconv_hs_dgrad(z, z, w, v, z, 4, 4, 1, 1, ia, oa)
    with pytest.raises(ValueError):
        ops.dwconv_hs_dgrad(z, z, w, v, z, 4, 4, 1, 1, 3, 3, torch.zeros(3, 1, 8), 0)
    with pytest.raises(ValueError):
        ops.dwconv_hs_dgrad(z, z, w, v, z, 4, 4, 1, 1, 3, 3, torch.zeros(4, 1, 8), 2)
    with pytest.raises(ValueError):
        ops.dwconv_hs_fwd(z, w, v, v, 1, 1, 3, 3, None, torch.zeros(1, 4, 4, 4))
    with pytest.raises(ValueError):  # the ReLU6-only op keeps rejecting Hardswish
        ops.dwconv_act_fwd(z, w, v, v, 1, 1, 3, 0)
    x = torch.zeros(1, 4, 4, 8)
    x[0, 1, 1, 3] = float("nan")
    w[:, 0, 1, 1] = 1.0
    pre = torch.zeros(1, 4, 4, 8)
    y = ops.dwconv_hs_fwd(x, w, v + 1, v, 1, 1, 3, 3, None, pre)
    for t in (y, pre):
        nan = torch.isnan(t)  # every window that covers the pixel (0 * NaN is NaN), that channel only
        assert nan[0, :3, :3, 3].all() and nan.sum() == 9
