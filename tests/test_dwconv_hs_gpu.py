"""tpamd.dwconv_hs_fwd / dwconv_hs_dgrad (the Hardswish-aware entry points of
csrc/kernels/dwconv_act.hip) against their fp64 PyTorch references (validated against autograd in
test_dwconv_hs.py) fed the same fp32 inputs. The derivative factors are functions of stored tensors
(z, and the kernel's own stored y / pre-activation, which the reference takes too), so no decision
can flip between the two: bounds are arithmetic only. Shapes and (k, stride, pad) lists are those of
test_dwconv_act_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = [(3, 3), (3, 1), (1, 3), (0, 3), (3, 0)]
OLD_ACTS = [(0, 0), (0, 2), (2, 0), (2, 2), (2, 1)]
SHAPES = [((3, 7, 9, 32), [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2)]),
          ((2, 8, 8, 64), [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2)]),
          ((2, 5, 36, 128), [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2)]),
          ((2, 5, 5, 32), [(3, 2, 2), (5, 2, 2)])]
CASES = [(shape, ksp) for shape, lst in SHAPES for ksp in lst]


def _ref_act(code, t):
    return t if code == 0 else t.clamp(min=0) if code == 1 else t * (t + 3).clamp(0, 6) / 6


def _inputs(shape, k, s, pad, in_act, out_act, seed):
    """fp32 inputs: z ~ N(0, 4^2) with exact -3.0 / 0.0 / 3.0 planted; weights and affine that centre
    the output's pre-activation on 0 with std >= 3.5; channel 0 copies the activated input (centre
    tap 1, affine (1, 0)), so with in_act == 0 the planted values reach the pre-activation; 4 padded
    channels at the end (zero weights and affine, garbage z)."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, H, W, C, generator=g) * 4
    w = torch.randn(C, 1, k, k, generator=g) * (1.2 / k)
    scale = torch.rand(C, generator=g) + 1.75
    a = _ref_act(in_act, z)
    mean = torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), w, None, s, pad, 1, C).mean((0, 2, 3))
    shift = -mean * scale + torch.randn(C, generator=g) * 0.5
    w[0].zero_()
    w[0, 0, k // 2, k // 2] = 1.0
    scale[0], shift[0] = 1.0, 0.0
    flat = z.view(-1, C)
    flat[0::11, :] = 0.0
    flat[3::11, :] = -3.0
    flat[7::11, :] = 3.0
    w[C - 4:].zero_()
    scale[C - 4:], shift[C - 4:] = 0.0, 0.0
    z[..., C - 4:] = torch.randn(B, H, W, 4, generator=g) * 1e3  # garbage under the padding
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    gr = torch.randn(B, Ho, Wo, C, generator=g)
    return z, w, scale, shift, gr


def _populated(code, t, lo=0.10):
    """Every region of the activation holds >= lo of t (Hardswish: < -3, middle, > 3; ReLU: <= 0, > 0)."""
    n = t.numel()
    if code == 3:
        return (t < -3).sum() >= lo * n and (t > 3).sum() >= lo * n and ((t >= -3) & (t <= 3)).sum() >= lo * n
    if code == 1:
        return (t <= 0).sum() >= lo * n and (t > 0).sum() >= lo * n
    return True


@pytest.mark.parametrize("in_act,out_act", ACTS)
@pytest.mark.parametrize("shape,ksp", CASES)
def test_dwconv_hs_kernels(cuda, shape, ksp, in_act, out_act):
    from torchpruner_amd import ops
    T = ops.require()
    k, s, pad = ksp
    B, H, W, C = shape
    z, w, scale, shift, g = _inputs(shape, k, s, pad, in_act, out_act, 100 * k + 10 * s + in_act * 4 + out_act)
    real = slice(0, C - 4)
    d = lambda t: t.double()
    # fp64 reference on the same fp32 inputs
    apoz_ref = torch.zeros(B, C, dtype=torch.float64)
    pre_ref = torch.empty(B, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1, C, dtype=torch.float64)
    y_ref = ops.dwconv_hs_fwd(d(z), d(w), d(scale), d(shift), s, pad, in_act, out_act, apoz_ref, pre_ref)
    body = pre_ref[..., 1:C - 4]
    assert _populated(in_act, z[..., real]) and _populated(out_act, body), "an activation region is under-populated"
    assert body.std() >= 3.5 and body.mean().abs() <= 0.5
    assert (z == -3).any() and (z == 0).any() and (z == 3).any()
    if in_act == 0 and s == 1 and pad == k // 2:  # channel 0 copies the input, planted kinks included
        assert all((pre_ref[..., 0] == v).any() for v in (-3.0, 0.0, 3.0))

    zc, wc, scc, shc, gc = (t.to(cuda) for t in (z, w, scale, shift, g))
    apoz = torch.zeros(B, C, device=cuda)
    pre = torch.full(pre_ref.shape, float("nan"), device=cuda)
    y = T.dwconv_hs_fwd(zc, wc, scc, shc, s, pad, in_act, out_act, apoz, pre)
    torch.testing.assert_close(y.cpu(), y_ref.float(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(pre.cpu(), pre_ref.float(), rtol=1e-4, atol=1e-4)
    assert (apoz.cpu().double() - apoz_ref).abs().max() <= 2  # only outputs within rounding of 0 may differ
    # the same result from the instantiations without APoZ and without pre
    assert torch.equal(T.dwconv_hs_fwd(zc, wc, scc, shc, s, pad, in_act, out_act), y)
    pre2 = torch.empty_like(pre)
    assert torch.equal(T.dwconv_hs_fwd(zc, wc, scc, shc, s, pad, in_act, out_act, None, pre2), y)
    assert torch.equal(pre2, pre)
    assert torch.equal(T.dwconv_hs_fwd(zc, wc, scc, shc, s, pad, in_act, out_act, torch.zeros_like(apoz)), y)
    assert (y[..., C - 4:] == 0).all() and (pre[..., C - 4:] == 0).all() and (apoz[:, C - 4:] == 0).all()

    R = T.dwconv_hs_tay_slots(H, W, C)
    assert R == ops.dwconv_hs_tay_slots(H, W, C) and R >= H
    saved = pre if out_act == 3 else y  # the operand the output's derivative is read from
    saved64 = d(saved.cpu())
    for tay_mode in (0, 1):
        # the reference takes the kernel's own stored output / pre-activation
        tay_ref = torch.zeros(R, B, C, dtype=torch.float64)
        dz_ref = ops.dwconv_hs_dgrad(d(g), saved64, d(w), d(scale), d(z), H, W, s, pad, in_act, out_act, tay_ref,
                                     tay_mode)
        tay = torch.zeros(R, B, C, device=cuda)
        dz = T.dwconv_hs_dgrad(gc, saved, wc, scc, zc, H, W, s, pad, in_act, out_act, tay, tay_mode)
        torch.testing.assert_close(dz.cpu(), dz_ref.float(), rtol=1e-4, atol=1e-4)
        tot, ref = tay.sum(0).cpu().double(), tay_ref.sum(0)
        torch.testing.assert_close(tot, ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))
        if in_act == 3:
            assert (dz.cpu()[z < -3] == 0).all()
        if in_act == 1:
            assert (dz.cpu()[z <= 0] == 0).all()
        assert (dz[..., C - 4:] == 0).all() and (tay[..., C - 4:] == 0).all()
        # bit-identical on a second run, with and without the partials
        tay2 = torch.zeros(R, B, C, device=cuda)
        assert torch.equal(T.dwconv_hs_dgrad(gc, saved, wc, scc, zc, H, W, s, pad, in_act, out_act, tay2, tay_mode), dz)
        assert torch.equal(tay2, tay)
        assert torch.equal(T.dwconv_hs_dgrad(gc, saved, wc, scc, zc, H, W, s, pad, in_act, out_act), dz)


@pytest.mark.parametrize("in_act,out_act", OLD_ACTS)
@pytest.mark.parametrize("shape,ksp", [((3, 7, 9, 32), (3, 1, 1)), ((2, 5, 36, 128), (5, 2, 2)),
                                       ((2, 5, 36, 128), (3, 2, 1)), ((2, 5, 5, 32), (5, 2, 2))])
def test_codes_0_to_2_are_bit_identical_to_dwconv_act(cuda, shape, ksp, in_act, out_act):
    """With and without `pre` (which takes the Hardswish instantiation of the templates)."""
    from torchpruner_amd import ops
    T = ops.require()
    k, s, pad = ksp
    B, H, W, C = shape
    z, w, scale, shift, g = _inputs(shape, k, s, pad, in_act, out_act, 7 + in_act * 3 + out_act)
    z[..., :C - 4] += 3  # populate the ReLU6 regions
    z.view(-1, C)[5::11, :C - 4] = 6.0
    shift[1:C - 4] += 3
    zc, wc, scc, shc, gc = (t.to(cuda) for t in (z, w, scale, shift, g))
    a1, a2, a3 = (torch.zeros(B, C, device=cuda) for _ in range(3))
    y1 = T.dwconv_act_fwd(zc, wc, scc, shc, s, pad, in_act, out_act, a1)
    y2 = T.dwconv_hs_fwd(zc, wc, scc, shc, s, pad, in_act, out_act, a2)
    pre = torch.empty_like(y1)
    y3 = T.dwconv_hs_fwd(zc, wc, scc, shc, s, pad, in_act, out_act, a3, pre)
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(a1, a2) and torch.equal(a1, a3)
    assert torch.equal(pre, T.dwconv_act_fwd(zc, wc, scc, shc, s, pad, in_act, 0))
    if out_act == 2:
        assert (y1 == 0).any() and (y1 == 6).any()
    R = T.dwconv_act_tay_slots(H, W, C)
    for mode in (0, 1):
        t1, t2 = torch.zeros(R, B, C, device=cuda), torch.zeros(R, B, C, device=cuda)
        d1 = T.dwconv_act_dgrad(gc, y1, wc, scc, zc, H, W, s, pad, in_act, out_act, t1, mode)
        d2 = T.dwconv_hs_dgrad(gc, y1, wc, scc, zc, H, W, s, pad, in_act, out_act, t2, mode)
        assert torch.equal(d1, d2) and torch.equal(t1, t2)


@pytest.mark.parametrize("in_act,out_act", [(3, 3), (0, 3), (3, 1)])
def test_dwconv_hs_forward_propagates_nan(cuda, in_act, out_act):
    from torchpruner_amd import ops
    T = ops.require()
    z, w, scale, shift, _ = _inputs((2, 8, 8, 64), 3, 1, 1, in_act, out_act, 5)
    z[1, 3, 4, 9] = float("nan")
    pre_ref = torch.empty(2, 8, 8, 64, dtype=torch.float64)
    ref = ops.dwconv_hs_fwd(z.double(), w.double(), scale.double(), shift.double(), 1, 1, in_act, out_act, None,
                            pre_ref)
    pre = torch.empty(2, 8, 8, 64, device=cuda)
    y = T.dwconv_hs_fwd(z.to(cuda), w.to(cuda), scale.to(cuda), shift.to(cuda), 1, 1, in_act, out_act, None, pre)
    assert torch.isnan(ref).sum() == 9 and torch.isnan(pre_ref).sum() == 9
    torch.testing.assert_close(y.cpu(), ref.float(), rtol=1e-4, atol=1e-4, equal_nan=True)
    torch.testing.assert_close(pre.cpu(), pre_ref.float(), rtol=1e-4, atol=1e-4, equal_nan=True)


def test_dwconv_hs_rejects_bad_arguments(cuda):
    from torchpruner_amd import ops
    T = ops.require()
    z = torch.zeros(1, 4, 4, 8, device=cuda)
    w, v = torch.zeros(8, 1, 3, 3, device=cuda), torch.zeros(8, device=cuda)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        T.dwconv_hs_fwd(torch.zeros(1, 4, 4, 6, device=cuda), torch.zeros(6, 1, 3, 3, device=cuda), v[:6], v[:6], 1, 1,
                        3, 3)
    with pytest.raises(RuntimeError, match="activation codes"):
        T.dwconv_hs_fwd(z, w, v, v, 1, 1, 4, 3)
    with pytest.raises(RuntimeError, match="activation codes"):
        T.dwconv_hs_dgrad(z, z, w, v, z, 4, 4, 1, 1, 3, -1)
    with pytest.raises(RuntimeError, match="activation codes"):  # the ReLU6-only op keeps rejecting Hardswish
        T.dwconv_act_fwd(z, w, v, v, 1, 1, 3, 2)
    with pytest.raises(RuntimeError, match="geometry"):
        T.dwconv_hs_fwd(z, w, v, v, 3, 1, 3, 3)
    with pytest.raises(RuntimeError, match="pre must"):
        T.dwconv_hs_fwd(z, w, v, v, 1, 1, 3, 3, None, torch.zeros(1, 4, 4, 4, device=cuda))
    with pytest.raises(RuntimeError, match="slab"):
        T.dwconv_hs_dgrad(z, z, w, v, z, 4, 4, 1, 1, 3, 3, torch.zeros(3, 1, 8, device=cuda), 0)
    with pytest.raises(RuntimeError, match="tay_mode"):
        T.dwconv_hs_dgrad(z, z, w, v, z, 4, 4, 1, 1, 3, 3, torch.zeros(4, 1, 8, device=cuda), 2)
