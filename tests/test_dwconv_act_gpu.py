"""tpamd.dwconv_act_fwd / dwconv_act_dgrad (csrc/kernels/dwconv_act.hip) against their fp64 PyTorch
references (validated against autograd in test_dwconv_act.py) fed the same fp32 inputs. The masks
are functions of the inputs, so no decision can flip between the two: bounds are arithmetic only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = [(0, 0), (0, 2), (2, 0), (2, 2), (2, 1)]
# (B, H, W, C), (k, stride, pad) lists: odd map with partial strips; a plain one; more than one
# 256-thread slice per row (36 / 4 strips x 32 quads = 288 threads: two slots per row, a ragged last
# slice); stride 2 with pad 2
SHAPES = [((3, 7, 9, 32), [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2)]),
          ((2, 8, 8, 64), [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2)]),
          ((2, 5, 36, 128), [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2)]),
          ((2, 5, 5, 32), [(3, 2, 2), (5, 2, 2)])]
CASES = [(shape, ksp) for shape, lst in SHAPES for ksp in lst]


def _inputs(shape, k, s, pad, in_act, out_act, seed):
    """fp32 inputs with each ReLU6 region holding >= 10 % of z and of the output's pre-activation,
    exact 0.0 / 6.0 planted in both (channel 0 copies the clamped input: centre tap 1, affine
    (1, 0)), and 4 padded channels at the end (zero weights and affine, garbage z)."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, H, W, C, generator=g) * 4 + 3
    w = torch.randn(C, 1, k, k, generator=g) * (1.2 / k)
    scale = torch.rand(C, generator=g) + 1.25  # pre-activation std >= 3.5 around 3: every region populated
    # centre the pre-activation on 3 whatever the input activation and the weights' sum are
    a = z.clamp(0, 6) if in_act else z
    mean = torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), w, None, s, pad, 1, C).mean((0, 2, 3))
    shift = 3.0 - mean * scale + torch.randn(C, generator=g) * 0.5
    w[0].zero_()
    w[0, 0, k // 2, k // 2] = 1.0
    scale[0], shift[0] = 1.0, 0.0
    flat = z.view(-1, C)
    flat[0::7, :] = 0.0
    flat[3::7, :] = 6.0
    w[C - 4:].zero_()
    scale[C - 4:], shift[C - 4:] = 0.0, 0.0
    z[..., C - 4:] = torch.randn(B, H, W, 4, generator=g) * 1e3  # garbage under the padding
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    gr = torch.randn(B, Ho, Wo, C, generator=g)
    return z, w, scale, shift, gr


def _regions(t, lo=0.10):
    n = t.numel()
    return ((t <= 0).sum() >= lo * n) and ((t >= 6).sum() >= lo * n) and (((t > 0) & (t < 6)).sum() >= lo * n)


@pytest.mark.parametrize("in_act,out_act", ACTS)
@pytest.mark.parametrize("shape,ksp", CASES)
def test_dwconv_act_kernels(cuda, shape, ksp, in_act, out_act):
    from torchpruner_amd import ops
    T = ops.require()
    k, s, pad = ksp
    B, H, W, C = shape
    z, w, scale, shift, g = _inputs(shape, k, s, pad, in_act, out_act, 100 * k + 10 * s + in_act * 3 + out_act)
    real = slice(0, C - 4)
    d = lambda t: t.double()
    # fp64 reference on the same fp32 inputs
    apoz_ref = torch.zeros(B, C, dtype=torch.float64)
    y_ref = ops.dwconv_act_fwd(d(z), d(w), d(scale), d(shift), s, pad, in_act, out_act, apoz_ref)
    pre_ref = ops.dwconv_act_fwd(d(z), d(w), d(scale), d(shift), s, pad, in_act, 0)
    assert _regions(z[..., real]) and _regions(pre_ref[..., 1:C - 4]), "a ReLU6 region is under-populated"
    assert (z == 0).any() and (z == 6).any()
    if s == 1 and pad == k // 2:  # channel 0 copies the (clamped) input, planted kinks included
        assert (pre_ref[..., 0] == 0).any() and (pre_ref[..., 0] == 6).any()

    zc, wc, scc, shc, gc = (t.to(cuda) for t in (z, w, scale, shift, g))
    apoz = torch.zeros(B, C, device=cuda)
    y = T.dwconv_act_fwd(zc, wc, scc, shc, s, pad, in_act, out_act, apoz)
    torch.testing.assert_close(y.cpu(), y_ref.float(), rtol=1e-4, atol=1e-4)
    assert (apoz.cpu().double() - apoz_ref).abs().max() <= 2  # only outputs within rounding of 0 may differ
    assert torch.equal(T.dwconv_act_fwd(zc, wc, scc, shc, s, pad, in_act, out_act), y)  # the no-APoZ instantiation
    assert (y[..., C - 4:] == 0).all() and (apoz[:, C - 4:] == 0).all()

    R = T.dwconv_act_tay_slots(H, W, C)
    assert R == ops.dwconv_act_tay_slots(H, W, C) and R >= H
    y32 = y.cpu()
    for tay_mode in (0, 1):
        # the reference takes the kernel's own stored output: the output mask is a function of it
        tay_ref = torch.zeros(R, B, C, dtype=torch.float64)
        dz_ref = ops.dwconv_act_dgrad(d(g), d(y32), d(w), d(scale), d(z), H, W, s, pad, in_act, out_act, tay_ref,
                                      tay_mode)
        tay = torch.zeros(R, B, C, device=cuda)
        dz = T.dwconv_act_dgrad(gc, y, wc, scc, zc, H, W, s, pad, in_act, out_act, tay, tay_mode)
        torch.testing.assert_close(dz.cpu(), dz_ref.float(), rtol=1e-4, atol=1e-4)
        tot, ref = tay.sum(0).cpu().double(), tay_ref.sum(0)
        torch.testing.assert_close(tot, ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))
        if in_act == 2:
            dead = (z <= 0) | (z >= 6)
            assert (dz.cpu()[dead] == 0).all()
        assert (dz[..., C - 4:] == 0).all() and (tay[..., C - 4:] == 0).all()
        # bit-identical on a second run, with and without the partials
        tay2 = torch.zeros(R, B, C, device=cuda)
        assert torch.equal(T.dwconv_act_dgrad(gc, y, wc, scc, zc, H, W, s, pad, in_act, out_act, tay2, tay_mode), dz)
        assert torch.equal(tay2, tay)
        assert torch.equal(T.dwconv_act_dgrad(gc, y, wc, scc, zc, H, W, s, pad, in_act, out_act), dz)


@pytest.mark.parametrize("in_act,out_act", [(2, 2), (0, 0)])
def test_dwconv_act_forward_propagates_nan(cuda, in_act, out_act):
    from torchpruner_amd import ops
    T = ops.require()
    z, w, scale, shift, _ = _inputs((2, 8, 8, 64), 3, 1, 1, in_act, out_act, 5)
    z[1, 3, 4, 9] = float("nan")
    ref = ops.dwconv_act_fwd(z.double(), w.double(), scale.double(), shift.double(), 1, 1, in_act, out_act)
    y = T.dwconv_act_fwd(z.to(cuda), w.to(cuda), scale.to(cuda), shift.to(cuda), 1, 1, in_act, out_act)
    assert torch.isnan(ref).sum() == 9
    torch.testing.assert_close(y.cpu(), ref.float(), rtol=1e-4, atol=1e-4, equal_nan=True)


def test_dwconv_act_rejects_bad_arguments(cuda):
    from torchpruner_amd import ops
    T = ops.require()
    z = torch.zeros(1, 4, 4, 8, device=cuda)
    w, v = torch.zeros(8, 1, 3, 3, device=cuda), torch.zeros(8, device=cuda)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        T.dwconv_act_fwd(torch.zeros(1, 4, 4, 6, device=cuda), torch.zeros(6, 1, 3, 3, device=cuda), v[:6], v[:6], 1, 1,
                         2, 2)
    with pytest.raises(RuntimeError, match="activation codes"):
        T.dwconv_act_fwd(z, w, v, v, 1, 1, 3, 2)
    with pytest.raises(RuntimeError, match="geometry"):
        T.dwconv_act_fwd(z, w, v, v, 3, 1, 2, 2)
    with pytest.raises(RuntimeError, match="slab"):
        T.dwconv_act_dgrad(z, z, w, v, z, 4, 4, 1, 1, 2, 2, torch.zeros(3, 1, 8, device=cuda), 0)
    with pytest.raises(RuntimeError, match="tay_mode"):
        T.dwconv_act_dgrad(z, z, w, v, z, 4, 4, 1, 1, 2, 2, torch.zeros(4, 1, 8, device=cuda), 2)
