"""tpamd.dwconv_silu_fwd / dwconv_silu_dgrad (csrc/kernels/dwconv_silu.hip) against their fp64 PyTorch
bodies (validated against autograd in test_dwconv_silu.py) on the same fp32 inputs. SiLU is smooth: no
branch can flip between the two, so the bounds are arithmetic only (those of test_dwconv_hs_gpu.py).

Shapes: C no multiple of the 32-channel slice, W wider than one column band, odd H; a stride-2 map with
pad 2; a map smaller than the kernel; (1, 19, 8, 32): five row bands of the finest split; and the
tile's remaining boundary, (32, 19, 2, 2048): 512 blocks before the row split, so the rows are cut into
two bands of 10 and 9 only and the LDS ring (6 rows for 5x5 stride 1) wraps inside a band. EDGE_SHAPES:
the band-arithmetic edges of test_dwconv_silu_edges_gpu.py (which asserts their splits and checks them
bit for bit on integer inputs), here under the real SiLU arithmetic."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KS4 = [(3, 1, 1), (3, 2, 1), (5, 1, 2), (5, 2, 2)]
SHAPES = [((3, 7, 9, 40), KS4), ((2, 5, 36, 72), KS4), ((2, 5, 5, 32), [(3, 2, 2), (5, 2, 2)]),
          ((2, 1, 1, 36), [(3, 1, 1), (5, 1, 2)]), ((1, 19, 8, 32), [(5, 1, 2), (3, 2, 1)]),
          ((32, 19, 2, 2048), [(5, 1, 2), (3, 2, 1)])]
EDGE_SHAPES = [((1, 8, 33, 8), KS4), ((1, 6, 66, 8), [(3, 2, 1), (5, 2, 2), (3, 1, 1)]),
               ((1, 4, 65, 8), [(5, 1, 2), (3, 1, 1)]), ((1, 21, 3, 8), KS4),
               ((2, 12, 12, 8), [(3, 2, 1), (5, 2, 2), (3, 2, 0), (5, 1, 4), (3, 1, 0)]),
               ((1, 9, 14, 8), [(3, 2, 1), (5, 2, 2), (5, 1, 2)]), ((300, 19, 4, 8), [(5, 1, 2), (3, 2, 1)]),
               ((2, 10, 16, 136), [(3, 1, 1), (5, 2, 2)])]
CASES = [(shape, ksp) for shape, lst in SHAPES + EDGE_SHAPES for ksp in lst]


def _inputs(shape, k, s, pad, in_act, seed):
    """fp32 inputs as test_dwconv_hs_gpu.py::_inputs builds them, without the planted kinks: z ~ N(0, 4^2),
    weights and affine that centre the pre-activation on 0 with std >= 3.5, 4 padded channels at the
    end (zero weights and affine, 1e3-scale garbage z)."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, H, W, C, generator=g) * 4
    w = torch.randn(C, 1, k, k, generator=g) * (1.2 / k)
    scale = torch.rand(C, generator=g) + 1.75
    a = torch.nn.functional.silu(z) if in_act else z
    mean = torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), w, None, s, pad, 1, C).mean((0, 2, 3))
    shift = -mean * scale + torch.randn(C, generator=g) * 0.5
    w[C - 4:].zero_()
    scale[C - 4:], shift[C - 4:] = 0.0, 0.0
    z[..., C - 4:] = torch.randn(B, H, W, 4, generator=g) * 1e3
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    return z, w, scale, shift, torch.randn(B, Ho, Wo, C, generator=g)


def _worst(got, ref, rtol, atol):
    """max of |got - ref| / (atol + rtol |ref|): <= 1 is assert_close's test"""
    return float(((got.double() - ref).abs() / (atol + rtol * ref.abs())).max())


@pytest.mark.parametrize("in_act", [0, 4])
@pytest.mark.parametrize("shape,ksp", CASES)
def test_dwconv_silu_kernels(cuda, shape, ksp, in_act):
    from torchpruner_amd import ops
    T = ops.require()
    (k, s, pad), (B, H, W, C) = ksp, shape
    z, w, scale, shift, g = _inputs(shape, k, s, pad, in_act, 100 * k + 10 * s + in_act)
    d = lambda t: t.double()
    Ho, Wo = g.shape[1:3]
    Rp, R = T.dwconv_silu_pool_slots(Ho, Wo, C), T.dwconv_silu_tay_slots(H, W, C)
    assert Rp == ops.dwconv_silu_pool_slots(Ho, Wo, C) >= 1 and R == ops.dwconv_silu_tay_slots(H, W, C) >= 1
    apoz_ref, pre_ref = torch.zeros(B, C, dtype=torch.float64), torch.empty(B, Ho, Wo, C, dtype=torch.float64)
    y_ref = ops.dwconv_silu_fwd(d(z), d(w), d(scale), d(shift), s, pad, in_act, 4, apoz_ref, pre_ref)

    zc, wc, scc, shc, gc = (t.to(cuda) for t in (z, w, scale, shift, g))
    fwd = lambda *opt: T.dwconv_silu_fwd(zc, wc, scc, shc, s, pad, in_act, 4, *opt)
    apoz, pre, pool = torch.zeros(B, C, device=cuda), torch.full(y_ref.shape, float("nan"), device=cuda), \
        torch.zeros(Rp, B, C, device=cuda)
    y = fwd(apoz, pre, pool)
    sums, sums_ref = pool.sum(0).cpu().double(), y_ref.sum((1, 2))
    worst = {"y": _worst(y.cpu(), y_ref, 1e-4, 1e-4), "pre": _worst(pre.cpu(), pre_ref, 1e-4, 1e-4),
             "pool": _worst(sums, sums_ref, 0.0, 1e-4 * float(sums_ref.abs().max())),
             "apoz": float((apoz.cpu().double() - apoz_ref).abs().max()) / 2}
    # the same bits without the optional outputs, and on a second run
    pre2, pool2 = torch.empty_like(pre), torch.zeros_like(pool)
    assert torch.equal(fwd(), y) and torch.equal(fwd(None, pre2), y) and torch.equal(pre2, pre)
    assert torch.equal(fwd(torch.zeros_like(apoz), None, pool2), y) and torch.equal(pool2, pool)
    pad_c = slice(C - 4, C)
    assert (y[..., pad_c] == 0).all() and (pre[..., pad_c] == 0).all() and (apoz[:, pad_c] == 0).all()
    assert (pool[..., pad_c] == 0).all()

    pre64 = d(pre.cpu())  # the reference takes the kernel's own stored pre-activation
    for mode in (0, 1):
        tay_ref = torch.zeros(R, B, C, dtype=torch.float64)
        dz_ref = ops.dwconv_silu_dgrad(d(g), pre64, d(w), d(scale), d(z), H, W, s, pad, in_act, 4, tay_ref, mode)
        tay = torch.zeros(R, B, C, device=cuda)
        dz = T.dwconv_silu_dgrad(gc, pre, wc, scc, zc, H, W, s, pad, in_act, 4, tay, mode)
        tot, ref = tay.sum(0).cpu().double(), tay_ref.sum(0)
        worst[f"dz{mode}"] = _worst(dz.cpu(), dz_ref, 1e-4, 1e-4)
        worst[f"tay{mode}"] = _worst(tot, ref, 0.0, 1e-4 * float(ref.abs().max()))
        assert (dz[..., pad_c] == 0).all() and (tay[..., pad_c] == 0).all()
        tay2 = torch.zeros_like(tay)
        assert torch.equal(T.dwconv_silu_dgrad(gc, pre, wc, scc, zc, H, W, s, pad, in_act, 4, tay2, mode), dz)
        assert torch.equal(tay2, tay)
        assert torch.equal(T.dwconv_silu_dgrad(gc, pre, wc, scc, zc, H, W, s, pad, in_act, 4), dz)
    print(f"dwconv_silu {shape} k{k} s{s} p{pad} in_act {in_act}: worst error / bound " +
          " ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst

    # z = +-100 and a NaN in one channel: finite / NaN exactly where the reference has them
    z[0, 0, 0, 0], z[0, H - 1, W - 1, 1], z[B - 1, H // 2, W // 2, 2] = 100.0, -100.0, float("nan")
    pre_ref = torch.empty_like(pre_ref)
    y_ref = ops.dwconv_silu_fwd(d(z), d(w), d(scale), d(shift), s, pad, in_act, 4, None, pre_ref)
    zc = z.to(cuda)
    y = T.dwconv_silu_fwd(zc, wc, scc, shc, s, pad, in_act, 4, None, pre)
    dz = T.dwconv_silu_dgrad(gc, pre, wc, scc, zc, H, W, s, pad, in_act, 4)
    dz_ref = ops.dwconv_silu_dgrad(d(g), d(pre.cpu()), d(w), d(scale), d(z), H, W, s, pad, in_act, 4)
    assert torch.isnan(y_ref).any() and not torch.isnan(y_ref[..., 0]).any()
    for got, ref in ((y, y_ref), (pre, pre_ref), (dz, dz_ref)):
        assert torch.equal(torch.isnan(got.cpu()), torch.isnan(ref)) and not torch.isinf(got).any()
        torch.testing.assert_close(got.cpu(), ref.float(), rtol=1e-4, atol=1e-4, equal_nan=True)


def test_dwconv_silu_rejects_bad_arguments(cuda):
    from torchpruner_amd import ops
    T = ops.require()
    z, w, v = torch.zeros(1, 4, 4, 8, device=cuda), torch.zeros(8, 1, 3, 3, device=cuda), torch.zeros(8, device=cuda)
    for codes in [(3, 4), (4, 3), (4, 0), (-1, 4)]:
        with pytest.raises(RuntimeError, match="activation codes"):
            T.dwconv_silu_fwd(z, w, v, v, 1, 1, *codes)
        with pytest.raises(RuntimeError, match="activation codes"):
            T.dwconv_silu_dgrad(z, z, w, v, z, 4, 4, 1, 1, *codes)
    assert T.dwconv_silu_tay_slots(0, 7, 8) == 0 and T.dwconv_silu_pool_slots(7, 7, 6) == 0  # rejected shapes: 0 slots
    with pytest.raises(RuntimeError, match="geometry"):
        T.dwconv_silu_fwd(z, w, v, v, 3, 1, 4, 4)
    with pytest.raises(RuntimeError, match="slab"):
        T.dwconv_silu_fwd(z, w, v, v, 1, 1, 4, 4, None, None, torch.zeros(2, 1, 8, device=cuda))
    with pytest.raises(RuntimeError, match="slab"):
        T.dwconv_silu_dgrad(z, z, w, v, z, 4, 4, 1, 1, 4, 4, torch.zeros(3, 1, 8, device=cuda), 0)
    with pytest.raises(RuntimeError, match="tay_mode"):
        T.dwconv_silu_dgrad(z, z, w, v, z, 4, 4, 1, 1, 4, 4, torch.zeros(1, 1, 8, device=cuda), 2)
    with pytest.raises(RuntimeError, match="16-byte|multiple of 4"):
        T.dwconv_silu_fwd(z[..., :6].contiguous(), w[:6], v[:6], v[:6], 1, 1, 4, 4)
