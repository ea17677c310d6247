"""The references that tests/test_wgrad_gpu.py holds the conv weight-gradient kernels (conv_wgrad.hip,
wino_wgrad.hip) against, each checked here on the CPU first:

- ``ref_dw64`` / ``mag_dw64``: the weight gradient in fp64 in the kernel's (Cout, Kpad) GEMM layout, and the same on
  the operands' absolute values (the magnitude the rounding-error bounds scale with);
- ``wino_wgrad_emul``: the three steps of wino_wgrad.hip (input / gradient transforms, 16 GEMMs over the tiles, output
  transform) in torch, in any dtype and on absolute values;
- ``combine_emul`` / ``lanes`` / ``eff_splits``: the split combine's summation order and the launcher's choice of
  lanes and splits, as their comments in conv_wgrad.hip state them.

The exact GPU tests rest on one condition, asserted here per shape: with integer operands in [-3, 3] every
intermediate of the direct kernel is an integer below 2^24 and every intermediate of the Winograd path a multiple of
1/4 below 2^22, so fp32 arithmetic in ANY order is exact and the kernels must reproduce the fp64 reference bit for
bit."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24  # unit roundoff of fp32

# (B, H, W, Cin, Cout, ks, stride, pad) of the direct kernel's cases
DIRECT_CASES = [
    (1, 5, 7, 4, 4, 1, 1, 0),       # one slice plus a 3-pixel tail, Kc = 4 of 32
    (3, 7, 9, 36, 132, 1, 1, 0),    # second M tile of 4 rows (cfg 0 and 2)
    (3, 10, 12, 36, 52, 3, 1, 1),   # Kc = 324 in Kpad = 352
    (2, 15, 13, 8, 68, 3, 2, 1),    # odd map, stride 2
    (2, 9, 8, 12, 8, 3, 1, 0),      # padding other than ks // 2
    (2, 9, 8, 12, 8, 3, 1, 2),
    (2, 14, 13, 4, 32, 5, 1, 2),    # 5x5
    (2, 30, 30, 4, 64, 7, 2, 3),    # the stem
    (2, 15, 13, 32, 64, 1, 2, 0),   # non-direct 1x1
    (33, 1, 1, 8, 8, 3, 1, 1),      # only the centre tap is real
]
# (B, H, W, Cin, Cout) of the Winograd cases; the last is the carried-width case (out (44, 50, 3, 3))
WINO_CASES = [(1, 2, 2, 8, 4), (3, 6, 6, 36, 36), (2, 8, 10, 32, 64), (2, 14, 14, 128, 100), (5, 16, 16, 8, 12),
              (3, 10, 8, 64, 64)]
WINO_CARRIED = (3, 10, 8, 64, 64)
WINO_CARRIED_REAL = (44, 50)  # Cout_r, Cin_r


def case_id(c):
    return "x".join(str(v) for v in c)


def out_hw(H, W, ks, stride, pad):
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def kpad_of(ks, Cin):
    return -(-ks * ks * Cin // 32) * 32


def operands(case, kind, seed=0):
    """x (B, H, W, Cin), g (B, Ho, Wo, Cout) fp32 NHWC of a direct case: ``int`` integers in [-3, 3], ``randn`` full
    24-bit mantissas."""
    B, H, W, Cin, Cout, ks, stride, pad = case
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    gen = torch.Generator().manual_seed(1000 * seed + sum(case))
    if kind == "int":
        return (torch.randint(-3, 4, (B, H, W, Cin), generator=gen).float(),
                torch.randint(-3, 4, (B, Ho, Wo, Cout), generator=gen).float())
    return torch.randn(B, H, W, Cin, generator=gen), torch.randn(B, Ho, Wo, Cout, generator=gen)


def ref_dw64(x, g, ks, stride, pad):
    """fp64 weight gradient of the conv as the kernel's (Cout, Kpad) matrix: column k = (kh*ks + kw)*Cin + ci, zero
    pad columns. x (B, H, W, Cin), g (B, Ho, Wo, Cout) NHWC."""
    Cin, Cout = x.shape[3], g.shape[3]
    w = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double(), (Cout, Cin, ks, ks), g.permute(0, 3, 1, 2).double(),
                                    stride=stride, padding=pad)
    out = torch.zeros(Cout, kpad_of(ks, Cin), dtype=torch.float64)
    out[:, :ks * ks * Cin] = w.permute(0, 2, 3, 1).reshape(Cout, -1)
    return out


def mag_dw64(x, g, ks, stride, pad):
    return ref_dw64(x.abs(), g.abs(), ks, stride, pad)


def param_of(dw, Cin, ks):
    """(Cout, Kpad) GEMM layout -> the (Cout, Cin, ks, ks) parameter layout."""
    return dw[:, :ks * ks * Cin].reshape(dw.shape[0], ks, ks, Cin).permute(0, 3, 1, 2)


_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1.]]
_A = [[1, 0], [1, 1], [1, -1], [0, -1.]]
_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1.]]


def wino_wgrad_emul(x, g, dtype, absolute=False):
    """The three steps of wino_wgrad.hip in torch, in ``dtype``: V = B^T d B per 4x4 input patch and dM = A dY A^T
    per 2x2 output-gradient tile, dU[xi] = sum_t dM[xi][t] (x) V[xi][t] (16 GEMMs over the tiles), dW = G^T dU G.
    x (B, H, W, Cin), g (B, H, W, Cout) NHWC -> (Cout, Cin, 3, 3). ``absolute``: every matrix and operand by its
    absolute value (the magnitude that bounds the rounding error of every step)."""
    fix = (lambda t: t.abs()) if absolute else (lambda t: t)
    bt, a, gg = (fix(torch.tensor(m, dtype=dtype)) for m in (_BT, _A, _G))
    Cin, Cout = x.shape[3], g.shape[3]
    xp = F.pad(fix(x.to(dtype)), (0, 0, 1, 1, 1, 1))
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                  # (B, H/2, W/2, Cin, 4, 4)
    V = torch.einsum("ir,bhwcrq,jq->ijbhwc", bt, d, bt).reshape(16, -1, Cin)
    dy = fix(g.to(dtype)).unfold(1, 2, 2).unfold(2, 2, 2)   # (B, H/2, W/2, Cout, 2, 2)
    M = torch.einsum("ia,bhwkac,jc->ijbhwk", a, dy, a).reshape(16, -1, Cout)
    dU = torch.einsum("xtk,xtc->xkc", M, V).reshape(4, 4, Cout, Cin)
    return torch.einsum("ia,ijkc,jb->kcab", gg, dU, gg)


def combine_emul(slabs, SL):
    """The split combine of conv_wgrad.hip (wgrad_combine_par) in fp32, on slabs (S, ...): lane w starts at 0.f and
    adds slabs w, w + SL, ... in increasing order, then lane 0 adds lanes 1 .. SL-1 in order."""
    assert slabs.dtype == torch.float32 and 1 <= SL <= slabs.shape[0]
    lane = []
    for w in range(SL):
        s = torch.zeros_like(slabs[0])
        for q in range(w, slabs.shape[0], SL):
            s = s + slabs[q]
        lane.append(s)
    s = lane[0]
    for i in range(1, SL):
        s = s + lane[i]
    return s


def lanes(n, splits):
    """Lanes per element of the combine over ``splits`` slabs of n elements (the comment in tp_conv_wgrad)."""
    return max(1, min(8, splits, -(-262144 // n)))


def eff_splits(P, splits):
    """(splits that run, 32-pixel slices per split) of a request for ``splits`` over P pixels: no more splits than
    slices, none of them empty."""
    slices = -(-P // 32)
    s = max(1, min(splits, slices))
    per = -(-slices // s)
    return -(-slices // per), per


# ---------------------------------------------------------------------------------------------- the checks
@pytest.mark.parametrize("case", [(2, 5, 4, 4, 4, 3, 2, 1), (1, 4, 5, 4, 8, 2, 1, 0), (2, 3, 3, 8, 4, 1, 2, 0),
                                  (1, 4, 4, 4, 4, 3, 1, 2)], ids=case_id)
def test_ref_dw64_layout(case):
    """ref_dw64 == the definition written as loops: dW[co][(kh*ks + kw)*Cin + ci] = sum g[b, oh, ow, co] *
    x[b, oh*s - p + kh, ow*s - p + kw, ci], zero in the pad columns."""
    B, H, W, Cin, Cout, ks, s, p = case
    x, g = operands(case, "randn")
    Ho, Wo = out_hw(H, W, ks, s, p)
    want = torch.zeros(Cout, kpad_of(ks, Cin), dtype=torch.float64)
    for b in range(B):
        for oh in range(Ho):
            for ow in range(Wo):
                for kh in range(ks):
                    for kw in range(ks):
                        ih, iw = oh * s - p + kh, ow * s - p + kw
                        if 0 <= ih < H and 0 <= iw < W:
                            k0 = (kh * ks + kw) * Cin
                            want[:, k0:k0 + Cin] += torch.outer(g[b, oh, ow].double(), x[b, ih, iw].double())
    got = ref_dw64(x, g, ks, s, p)
    assert got.shape == want.shape
    assert (got[:, ks * ks * Cin:] == 0).all()
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    back = param_of(got, Cin, ks)
    assert back.shape == (Cout, Cin, ks, ks) and back[1, 2, ks - 1, 0] == got[1, ((ks - 1) * ks) * Cin + 2]


@pytest.mark.parametrize("case", WINO_CASES, ids=case_id)
def test_wino_emul_is_the_weight_gradient(case):
    """The fp64 emulation of the three Winograd steps == conv2d_weight (stride 1, pad 1) to 1e-9, and its absolute
    form dominates the direct magnitude (|sum| <= sum of | |)."""
    B, H, W, Cin, Cout = case
    x, g = operands((B, H, W, Cin, Cout, 3, 1, 1), "randn")
    ref = param_of(ref_dw64(x, g, 3, 1, 1), Cin, 3)
    got = wino_wgrad_emul(x, g, torch.float64)
    assert float((got - ref).abs().max()) < 1e-9
    mag = wino_wgrad_emul(x, g, torch.float64, absolute=True)
    assert bool((mag >= ref.abs() - 1e-9).all())
    # and the fp32 run stays under the bound the GPU test uses (S = 1 on the CPU)
    T = B * (H // 2) * (W // 2)
    err = (wino_wgrad_emul(x, g, torch.float32).double() - ref).abs()
    assert bool((err <= (T + 1 + 16) * U24 * mag).all())


def test_combine_emul_order():
    gen = torch.Generator().manual_seed(5)
    slabs = torch.randn(40, 8, 32, generator=gen)
    seq = torch.zeros(8, 32)
    for q in range(40):
        seq = seq + slabs[q]
    assert torch.equal(combine_emul(slabs, 1), seq)
    # 2 lanes written out: (s0 + s2 + ...) + (s1 + s3 + ...)
    even, odd = torch.zeros(8, 32), torch.zeros(8, 32)
    for q in range(0, 40, 2):
        even, odd = even + slabs[q], odd + slabs[q + 1]
    assert torch.equal(combine_emul(slabs, 2), even + odd)
    ref = slabs.double().sum(0)
    mag = slabs.double().abs().sum(0)
    for SL in (1, 2, 3, 4, 6, 8):
        got = combine_emul(slabs, SL)
        assert bool(((got.double() - ref).abs() <= 40 * U24 * mag).all())
    # the order is visible in the bits: this is what the GPU test's comparison can tell apart
    assert not torch.equal(combine_emul(slabs, 8), seq)
    assert not torch.equal(combine_emul(slabs, 4), combine_emul(slabs, 8))
    # a lane with one slab: 0.f + v == v
    assert torch.equal(combine_emul(slabs[:3], 3), (slabs[0] + slabs[1]) + slabs[2])


def test_lanes_and_splits():
    assert lanes(512 * 512, 7) == 1        # the in-order promise: n >= 262144
    assert lanes(262145, 64) == 1 and lanes(262143, 64) == 2
    assert lanes(8 * 32, 40) == 8
    assert lanes(128 * 512, 6) == 4
    assert lanes(96 * 1024, 6) == 3
    assert lanes(16 * 160, 6) == 6
    assert lanes(512 * 4608, 2) == 1
    assert lanes(64, 1) == 1
    for n in (1, 100, 32768, 32769, 131072, 131073, 262144, 10 ** 7):
        for s in range(1, 70):
            assert lanes(n, s) == max(1, min(8, s, math.ceil(262144 / n)))
    assert eff_splits(197, 7) == (7, 1) and eff_splits(1277, 40) == (40, 1) and eff_splits(185, 6) == (6, 1)
    assert eff_splits(384, 6) == (6, 2) and eff_splits(64, 2) == (2, 1) and eff_splits(35, 7) == (2, 1)
    assert eff_splits(390, 7) == (7, 2) and eff_splits(390, 5) == (5, 3) and eff_splits(33, 1) == (1, 2)
    assert eff_splits(5 * 32, 4) == (3, 2)  # 5 slices in 4 splits: 2 per split, so only 3 run


@functools.lru_cache(maxsize=None)
def direct_int_reference(case):
    x, g = operands(case, "int")
    return x, g, ref_dw64(x, g, *case[5:])


# with the grid-stride combine's case and the out= layouts' shape
@pytest.mark.parametrize("case", DIRECT_CASES + [(1, 8, 8, 512, 512, 3, 1, 1), (2, 10, 12, 64, 64, 3, 1, 1)], ids=case_id)
def test_direct_integer_operands_are_exact_in_fp32(case):
    """Integers in [-3, 3]: the magnitude stays below 2^24, so every partial sum of the pixel reduction, in any order
    and any split, is an integer fp32 holds exactly; the fp32 conv2d_weight equals the fp64 one."""
    x, g, ref = direct_int_reference(case)
    B, H, W, Cin, Cout, ks, s, p = case
    assert float(mag_dw64(x, g, ks, s, p).max()) < 2 ** 24
    assert bool((ref == ref.round()).all())
    w32 = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (Cout, Cin, ks, ks), g.permute(0, 3, 1, 2), stride=s,
                                      padding=p)
    assert torch.equal(w32.double(), param_of(ref, Cin, ks))


@functools.lru_cache(maxsize=None)
def wino_int_reference(case):
    B, H, W, Cin, Cout = case
    x, g = operands((B, H, W, Cin, Cout, 3, 1, 1), "int")
    return x, g, param_of(ref_dw64(x, g, 3, 1, 1), Cin, 3).contiguous()


@pytest.mark.parametrize("case", WINO_CASES + [(2, 10, 12, 64, 64)], ids=case_id)  # the last: the out= layouts' shape
def test_wino_integer_operands_are_exact_in_fp32(case):
    """Integers in [-3, 3]: the fp32 emulation equals the fp64 reference exactly and the absolute-value emulation
    stays below 2^22: V, dM and dU are integers, the output transform multiplies by 1/2 twice, so every intermediate
    is a multiple of 1/4 below 2^22 and any order of fp32 operations is exact."""
    x, g, ref = wino_int_reference(case)
    mag = wino_wgrad_emul(x, g, torch.float64, absolute=True)
    print(f"wgrad math wino case={case_id(case)} max_magnitude={float(mag.max()):.0f}")
    assert float(mag.max()) < 2 ** 22
    assert bool((ref * 4 == (ref * 4).round()).all())
    assert torch.equal(wino_wgrad_emul(x, g, torch.float32).double(), ref)
    assert torch.equal(wino_wgrad_emul(x, g, torch.float64), ref)
