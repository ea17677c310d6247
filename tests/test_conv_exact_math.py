"""Operand generators, fp64 references and case tables that tests/test_conv_exact_gpu.py holds the forward and
data-gradient convs against (conv_mfma.hip: the stride-1 implicit GEMM and the GEN kernels; winograd.hip: F(2x2);
wino4.hip: F(4x4)), each checked here on the CPU first.

The exact GPU tests rest on one condition, asserted here for every case of the tables:

- implicit GEMM / GEN: x, g, w are integers in [-3, 3], so every product and every partial sum of an output element,
  in any order and for any K split, is an integer bounded by the same conv on the absolute values; that bound stays
  below 2^24 (the largest is asserted to be <= 9 * 96 * 9 = 7776), so fp32 holds every intermediate exactly;
- F(2x2): the weights are multiples of 4 in [-8, 8], so U = G w G^T (entries of G: 0, +-1, +-1/2) is an integer, and
  so are V = B^T d B, the per-point channel sums and A^T m A; the emulation on absolute values bounds every partial
  sum and stays below 2^24 (asserted < 2.5e5), and the fp32 emulation equals the fp64 one;
- the epilogue operands (scale in {0.5, 1, 2}, integer shift / res, slope 0.25, act in [0, 3]) keep every value a
  multiple of 1/8 far below 2^20, and the Taylor sums are bounded by sum |dx| * act < 2^24: the reference survives a
  round trip through float32 unchanged.

Together: "the kernel equals fp64 bit for bit" is a theorem about a correct kernel, not a hope. One dropped,
duplicated or misplaced term changes an integer-valued output by at least 1 (every non-zero operand has magnitude
>= 1), so no tolerance is needed and none is given.

Pool argmax: the expected byte (dy * 2 + dx of the window maximum) is defined where the maximum is unique. Measured
here from the references alone: over the pooled cases the share of windows with a unique positive maximum is between
0.91 and 0.94 (the assertion asks for >= 0.5), so the argmax comparison is never vacuous.

F(4x4) cannot be exact: G holds 1/6, 1/12 and 1/24, so even a 1x1-support integer weight (only the centre tap
non-zero) gives U = w * g_i1 * g_j1 with factors 1/6 and 1/12 that fp32 rounds. ``wino4_bound`` is the first-order
bound the GPU test holds every element to instead; its rounding count is written out at its definition."""
import functools

import pytest
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24  # unit roundoff of fp32
CFGS = [0, 1, 2, 3, 4, 5, 6]


def case_id(c):
    return "x".join(str(v) for v in c)


# ------------------------------------------------------------------------------------------ operand generators
def gen_of(tag, key):
    """A CPU generator seeded by the case alone (no hash(): the same operands in every process)."""
    return torch.Generator().manual_seed(100003 * tag + sum((i + 1) * int(v) for i, v in enumerate(key)))


def ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()


def act_ints(shape, gen):
    """The ReLU mask / Taylor operand: integers in [0, 3], a third of them zero."""
    r = torch.randint(0, 9, tuple(shape), generator=gen)
    return torch.tensor([0., 0., 0., 1., 1., 2., 2., 3., 3.])[r]


def scales(n, gen):
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=gen)]


def wino2_weights_int(shape, gen):
    """Multiples of 4 in [-8, 8]: G w G^T is an integer."""
    return 4.0 * torch.randint(-2, 3, tuple(shape), generator=gen).float()


def argmax_bytes(shape, gen):
    return torch.randint(0, 4, tuple(shape), generator=gen, dtype=torch.uint8)


SLOPE = 0.25


# ------------------------------------------------------------------------------------------------- references
def ref_conv(x, w, stride=1, pad=None):
    """fp64 conv of NHWC x with w (Cout, Cin, ks, ks) -> NHWC."""
    pad = w.shape[-1] // 2 if pad is None else pad
    return F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=stride, padding=pad).permute(0, 2, 3, 1)


def ref_fwd(x, w, scale=None, shift=None, res=None, relu=False, slope=0.0, stride=1, pad=None):
    """acc * scale + shift, then + res, then ReLU / LeakyReLU (the order of the kernels' epilogues)."""
    y = ref_conv(x, w, stride, pad)
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if res is not None:
        y = y + res.double()
    if relu:
        y = torch.where(y > 0, y, y * slope)
    return y


def ref_pool(y):
    """2x2 max-pool of NHWC y: (pooled, argmax byte dy * 2 + dx, mask of windows whose maximum is unique and
    positive: only there the byte is defined and compared)."""
    B, H, W, C = y.shape
    win = y.unfold(1, 2, 2).unfold(2, 2, 2).reshape(B, H // 2, W // 2, C, 4)  # window order (dy, dx)
    best = win.max(-1).values
    hit = win == best.unsqueeze(-1)
    arg = hit.float().argmax(-1).to(torch.uint8)
    return best, arg, (hit.sum(-1) == 1) & (best > 0)


def ref_apoz(y):
    return (y > 0).sum((1, 2)).double()


def ref_dgrad(g, wf, in_hw, stride=1, pad=None):
    """fp64 dL/dx (NHWC) of y = conv2d(x, wf), wf (C, N, ks, ks) mapping N -> C channels, for NHWC g (B, H, W, C)."""
    pad = wf.shape[-1] // 2 if pad is None else pad
    dx = torch.nn.grad.conv2d_input((g.shape[0], wf.shape[1]) + tuple(in_hw), wf.double(),
                                    g.permute(0, 3, 1, 2).double(), stride=stride, padding=pad)
    return dx.permute(0, 2, 3, 1)


def ref_bwd_out(dx, act, bn_scale, slope=0.0):
    """The dgrad epilogue's output: dx * bn_scale where act > 0, times slope elsewhere."""
    v = dx * bn_scale.double()
    return torch.where(act.double() > 0, v, v * slope)


def ref_taylor(dx, act, mode):
    """Per (image, channel): mode 0 -(dx * act), 1 |dx|, 2 |dx| where act > 0, summed over the pixels."""
    a = act.double()
    t = {0: -(dx * a), 1: dx.abs(), 2: torch.where(a > 0, dx.abs(), torch.zeros((), dtype=torch.float64))}[mode]
    return t.sum((1, 2))


def unpool(gp, am):
    """The full-resolution gradient a pooled gradient and its argmax bytes imply: gp at position (byte >> 1, byte & 1)
    of each 2x2 window, zero at the other three."""
    B, H, W, C = gp.shape
    out = torch.zeros(B, 2 * H, 2 * W, C, dtype=gp.dtype)
    for q in range(4):
        out[:, q // 2::2, q % 2::2, :] = torch.where(am == q, gp, torch.zeros((), dtype=gp.dtype))
    return out


def res_scatter(res, Ho, Wo, s):
    """A (B, ceil(Ho/s), ceil(Wo/s), N) residual added at the pixels with oh % s == 0 and ow % s == 0."""
    full = torch.zeros(res.shape[0], Ho, Wo, res.shape[3], dtype=torch.float64)
    full[:, ::s, ::s] = res.double()
    return full


def survives_fp32(t):
    return torch.equal(t.float().double(), t)


# -------------------------------------------------------------------------------- GEMM layouts of the bindings
def ceil32(n):
    return -(-n // 32) * 32


def igemm_w(w):
    """conv_fwd's operand: (Cout, ks*ks*Cin), column (kh, kw, ci)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def igemm_wt(wf):
    """conv_dgrad's operand of the forward weight wf (C, N, ks, ks): (N, ks*ks*C) with flipped taps."""
    return wf.flip(2, 3).permute(1, 2, 3, 0).reshape(wf.shape[1], -1).contiguous()


def gen_w(w, fill):
    """conv_gen's operand (Cout, conv_gen_k(ks, Cin)): every tap's channels padded to 32 (a 4-channel input: the
    packed taps padded once at the end); the padding columns hold ``fill``."""
    Cout, Cin, ks, _ = w.shape
    wk = w.permute(0, 2, 3, 1)
    if Cin == 4:
        wk = wk.reshape(Cout, -1)
        return F.pad(wk, (0, ceil32(wk.shape[1]) - wk.shape[1]), value=fill).contiguous()
    return F.pad(wk, (0, ceil32(Cin) - Cin), value=fill).reshape(Cout, -1).contiguous()


def gen_wt(wf, transposed, fill):
    """conv_gen_bwd's operand of the forward weight wf (C, N, ks, ks): (N, ks*ks*ceil32(C)), column (kh, kw, co);
    natural taps for the transposed (strided) data gradient, flipped taps for the stride-1 one."""
    C, N, ks, _ = wf.shape
    wk = (wf if transposed else wf.flip(2, 3)).permute(1, 2, 3, 0)
    return F.pad(wk, (0, ceil32(C) - C), value=fill).reshape(N, -1).contiguous()


# ------------------------------------------------------------------------------------------- Winograd matrices
_BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1.]]
_AT2 = [[1, 1, 1, 0], [0, 1, -1, -1.]]
_G2 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1.]]
_BT4 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
        [0, 4, 0, -5, 0, 1.]]
_AT4 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1.]]
_G4 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
       [1 / 24, -1 / 12, 1 / 6], [0, 0, 1.]]


def wino_emul(x, w, m, dtype=torch.float64, absolute=False):
    """F(m x m, 3x3) in torch, m = 2 or 4, as winograd.hip / wino4.hip arrange it: U = G w G^T, V = B^T d B per
    (m + 2)^2 input patch (zero halo, a partial last tile padded with zeros), M = sum_c U (.) V per transform point,
    Y = A^T M A. x (B, H, W, C) NHWC, w (K, C, 3, 3) -> (Y (B, H, W, K), {stage: largest magnitude}).
    ``absolute``: every matrix and operand by its absolute value (the magnitude that bounds every partial sum and
    the rounding error of every step)."""
    fix = (lambda t: t.abs()) if absolute else (lambda t: t)
    bt, at, gg = (fix(torch.tensor(t, dtype=dtype)) for t in ((_BT2, _AT2, _G2) if m == 2 else (_BT4, _AT4, _G4)))
    B, H, W, C = x.shape
    Hp, Wp = -(-H // m) * m, -(-W // m) * m
    xp = F.pad(fix(x.to(dtype)), (0, 0, 1, 1 + Wp - W, 1, 1 + Hp - H))
    d = xp.unfold(1, m + 2, m).unfold(2, m + 2, m)            # (B, th, tw, C, m+2, m+2)
    U = torch.einsum("ia,kcab,jb->kcij", gg, fix(w.to(dtype)), gg)
    V = torch.einsum("ir,bhwcrq,jq->bhwcij", bt, d, bt)
    M = torch.einsum("kcij,bhwcij->bhwkij", U, V)
    Y = torch.einsum("ai,bhwkij,cj->bhwkac", at, M, at)       # (B, th, tw, K, m, m)
    K = w.shape[0]
    y = Y.permute(0, 1, 4, 2, 5, 3).reshape(B, Hp, Wp, K)[:, :H, :W]
    return y, {"U": float(U.abs().max()), "V": float(V.abs().max()), "M": float(M.abs().max()),
               "Y": float(Y.abs().max()), "U_obj": U, "V_obj": V, "M_obj": M}


# Roundings on any path from an operand pair to an output element of wino4.hip, one K pass, counted from its code:
#   1      U = G w G^T: formed in fp64 by weight_transform_one and rounded to fp32 once;
#   4      V = B^T d B: two bt6 passes, each at most a rounded difference / sum feeding one fmaf (depth 2);
#   1 + C  the channel sum on the MFMA: a product and one accumulation per term;
#   6      Y = A^T m A: two at6 passes of depth 3 (y0 = (m0 + a) + c; y3 = fmaf(8, d, b) + m5);
#   1      the split-points variant adds its two half-grid partial outputs;
#   2      the affine (acc * scale, + shift); the dgrad epilogue's single product by bn_scale is covered by it.
# 15 + C in all (the issue's estimate of 40 counted the 6 + 6 and 3 + 3 TERMS of the transforms, not the depth of the
# operations that sum them). Second order included: n u / (1 - n u).
WINO4_DEPTH = 15


def gamma(n):
    return n * U24 / (1.0 - n * U24)


def wino4_bound(x, w, scale=None, shift=None):
    """E (B, S, S, K): |fp32 F(4x4) - exact| <= E per element, from absolute values in fp64:
    gamma(C + 15) * (|A^T| (sum_c (|G| |w| |G^T|) (.) (|B^T| |d| |B|)) |A| * |scale| + |shift|)."""
    mag, _ = wino_emul(x, w, 4, torch.float64, absolute=True)
    if scale is not None:
        mag = mag * scale.double().abs()
    if shift is not None:
        mag = mag + shift.double().abs()
    return gamma(x.shape[3] + WINO4_DEPTH) * mag


def taylor_bound(E, dx, act, mode):
    """Bound of the fp32 partial sums of ref_taylor given the per-element bound E of dx: the terms' own error
    (E * act, or E for |dx|), one rounding of each product and one per addition of the npix-term sum (in any order,
    over any number of slots, folded here in fp64)."""
    a = act.double()
    zero = torch.zeros((), dtype=torch.float64)
    term = {0: dx.abs() * a, 1: dx.abs(), 2: torch.where(a > 0, dx.abs(), zero)}[mode]
    eterm = {0: E * a, 1: E, 2: torch.where(a > 0, E, zero)}[mode]
    npix = dx.shape[1] * dx.shape[2]
    return eterm.sum((1, 2)) + gamma(npix + 1) * (term + eterm).sum((1, 2))


# ------------------------------------------------------------------------------------------------ case tables
# (B, H, W, Cin, Cout) of the stride-1 implicit GEMM (3x3); the data gradient reads g with Cin channels (a multiple
# of 32, the GEMM's K side) and writes Cout channels (the N side), so both directions meet the same partial tiles
IGEMM_SHAPES = [
    (3, 6, 10, 32, 96),    # M = 180: a partial last M tile for every cfg; N partial for BN = 128 and 64
    (1, 2, 2, 32, 32),     # M = 4: one pooling window
    (5, 4, 4, 96, 36),     # three K slices per tap; N no multiple of 32
    (2, 16, 16, 32, 64),   # M = 512 crosses the 256-row tile with two images
    (7, 2, 2, 64, 132),    # N one quad past a 128 tile
]
LINEAR_SHAPES = [(37, 64, 12), (3, 96, 132)]  # ks = 1 as a linear layer: (B, K, N)
IGEMM_SPLITS = [1, 2, 4, 1000]  # 1000: above every K slice count (clamped by the launcher)

# conv_gen forward: (H, W, Cin, Cout, ks, stride, pad), B = 3
GEN_FWD_CASES = [
    (9, 7, 32, 36, 1, 1, 0),
    (9, 7, 36, 64, 1, 2, 0),      # pruned width: Cin = 36 in a 64-column tap
    (9, 7, 32, 132, 3, 1, 1),
    (15, 13, 40, 36, 3, 2, 1),    # odd map: the last stride-2 window is partial; pruned width
    (9, 7, 8, 4, 3, 1, 0),        # pad 0
    (9, 7, 32, 64, 3, 1, 2),      # pad 2
    (15, 13, 8, 36, 5, 1, 2),     # 5x5
    (15, 13, 4, 64, 7, 2, 3),     # the packed 4-channel path: the stem
    (9, 7, 4, 132, 3, 1, 1),      # ... and 3x3
]
# conv_gen_bwd: (in_h, in_w, C (gradient channels), N (output channels), ks, stride, transposed), B = 3, pad ks // 2
GEN_BWD_CASES = [
    (20, 18, 32, 64, 3, 2, True),   # even sizes: the parity row order; 90 pixels per phase: partials on the 256 tiles
    (15, 13, 64, 36, 3, 2, True),   # odd sizes
    (14, 10, 64, 32, 1, 2, True),
    (9, 7, 40, 132, 1, 2, True),    # pruned gradient width
    (12, 8, 32, 36, 1, 1, False),   # 96 pixels per image: a 256-row tile spans three images (partials allowed)
    (10, 6, 40, 64, 3, 1, False),   # flipped 3x3
]
# F(2x2): (B, H, W, Cin, Cout); the first three are odd maps (direct loads, no pooling)
WINO2_ODD = [(3, 7, 7, 64, 64), (2, 5, 9, 32, 32), (2, 1, 5, 32, 32)]
WINO2_EVEN = [
    (2, 8, 8, 32, 64),     # four images per staged block: half a block
    (3, 4, 4, 64, 32),     # sixteen images per block
    (5, 8, 8, 32, 32),     # images kind: one full block and a quarter of one
    (2, 16, 32, 32, 32),   # rows kind (W/2 = 16 | 64): four tile rows per block, blocks never partial there
    (3, 14, 14, 32, 32),   # W/2 = 7: the row-span staged input, blocks straddling images, partial last block
]
# F(4x4): (S, C, K, B, ko) = tests/test_wino4_epilogue_gpu.py's SHAPES and BAND
WINO4_SHAPES = [(32, 8, 32, 1, 0), (32, 16, 64, 2, 0), (16, 8, 64, 3, 0), (8, 16, 32, 5, 0), (4, 8, 32, 33, 0),
                (16, 8, 64, 3, 36), (16, 8, 64, 3, 60)]
WINO4_BAND = (7, 8, 32, 3, 0)


@functools.lru_cache(maxsize=None)
def igemm_fwd_case(shape, ks=3):
    """Operands and the fp64 pre-activation parts of a stride-1 forward case (shared by every cfg / split)."""
    B, H, W, Cin, Cout = shape
    gen = gen_of(1, shape + (ks,))
    x = ints((B, H, W, Cin), -3, 3, gen)
    w = ints((Cout, Cin, ks, ks), -3, 3, gen)
    return x, w, scales(Cout, gen), ints((Cout,), -4, 4, gen)


@functools.lru_cache(maxsize=None)
def igemm_bwd_case(shape, ks=3):
    """g (B, H, W, Cin), pooled gp + argmax bytes (even maps), wf (Cin, Cout, ks, ks), act, bn_scale."""
    B, H, W, Cin, Cout = shape
    gen = gen_of(2, shape + (ks,))
    g = ints((B, H, W, Cin), -3, 3, gen)
    wf = ints((Cin, Cout, ks, ks), -3, 3, gen)
    act = act_ints((B, H, W, Cout), gen)
    sc = scales(Cout, gen)
    gp = am = None
    if H % 2 == 0 and W % 2 == 0:
        gp = ints((B, H // 2, W // 2, Cin), -3, 3, gen)
        am = argmax_bytes((B, H // 2, W // 2, Cin), gen)
    return g, wf, act, sc, gp, am


@functools.lru_cache(maxsize=None)
def wino2_fwd_case(shape):
    B, H, W, Cin, Cout = shape
    gen = gen_of(3, shape)
    x = ints((B, H, W, Cin), -3, 3, gen)
    w = wino2_weights_int((Cout, Cin, 3, 3), gen)
    return x, w, scales(Cout, gen), ints((Cout,), -4, 4, gen)


@functools.lru_cache(maxsize=None)
def wino2_bwd_case(shape):
    """The data gradient of a conv Cout -> Cin of the shape's names: g has Cin channels, the output Cout."""
    B, H, W, Cin, Cout = shape
    gen = gen_of(4, shape)
    g = ints((B, H, W, Cin), -3, 3, gen)
    wf = wino2_weights_int((Cin, Cout, 3, 3), gen)
    act = act_ints((B, H, W, Cout), gen)
    sc = scales(Cout, gen)
    gp = am = None
    if H % 2 == 0 and W % 2 == 0:
        gp = ints((B, H // 2, W // 2, Cin), -3, 3, gen)
        am = argmax_bytes((B, H // 2, W // 2, Cin), gen)
    return g, wf, act, sc, gp, am


@functools.lru_cache(maxsize=None)
def gen_fwd_case(case):
    H, W, Cin, Cout, ks, stride, pad = case
    gen = gen_of(5, case)
    x = ints((3, H, W, Cin), -3, 3, gen)
    w = ints((Cout, Cin, ks, ks), -3, 3, gen)
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    return x, w, scales(Cout, gen), ints((Cout,), -4, 4, gen), ints((3, Ho, Wo, Cout), -8, 8, gen)


@functools.lru_cache(maxsize=None)
def gen_bwd_case(case):
    """g at the forward conv's output size, wf (C, N, ks, ks), the two residuals (dense, stride-2) and the mask."""
    ih, iw, C, N, ks, stride, transposed = case
    pad = ks // 2
    gen = gen_of(6, case[:6] + (int(transposed),))
    H, W = (ih + 2 * pad - ks) // stride + 1, (iw + 2 * pad - ks) // stride + 1
    g = ints((3, H, W, C), -3, 3, gen)
    wf = ints((C, N, ks, ks), -3, 3, gen)
    res1 = ints((3, ih, iw, N), -8, 8, gen)
    res2 = ints((3, -(-ih // 2), -(-iw // 2), N), -8, 8, gen)
    mask = act_ints((3, ih, iw, N), gen)
    return g, wf, res1, res2, mask


@functools.lru_cache(maxsize=None)
def wino4_fwd_case(shape):
    """Randn operands (full 24-bit mantissas) of an F(4x4) forward case, the fp64 output and its bound E."""
    S, C, K, B, ko = shape
    kw = ko or K
    gen = gen_of(7, shape)
    x = torch.randn(B, S, S, C, generator=gen)
    w = torch.randn(kw, C, 3, 3, generator=gen) / (3 * C ** 0.5)
    sc = torch.rand(kw, generator=gen) + 0.5
    sh = torch.randn(kw, generator=gen) * 0.1
    return x, w, sc, sh, ref_fwd(x, w, sc, sh), wino4_bound(x, w, sc, sh)


@functools.lru_cache(maxsize=None)
def wino4_bwd_case(shape):
    """The data gradient of a conv kw -> C: g (B, S, S, C), wf (C, kw, 3, 3), act, bn_scale, unpool bytes; the fp64
    dx and its bound (before bn_scale)."""
    S, C, K, B, ko = shape
    kw = ko or K
    gen = gen_of(8, shape)
    wf = torch.randn(C, kw, 3, 3, generator=gen) / (3 * kw ** 0.5)
    g = torch.randn(B, S, S, C, generator=gen)
    act = torch.relu(torch.randn(B, S, S, kw, generator=gen))
    sc = torch.rand(kw, generator=gen) + 0.5
    am = argmax_bytes((B, S, S, kw), gen)
    dx = ref_dgrad(g, wf, (S, S))
    E = wino4_bound(g, wf.flip(2, 3).transpose(0, 1), None, None)
    return g, wf, act, sc, am, dx, E


# ------------------------------------------------------------------------------------------------- the checks
def test_generators():
    gen = gen_of(0, (1, 2, 3))
    a = act_ints((4000,), gen)
    assert set(a.tolist()) == {0.0, 1.0, 2.0, 3.0} and 0.28 < float((a == 0).float().mean()) < 0.39
    assert set(scales(300, gen).tolist()) == {0.5, 1.0, 2.0}
    w = wino2_weights_int((500,), gen)
    assert set(w.tolist()) == {-8.0, -4.0, 0.0, 4.0, 8.0}
    x = ints((2000,), -3, 3, gen)
    assert set(x.tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert torch.equal(ints((5,), -3, 3, gen_of(1, (4, 5))), ints((5,), -3, 3, gen_of(1, (4, 5))))


def test_reference_definitions():
    """ref_conv / ref_dgrad / ref_pool / unpool / res_scatter == their definitions written as loops."""
    gen = gen_of(0, (7,))
    x, w = ints((2, 5, 4, 3), -3, 3, gen), ints((2, 3, 3, 3), -3, 3, gen)
    for stride, pad in ((1, 1), (2, 1), (1, 0), (1, 2)):
        Ho, Wo = (5 + 2 * pad - 3) // stride + 1, (4 + 2 * pad - 3) // stride + 1
        want = torch.zeros(2, Ho, Wo, 2, dtype=torch.float64)
        for oh in range(Ho):
            for ow in range(Wo):
                for kh in range(3):
                    for kw in range(3):
                        ih, iw = oh * stride - pad + kh, ow * stride - pad + kw
                        if 0 <= ih < 5 and 0 <= iw < 4:
                            want[:, oh, ow] += x[:, ih, iw].double() @ w[:, :, kh, kw].double().t()
        assert torch.equal(ref_conv(x, w, stride, pad), want)
        # the data gradient is the adjoint: <conv(x), g> == <x, dgrad(g)>
        g = ints((2, Ho, Wo, 2), -3, 3, gen)
        assert float((want * g.double()).sum()) == float((x.double() * ref_dgrad(g, w, (5, 4), stride, pad)).sum())
    y = torch.tensor([[1., 5.], [5., 2.]]).view(1, 2, 2, 1).double()
    best, arg, ok = ref_pool(y)
    assert float(best) == 5 and not bool(ok)                      # a tie: the byte is not compared
    best, arg, ok = ref_pool(torch.tensor([[1., -5.], [0., 7.]]).view(1, 2, 2, 1).double())
    assert float(best) == 7 and int(arg) == 3 and bool(ok)       # byte = dy * 2 + dx
    best, arg, ok = ref_pool(torch.tensor([[-1., -5.], [-2., -7.]]).view(1, 2, 2, 1).double())
    assert float(best) == -1 and int(arg) == 0 and not bool(ok)  # unique but not positive
    gp = torch.tensor([3., 4.]).view(1, 1, 2, 1)
    am = torch.tensor([1, 2], dtype=torch.uint8).view(1, 1, 2, 1)
    assert unpool(gp, am).view(2, 4).tolist() == [[0, 3, 0, 0], [0, 0, 4, 0]]
    r = res_scatter(torch.ones(1, 2, 2, 1), 3, 3, 2).view(3, 3)
    assert r.tolist() == [[1, 0, 1], [0, 0, 0], [1, 0, 1]]
    # the GEMM layouts: column (kh, kw, ci) per tap, padding columns filled
    w4 = ints((4, 8, 3, 3), -3, 3, gen)
    assert igemm_w(w4)[1, (2 * 3 + 1) * 8 + 5] == w4[1, 5, 2, 1]
    assert igemm_wt(w4)[5, (0 * 3 + 1) * 4 + 2] == w4[2, 5, 2, 1]
    gw = gen_w(w4, 7.0)
    assert gw.shape == (4, 9 * 32) and gw[1, (2 * 3 + 1) * 32 + 5] == w4[1, 5, 2, 1] and gw[1, 32 + 8] == 7.0
    assert gen_w(ints((4, 4, 7, 7), -3, 3, gen), 7.0).shape == (4, 224)
    assert gen_wt(w4, True, 0.0)[5, (2 * 3 + 1) * 32 + 2] == w4[2, 5, 2, 1]
    assert gen_wt(w4, False, 0.0)[5, (0 * 3 + 1) * 32 + 2] == w4[2, 5, 2, 1]


def _igemm_all():
    return [(s, 3) for s in IGEMM_SHAPES] + [((b, 1, 1, k, n), 1) for b, k, n in LINEAR_SHAPES]


@pytest.mark.parametrize("shape,ks", _igemm_all(), ids=lambda v: case_id(v) if isinstance(v, tuple) else str(v))
def test_igemm_integer_operands_are_exact_in_fp32(shape, ks):
    """Forward and data gradient of every stride-1 case: the conv on absolute values (the bound of every partial sum
    in any order) stays <= 7776 < 2^24, the fp32 torch conv equals the fp64 one, every epilogue the GPU test asks
    for survives float32, and the Taylor sums are bounded by sum |dx| act < 2^24."""
    x, w, sc, sh = igemm_fwd_case(shape, ks)
    mag = float(ref_conv(x.abs(), w.abs()).max())
    y = ref_conv(x, w)
    assert mag <= 9 * 96 * 9 and bool((y == y.round()).all())
    y32 = F.conv2d(x.permute(0, 3, 1, 2), w, padding=ks // 2).permute(0, 2, 3, 1)
    assert torch.equal(y32.double(), y)
    for relu, slope in ((False, 0.0), (True, 0.0), (True, SLOPE)):
        assert survives_fp32(ref_fwd(x, w, sc, sh, None, relu, slope))
    g, wf, act, bsc, gp, am = igemm_bwd_case(shape, ks)
    for gg in [g] + ([unpool(gp, am)] if gp is not None else []):
        dx = ref_dgrad(gg, wf, shape[1:3])
        assert float(ref_dgrad(gg.abs(), wf.abs(), shape[1:3]).max()) <= 9 * 96 * 9
        assert bool((dx == dx.round()).all())
        assert survives_fp32(ref_bwd_out(dx, act, bsc)) and survives_fp32(ref_bwd_out(dx, act, bsc, SLOPE))
        for mode in (0, 1):
            assert float((dx.abs() * (act.double() if mode == 0 else 1)).sum((1, 2)).max()) < 2 ** 24
            assert survives_fp32(ref_taylor(dx, act, mode))
    print(f"conv exact math igemm {case_id(shape)} ks={ks}: largest sum of magnitudes {mag:.0f}")


@pytest.mark.parametrize("case", GEN_FWD_CASES, ids=case_id)
def test_gen_fwd_integer_operands_are_exact_in_fp32(case):
    H, W, Cin, Cout, ks, stride, pad = case
    x, w, sc, sh, res = gen_fwd_case(case)
    mag = float(ref_conv(x.abs(), w.abs(), stride, pad).max())
    assert mag <= 9 * 96 * 9
    for r in (None, res):
        for relu in (False, True):
            assert survives_fp32(ref_fwd(x, w, sc, sh, r, relu, 0.0, stride, pad))


@pytest.mark.parametrize("case", GEN_BWD_CASES, ids=case_id)
def test_gen_bwd_integer_operands_are_exact_in_fp32(case):
    ih, iw, C, N, ks, stride, transposed = case
    g, wf, res1, res2, mask = gen_bwd_case(case)
    dx = ref_dgrad(g, wf, (ih, iw), stride)
    assert float(ref_dgrad(g.abs(), wf.abs(), (ih, iw), stride).max()) <= 9 * 96 * 9
    assert bool((dx == dx.round()).all()) and survives_fp32(dx + res1.double())
    assert float(((dx.abs() + 8) * 3).sum((1, 2)).max()) < 2 ** 24  # every Taylor partial sum, res included


def _wino2_stage_checks(x, w, tag):
    y64, s64 = wino_emul(x, w, 2, torch.float64)
    y32, _ = wino_emul(x, w, 2, torch.float32)
    _, sab = wino_emul(x, w, 2, torch.float64, absolute=True)
    for k in ("U_obj", "V_obj", "M_obj"):
        assert bool((s64[k] == s64[k].round()).all()), k           # integers at every stage
    worst = max(sab[k] for k in ("U", "V", "M", "Y"))
    assert worst < 2.5e5 < 2 ** 24                                 # and so is every partial sum, in any order
    ref = ref_conv(x, w)
    assert torch.equal(y64, ref) and torch.equal(y32.double(), ref) and bool((ref == ref.round()).all())
    print(f"conv exact math F(2x2) {tag}: largest magnitude U {sab['U']:.0f} V {sab['V']:.0f} M {sab['M']:.0f} "
          f"Y {sab['Y']:.0f}")
    return ref


@pytest.mark.parametrize("shape", WINO2_ODD + WINO2_EVEN, ids=case_id)
def test_wino2_integer_operands_are_exact_in_fp32(shape):
    """The fp64 emulation of U = G w G^T, V = B^T d B, the per-point channel sums and A^T m A: integers at every
    stage, below 2.5e5 on absolute values, equal to conv2d in fp64 AND in fp32, forward and data gradient."""
    B, H, W, Cin, Cout = shape
    x, w, sc, sh = wino2_fwd_case(shape)
    _wino2_stage_checks(x, w, "fwd " + case_id(shape))
    assert survives_fp32(ref_fwd(x, w, sc, sh, None, True))
    g, wf, act, bsc, gp, am = wino2_bwd_case(shape)
    for gg in [g] + ([unpool(gp, am)] if gp is not None else []):
        dx = _wino2_stage_checks(gg, wf.flip(2, 3).transpose(0, 1), "dgrad " + case_id(shape))
        assert torch.equal(dx, ref_dgrad(gg, wf, (H, W)))
        assert survives_fp32(ref_bwd_out(dx, act, bsc))
        for mode in (0, 1):
            assert float((dx.abs() * (act.double() if mode == 0 else 1)).sum((1, 2)).max()) < 2 ** 24
            assert survives_fp32(ref_taylor(dx, act, mode))


def pooled_cases():
    """(name, fp64 pre-pool output) of every pooled case of the GPU file."""
    out = []
    for shape in IGEMM_SHAPES:
        x, w, sc, sh = igemm_fwd_case(shape, 3)
        for relu in (False, True):
            out.append((f"igemm {case_id(shape)} relu={relu}", ref_fwd(x, w, sc, sh, None, relu)))
    for shape in WINO2_EVEN:
        x, w, sc, sh = wino2_fwd_case(shape)
        out.append((f"F(2x2) {case_id(shape)}", ref_fwd(x, w, sc, sh, None, True)))
    return out


def test_pool_argmax_is_not_vacuous():
    """At least half of the windows of every pooled case have a unique positive maximum (measured: 0.916 .. 0.938)."""
    for name, y in pooled_cases():
        share = float(ref_pool(y)[2].float().mean())
        print(f"conv exact math pool {name}: unique positive maximum in {share:.3f} of the windows")
        assert share >= 0.5, (name, share)


@pytest.mark.parametrize("shape", [(8, 16, 32, 2, 0), (4, 8, 32, 3, 0), WINO4_BAND], ids=case_id)
def test_wino4_bound_holds_for_the_fp32_emulation(shape):
    """The F(4x4) emulation in fp64 is the conv (1e-9); its absolute form dominates |conv|; and the same steps in
    fp32 on the CPU stay under wino4_bound, per element."""
    S, C, K, B, ko = shape
    x, w, sc, sh, ref, E = wino4_fwd_case(shape)
    y64, _ = wino_emul(x, w, 4, torch.float64)
    assert float((y64 - ref_conv(x, w)).abs().max()) < 1e-9
    mag, _ = wino_emul(x, w, 4, torch.float64, absolute=True)
    assert bool((mag >= ref_conv(x, w).abs() - 1e-9).all())
    y32, _ = wino_emul(x, w, 4, torch.float32)
    err = (y32.double() * sc.double() + sh.double() - ref).abs()
    assert bool((err <= E).all()), float((err / E).max())
    print(f"conv exact math F(4x4) {case_id(shape)}: CPU fp32 emulation worst err / E {float((err / E).max()):.3f}")


def test_wino4_centre_tap_is_not_exact():
    """Why F(4x4) has no exact integer case: a weight with only the centre tap set gives U = w * G[i][1] * G[j][1],
    and 1/36 (G[1][1]^2) is no fp32 number."""
    w = torch.zeros(1, 1, 3, 3)
    w[0, 0, 1, 1] = 3.0
    _, st = wino_emul(torch.ones(1, 4, 4, 1), w, 4, torch.float64)
    U = st["U_obj"]
    assert not torch.equal(U.float().double(), U)


def test_wino4_relu_needs_no_skipped_elements():
    """max(., 0) and the window maximum are 1-Lipschitz: |relu(a) - relu(b)| <= |a - b|, so an output the ReLU
    zeroes obeys the same bound E as its pre-activation and the GPU test compares every element (share skipped: 0,
    under the 1% the issue allows). Checked from the references alone on perturbed copies."""
    for shape in WINO4_SHAPES[2:5]:
        x, w, sc, sh, ref, E = wino4_fwd_case(shape)
        gen = gen_of(9, shape)
        pert = ref + E * (2 * torch.rand(ref.shape, generator=gen, dtype=torch.float64) - 1)
        assert bool(((torch.relu(pert) - torch.relu(ref)).abs() <= E).all())
        Ep = E.unfold(1, 2, 2).unfold(2, 2, 2).reshape(*ref_pool(ref)[0].shape, 4).max(-1).values
        assert bool(((ref_pool(torch.relu(pert))[0] - ref_pool(torch.relu(ref))[0]).abs() <= Ep).all())
