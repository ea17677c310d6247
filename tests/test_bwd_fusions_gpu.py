"""The two kernels of the bottleneck backward fusion (engine/train.py ``_BNLink``), each against fp64:

- ``conv_gen_bwd_bn`` (the ``res_bits`` / ``bnb_*`` epilogue of ``tp_conv_gen``, conv_mfma.hip): the 1x1 data
  gradient, the raw residual masked by ReLU bits and the per-M-tile BatchNorm backward statistics, on every tile
  config 0..6, on ``CFG_SB | cfg`` and (one large shape) on ``cfg | CFG_SK``, element by element and tile by tile;
- ``bn_train_bwd(pre=)`` / ``bn_train_fwd(pre=)`` (``tp_bn_bwd_train_pre`` / ``tp_bn_fwd_train_pre``, batchnorm.hip):
  the fold of such tile statistics, through the G <= 256 and the G > 256 (``per > 1``) path of ``bn_fold_tiles``;
- both chained the way ``_BNLink`` wires them.

The bit masks are inputs of the kernels, not decisions they take, so no element can flip by rounding and nothing
is left out of a comparison. The reference helpers (the bit layout, the BN backward formula) are tested on the CPU
against autograd first. No bound is fitted to what the kernels give: each is derived in its test's docstring or is
the stated margin over the statistics-pass path that tests/test_train_gpu.py already covers. Every GPU test prints
its figures; those of an MI355X run are in profiles/numerics/bwd_fusions.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops
from torchpruner_amd.engine.fused_chain import CFG_SB, CFG_SK

U24 = 2.0 ** -24   # unit roundoff of fp32
FOLD = 2.0 ** -50  # the fp64 fold of the tile statistics, relative to the sum of their magnitudes
RPT_MAX = 16       # rows one thread adds in fp32 before the fp64 fold: BM / RSTEP, RSTEP = NT / (BN / 4), of the
                   # seven Tile<BM, BN, WM, WN> of gen_cfg (conv_mfma.hip): 16, 16, 4, 8, 8, 8, 4 for cfg 0..6
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the kernels take eps as a float


# ------------------------------------------------------------------------------------ reference helpers
def _nibble_weights(dev):
    return torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=dev)


def pack_bits(b):
    """bool (P, C) -> uint8[ceil(P*C/4)] in the kernels' layout: byte i, bit q = flat element 4i + q, low nibble
    only (``bits_mask`` in conv_mfma.hip, the comment on ``tp_bn_fwd_train`` in batchnorm.hip)."""
    flat = b.reshape(-1).to(torch.uint8)
    if flat.numel() % 4:
        flat = torch.cat([flat, flat.new_zeros(4 - flat.numel() % 4)])
    return (flat.view(-1, 4) * _nibble_weights(b.device)).sum(1).to(torch.uint8)


def unpack_bits(by, P, C):
    """The inverse of :func:`pack_bits`: uint8[ceil(P*C/4)] -> bool (P, C)."""
    return ((by.view(-1, 1) & _nibble_weights(by.device)) != 0).reshape(-1)[:P * C].view(P, C)


def bn_bwd_ref(g, x, gamma, mean, invstd, bits, cr):
    """Backward of y = act(BN(x)) over the rows of x (P, C) in fp64, from the forward's saved mean / invstd (C,) and
    the activation's pass bits (bool (P, C), None: no activation). Channels c >= cr are padding: everything is zero
    there and dgamma / dbeta have cr entries (gamma (cr,), None: ones).
    gm = g * bits, dbeta = sum gm, dgamma = sum gm * xhat, dx = gamma * invstd * (gm - dbeta/P - xhat * dgamma/P),
    dres = gm."""
    P, C = x.shape
    live = (torch.arange(C, device=x.device) < cr).double()
    gm = g.double() * live
    if bits is not None:
        gm = gm * bits.double()
    is64 = invstd.double()
    xhat = (x.double() - mean.double()) * is64
    dbeta, dgamma = gm.sum(0), (gm * xhat).sum(0)
    ga = torch.ones(C, dtype=torch.float64, device=x.device)
    if gamma is not None:
        ga[:cr] = gamma.double()
    dx = ga * is64 * (gm - dbeta / P - xhat * dgamma / P) * live
    return {"gm": gm, "dbeta": dbeta[:cr], "dgamma": dgamma[:cr], "dx": dx, "dres": gm}


@pytest.mark.parametrize("P,C", [(1, 4), (3, 8), (5, 13), (7, 70), (2, 1)])
def test_pack_bits_round_trip(P, C):
    g = torch.Generator().manual_seed(P * 100 + C)
    b = torch.rand(P, C, generator=g) < 0.5
    by = pack_bits(b)
    assert by.dtype == torch.uint8 and by.numel() == (P * C + 3) // 4 and int(by.max()) < 16
    assert torch.equal(unpack_bits(by, P, C), b)
    # the layout itself, element by element: flat element e is bit e % 4 of byte e // 4
    flat = b.reshape(-1).tolist()
    for e, bit in enumerate(flat):
        assert ((int(by[e // 4]) >> (e % 4)) & 1) == int(bit)
    for e in range(len(flat), 4 * by.numel()):  # the bits past the last element are clear
        assert ((int(by[e // 4]) >> (e % 4)) & 1) == 0


@pytest.mark.parametrize("C,cr", [(8, 8), (13, 13), (70, 70), (13, 10), (70, 66)])
def test_bn_bwd_ref_matches_autograd(C, cr):
    """bn_bwd_ref == fp64 autograd of relu(batch_norm(x, training=True)) with bits = (y > 0), and zero at c >= cr."""
    P = 37
    g = torch.Generator().manual_seed(C + cr)
    x = (torch.randn(P, C, generator=g, dtype=torch.float64) * 3 + 1)
    x[:, cr:] = 0
    gy = torch.randn(P, C, generator=g, dtype=torch.float64)
    gamma = (torch.rand(cr, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(cr, generator=g, dtype=torch.float64).requires_grad_(True)
    xr = x[:, :cr].clone().requires_grad_(True)
    y = torch.relu(F.batch_norm(xr, None, None, gamma, beta, True, 0.1, EPS))
    y.backward(gy[:, :cr])
    mean = x.mean(0)
    invstd = (x.var(0, unbiased=False) + EPS).rsqrt()
    bits = torch.zeros(P, C, dtype=torch.bool)
    bits[:, :cr] = y > 0
    assert 0.2 < float(bits[:, :cr].double().mean()) < 0.8
    ref = bn_bwd_ref(gy, x, gamma.detach(), mean, invstd, bits, cr)
    tight = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(ref["dx"][:, :cr], xr.grad, **tight)
    torch.testing.assert_close(ref["dgamma"], gamma.grad, **tight)
    torch.testing.assert_close(ref["dbeta"], beta.grad, **tight)
    assert torch.equal(ref["dres"][:, :cr], gy[:, :cr] * (y > 0))
    assert not bool(ref["dx"][:, cr:].any()) and not bool(ref["dres"][:, cr:].any())
    # without an activation: plain batch norm
    xr2 = x[:, :cr].clone().requires_grad_(True)
    F.batch_norm(xr2, None, None, gamma.detach(), None, True, 0.1, EPS).backward(gy[:, :cr])
    plain = bn_bwd_ref(gy, x, gamma.detach(), mean, invstd, None, cr)
    torch.testing.assert_close(plain["dx"][:, :cr], xr2.grad, **tight)


def _ratio(err, bound):
    """max err / bound over the entries with a non-zero bound; asserts err <= bound everywhere (0 <= 0 included)."""
    worst = float(torch.where(bound > 0, err / bound, torch.zeros_like(err)).max()) if err.numel() else 0.0
    assert bool((err <= bound).all()), f"max err / bound = {worst}, {int((err > bound).sum())} entries over"
    return worst


# --------------------------------------------------------------------------------------- conv_gen_bwd_bn
# (B, H, W, C, N)
SHAPES = [(1, 1, 1, 8, 8),          # one row, minimum widths
          (3, 7, 9, 64, 36),        # M = 189 ragged for 64/128/256-row tiles, N below one 64-wide tile
          (2, 14, 14, 40, 136),     # C off the 32-wide K slice, N = 2 tiles + 8 columns
          (5, 8, 8, 96, 64),        # M = 320: exact for 64-row tiles, ragged for 128/256
          (4, 16, 16, 256, 128)]    # exact multiples everywhere
SK_SHAPE = (256, 7, 7, 256, 512)    # the M x N of test_streamk_dgrad_mask_res_taylor (stream-K applies), K = 256
# name -> (res_stride, 0 = no res; res_bits; bn; bn_bits)
VARIANTS = {"bn_bits": (0, False, True, True), "res_bn": (1, False, True, False), "res_rbits": (1, True, False, False),
            "full": (1, True, True, True), "res2_bn_bits": (2, False, True, True)}


def _tile_m(cfg):
    """tp_conv_tile_m"""
    base = cfg & ~(CFG_SK | CFG_SB)
    return 256 if base in (1, 5) else 64 if base == 2 else 128


def _make_operands(shape, pad, dev):
    """fp32 operands of one shape on the device. ``pad``: the columns from cr = N - 8 up are channel padding (wt
    rows, bn_y and res columns zero there)."""
    B, H, W, C, N = shape
    gen = torch.Generator().manual_seed(sum(p * s for p, s in zip((10007, 1009, 101, 11, 1), shape)) + int(pad))
    K, M = (C + 31) // 32 * 32, B * H * W
    o = {"g": torch.randn(B, H, W, C, generator=gen), "wt": torch.zeros(N, K),
         "res": torch.randn(B, H, W, N, generator=gen),
         "res2": torch.randn(B, (H + 1) // 2, (W + 1) // 2, N, generator=gen),
         "y": torch.randn(B, H, W, N, generator=gen) * 2 + 0.5,
         "mean": torch.rand(N, generator=gen) + 0.5, "invstd": torch.rand(N, generator=gen) + 0.5}
    o["wt"][:, :C] = torch.randn(N, C, generator=gen) * C ** -0.5
    rbits, bbits = torch.rand(M, N, generator=gen) < 0.5, torch.rand(M, N, generator=gen) < 0.5
    if pad:
        cr = N - 8
        o["wt"][cr:] = 0
        for k in ("res", "res2", "y"):
            o[k][..., cr:] = 0
    o = {k: v.to(dev) for k, v in o.items()}
    o["rbits"], o["bbits"] = rbits.to(dev), bbits.to(dev)
    o["rbytes"], o["bbytes"] = pack_bits(o["rbits"]), pack_bits(o["bbits"])
    o["shape"], o["K"] = shape, K
    return o


def _make_reference(o, variant):
    """fp64 on the device: dx (M, N), its element bound E, and for the statistics the (2, M, N) stacks of
    the terms gm * w, their bounds' first part bit * E * w and their magnitudes |gm * w| (w = 1, |xhat|)."""
    B, H, W, C, N = o["shape"]
    M = B * H * W
    rs, rb, bn, bb = VARIANTS[variant]
    g, wt = o["g"].view(M, C).double(), o["wt"][:, :C].double()
    dx = g @ wt.t()
    mag = g.abs() @ wt.abs().t()
    if rs:
        res = o["res"].double()
        if rs == 2:  # the residual lives at the even-phase pixels
            res = torch.zeros_like(res)
            res[:, ::2, ::2] = o["res2"].double()
        res = res.view(M, N)
        dx = dx + (res * o["rbits"] if rb else res)
        mag = mag + res.abs()
    r = {"dx": dx, "E": (o["K"] + 4) * U24 * mag}
    if bn:
        bits = o["bbits"].double() if bb else torch.ones_like(dx)
        xhat = (o["y"].view(M, N).double() - o["mean"].double()) * o["invstd"].double()
        gm = dx * bits
        r["terms"] = torch.stack([gm, gm * xhat])
        r["e_terms"] = torch.stack([bits * r["E"], bits * r["E"] * xhat.abs()])
    return r


_operands = functools.lru_cache(maxsize=None)(_make_operands)


@functools.lru_cache(maxsize=None)
def _reference(shape, pad, variant, dev):
    """Computed once per (shape, variant), read-only."""
    return _make_reference(_operands(shape, pad, dev), variant)


def _tile_sums(a, tm):
    """(2, M, N) -> (ceil(M / tm), 2, N): sums over the rows [t*tm, min((t+1)*tm, M)) of every tile t."""
    M = a.shape[1]
    tiles = -(-M // tm)
    return F.pad(a, (0, 0, 0, tiles * tm - M)).view(2, tiles, tm, -1).sum(2).permute(1, 0, 2)


def _launch(T, o, variant, cfg):
    rs, rb, bn, bb = VARIANTS[variant]
    res = None if not rs else o["res"] if rs == 1 else o["res2"]
    return T.conv_gen_bwd_bn(o["g"], o["wt"], res, max(rs, 1), o["rbytes"] if rb else None, o["y"] if bn else None,
                             o["mean"] if bn else None, o["invstd"] if bn else None, o["bbytes"] if bb else None, cfg)


def _check_conv(dx, part, o, ref, variant, cfg):
    """dx element by element and part tile by tile against fp64; returns the three largest err / bound."""
    B, H, W, C, N = o["shape"]
    M, tm = B * H * W, _tile_m(cfg)
    assert tuple(dx.shape) == (B, H, W, N)
    r_dx = _ratio((dx.view(M, N).double() - ref["dx"]).abs(), ref["E"])
    if not VARIANTS[variant][2]:
        assert part is None or part.numel() == 0  # no BN: no statistics
        return r_dx, 0.0, 0.0
    assert part.dtype == torch.float64 and tuple(part.shape) == (-(-M // tm), 2, N)
    want = _tile_sums(ref["terms"], tm)
    bound = _tile_sums(ref["e_terms"], tm) + (RPT_MAX + 4) * U24 * _tile_sums(ref["terms"].abs(), tm)
    err = (part - want).abs()
    return r_dx, _ratio(err[:, 0], bound[:, 0]), _ratio(err[:, 1], bound[:, 1])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", range(7))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_gen_bwd_bn_every_tile_config(cuda, shape, variant, cfg):
    """dx = g @ wt[:, :C]^T + res * res_bits (NOT masked by bn_bits: the kernel stores the raw gradient and masks
    inside the statistics only) and part[t] = (sum gm, sum gm * xhat) over the rows of M tile t, gm = dx * bn_bits,
    xhat = (bn_y - mean) * invstd, against fp64 — every element, every (tile, statistic, column).

    dx, per element:  E = (K + 4) * 2^-24 * ((|g| @ |wt|^T) + |res|),  K = conv_gen_k(1, C). The fp32 MFMA is a
    k-ordered fma chain with one rounding per k step, each relative to a partial sum that the magnitude sum bounds;
    the residual add is one more, a stream-K tile's merge of its two partial sums another (the form of the
    prefix-delta bound in test_shapley_delta_gpu.py).

    part, per (tile, column), with w = 1 for the first statistic and w = |xhat| for the second:
        sum_rows bit * E * w  +  (RPT_MAX + 4) * 2^-24 * sum_rows |gm_ref * w|.
    First part: the kernel sums its own fp32 dx, each within E of the reference. Second part: the fp32 evaluation of
    one term gm * xhat rounds three times (the subtraction, the two products; y, mean and invstd are fp32 inputs,
    read exactly by the reference), and a thread adds at most RPT_MAX = 16 terms into its fp32 partial (BM / RSTEP
    rows, see RPT_MAX above), one rounding per add, relative to a running sum that sum |gm * w| bounds: RPT_MAX + 3
    roundings, the fourth unit covers the products of two roundings. The RSTEP partials of a column are then added in
    fp64 (2^-53: nothing at this scale).

    Also: ``CFG_SB | cfg`` (single-buffered LDS stage, K <= 256 here) gives the bits of ``cfg`` for dx and part (same
    MFMA order); a second call gives the same bits (no atomics); for the full variant, with the columns from
    cr = N - 8 up made channel padding (wt rows, bn_y and res columns zero), dx and part are exactly zero there."""
    T = ops.require()
    dev = str(cuda)
    o = _operands(shape, False, dev)
    assert o["K"] == T.conv_gen_k(1, shape[3]) <= 256
    ref = _reference(shape, False, variant, dev)
    dx, part = _launch(T, o, variant, cfg)
    r = _check_conv(dx, part, o, ref, variant, cfg)
    print(f"bwd_fusions conv shape={'x'.join(map(str, shape))} variant={variant} cfg={cfg} "
          f"dx={r[0]:.4f} stat0={r[1]:.4f} stat1={r[2]:.4f}")
    has_part = VARIANTS[variant][2]
    for other in (cfg, CFG_SB | cfg):  # repeatable; the single-buffered stage is the same arithmetic
        dx2, part2 = _launch(T, o, variant, other)
        assert torch.equal(dx2, dx), f"dx of cfg {other} differs from cfg {cfg}"
        if has_part:
            assert part2.shape == part.shape and torch.equal(part2, part), f"part of cfg {other} differs from {cfg}"
    if variant == "full":
        N, cr = shape[4], shape[4] - 8
        op = _operands(shape, True, dev)
        dxp, partp = _launch(T, op, variant, cfg)
        _check_conv(dxp, partp, op, _reference(shape, True, variant, dev), variant, cfg)
        assert not bool(dxp[..., cr:].any()) and not bool(partp[:, :, cr:].any()), "padding columns are not zero"
        assert cr == 0 or (bool(dxp[..., :cr].any()) and bool(partp[:, :, :cr].any()))


@pytest.mark.gpu
def test_conv_gen_bwd_bn_streamk(cuda):
    """``cfg | CFG_SK`` with the full epilogue (res + res_bits + bn + bn_bits) at a shape where stream-K applies:
    cut tiles get their epilogue, statistics included, from the fixup launch. Against fp64 per element and per tile
    under the bounds of test_conv_gen_bwd_bn_every_tile_config (the merge of a cut tile's two partial sums is one of
    the K + 4 roundings); against the data-parallel launch of the same cfg: the same part.shape, and both within
    their bound of the same reference, so they differ by at most twice the bound; and bit for bit repeatable."""
    T = ops.require()
    B, H, W, C, N = SK_SHAPE
    M = B * H * W
    cfgs = [c for c in range(7) if T.conv_sk_ws(c, 1, False, M, N) > 0]
    assert cfgs, f"stream-K applies to no tile config at M={M} N={N}"
    o = _make_operands(SK_SHAPE, False, cuda)
    ref = _make_reference(o, "full")
    for cfg in cfgs:
        dx, part = _launch(T, o, "full", cfg | CFG_SK)
        r = _check_conv(dx, part, o, ref, "full", cfg)
        print(f"bwd_fusions streamk shape={'x'.join(map(str, SK_SHAPE))} variant=full cfg={cfg}|SK "
              f"dx={r[0]:.4f} stat0={r[1]:.4f} stat1={r[2]:.4f}")
        dx2, part2 = _launch(T, o, "full", cfg | CFG_SK)
        assert torch.equal(dx2, dx) and torch.equal(part2, part), f"cfg {cfg}: stream-K is not repeatable"
        dxd, partd = _launch(T, o, "full", cfg)
        _check_conv(dxd, partd, o, ref, "full", cfg)
        assert partd.shape == part.shape
        tm = _tile_m(cfg)
        _ratio((dx.double() - dxd.double()).abs().view(M, N), 2 * ref["E"])
        _ratio((part - partd).abs(), 2 * (_tile_sums(ref["e_terms"], tm)
                                          + (RPT_MAX + 4) * U24 * _tile_sums(ref["terms"].abs(), tm)))


# ------------------------------------------------------------------------- the tile fold: synthetic tiles
GS = [1, 3, 255, 256, 257, 511, 1000]  # bn_fold_tiles: per = 1 up to 256 tiles, per = 2 .. 4 above
CCR = [(8, 8), (52, 52), (70, 70), (130, 130), (13, 13), (13, 10), (70, 66)]  # (C, cr): <64, >64, >128 channels
P_ROWS = 96


@functools.lru_cache(maxsize=None)
def _bn_case(C, cr, G, dev):
    """Rows, gradient, bits and the tile of every row: P_ROWS rows cut into G contiguous tiles of random length
    (many of them empty when G > P_ROWS). x is zero at the padding channels c >= cr, as the forward leaves it, and
    so are the bits; g is not."""
    gen = torch.Generator().manual_seed(1000 * C + 10 * cr + G)
    x = torch.randn(P_ROWS, C, generator=gen) * 3 + 1
    x[:, cr:] = 0
    g = torch.randn(P_ROWS, C, generator=gen)
    bits = torch.rand(P_ROWS, C, generator=gen) < 0.5
    bits[:, cr:] = False
    ym = torch.where(bits, torch.rand(P_ROWS, C, generator=gen) + 0.1, -torch.rand(P_ROWS, C, generator=gen))
    ym = torch.where(~bits & (torch.rand(P_ROWS, C, generator=gen) < 0.2), torch.zeros(()), ym)  # 0 does not pass
    assert torch.equal(ym > 0, bits)
    gamma, beta = torch.rand(cr, generator=gen) + 0.5, torch.randn(cr, generator=gen)
    cuts = torch.sort(torch.randint(0, P_ROWS + 1, (G - 1,), generator=gen)).values
    tile = torch.searchsorted(cuts, torch.arange(P_ROWS), right=True)  # tile t = rows [cuts[t-1], cuts[t])
    assert int(tile.max()) < G and bool((tile[1:] >= tile[:-1]).all())
    x64 = x.double()
    mean = x64.mean(0).float()
    invstd = (x64.var(0, unbiased=False) + EPS).rsqrt().float()
    c = {"x": x, "g": g, "bits": bits, "ym": ym, "gamma": gamma, "beta": beta, "tile": tile, "mean": mean,
         "invstd": invstd}
    return {k: v.to(dev) for k, v in c.items()}


def _tile_pre(vals, tile, G):
    """(P, 2, C) fp64 per-row terms -> (G, 2, C) per-tile sums (zeros for an empty tile)."""
    return torch.zeros(G, *vals.shape[1:], dtype=torch.float64, device=vals.device).index_add_(0, tile, vals)


def _dx_yardstick(what, got_pre, got_none, want):
    """The pre= path against the statistics-pass path (pre=None), both fp32 evaluations of one formula whose
    statistics differ by rounding only: its largest error may be 4x the other's, plus 1e-7 * max |reference|."""
    e_pre = float((got_pre.double() - want).abs().max())
    e_none = float((got_none.double() - want).abs().max())
    assert e_pre <= 4 * e_none + 1e-7 * float(want.abs().max()), (what, e_pre, e_none)
    return e_pre, e_none


@pytest.mark.gpu
@pytest.mark.parametrize("C,cr", CCR)
@pytest.mark.parametrize("G", GS)
def test_bn_train_bwd_pre_synthetic_tiles(cuda, G, C, cr):
    """``bn_train_bwd(pre=)`` on tile statistics built here: pre[t] = fp64 (sum gm, sum gm * xhat) over the rows of
    tile t. With the forward's bit mask (``mask=``), with its output instead (``ym=``) and with no activation.

    dgamma / dbeta against fp64: |err| <= 2^-24 * |value| + 2^-50 * sum_t |pre[t]|, the one fp32 rounding of the
    stored value plus the fp64 fold of the tiles (bn_fold_tiles, then fold_groups of the finalize kernel).
    dx against bn_bwd_ref under the margin of _dx_yardstick; dres is g * bits exactly. Padding channels (cr < C): dx is
    zero whatever g holds there; dres is the masked gradient as it is, zero where the forward's bits are zero, and
    without an activation g itself (the kernel has no bits to mask it by: pinned here, not part of bn_bwd_ref)."""
    T = ops.require()
    c = _bn_case(C, cr, G, str(cuda))
    x, g, tile = c["x"], c["g"], c["tile"]
    xhat = (x.double() - c["mean"].double()) * c["invstd"].double()
    for mode in ("mask", "ym", "none"):
        bits = None if mode == "none" else c["bits"]
        gm_k = g.double() if bits is None else g.double() * bits  # what the kernels call gm (padding not zeroed)
        pre = _tile_pre(torch.stack([gm_k, gm_k * xhat], 1), tile, G)
        ref = bn_bwd_ref(g, x, c["gamma"], c["mean"], c["invstd"], bits, cr)
        kw = dict(ym=c["ym"] if mode == "ym" else None, want_dres=True,
                  mask=pack_bits(c["bits"]) if mode == "mask" else None, cr=cr, act=0 if mode == "none" else 1)
        dx, dgamma, dbeta, dres = T.bn_train_bwd(g, x, c["gamma"], c["mean"], c["invstd"], True, pre=pre, **kw)
        dx0, _, _, dres0 = T.bn_train_bwd(g, x, c["gamma"], c["mean"], c["invstd"], True, pre=None, **kw)
        assert tuple(dgamma.shape) == tuple(dbeta.shape) == (cr,) and dx.shape == x.shape == dres.shape
        terms = pre.abs().sum(0)[:, :cr]
        r_b = _ratio((dbeta.double() - ref["dbeta"]).abs(), U24 * ref["dbeta"].abs() + FOLD * terms[0])
        r_g = _ratio((dgamma.double() - ref["dgamma"]).abs(), U24 * ref["dgamma"].abs() + FOLD * terms[1])
        e_pre, e_none = _dx_yardstick((mode, G, C, cr), dx, dx0, ref["dx"])
        assert not bool(dx[:, cr:].any())
        assert torch.equal(dres.double()[:, :cr], ref["dres"][:, :cr]) and torch.equal(dres, dres0)
        assert torch.equal(dres[:, cr:], g[:, cr:] if mode == "none" else torch.zeros_like(g[:, cr:]))
        print(f"bwd_fusions fold_bwd G={G} C={C} cr={cr} mode={mode} dbeta={r_b:.4f} dgamma={r_g:.4f} "
              f"dx_err_pre={e_pre:.3e} dx_err_none={e_none:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("C,cr", CCR)
@pytest.mark.parametrize("G", GS)
def test_bn_train_fwd_pre_synthetic_tiles(cuda, G, C, cr):
    """``bn_train_fwd(pre=)`` on pre[t] = fp64 (sum x, sum x^2) of tile t, against fp64 batch norm, with and without
    the ReLU. Bounds (s = sum_t |pre[t, 0]|, q = sum_t |pre[t, 1]| per channel, P rows):
      mean:   2^-24 * |mean| + 2^-50 * s / P  (the fp64 fold, one rounding to fp32);
      invstd: 2^-24 * invstd + invstd * dv / (2 * (var + eps)),  dv = 2^-48 * (q / P + mean^2): var = q/P - mean^2 is
              formed in fp64 from the folded sums (two folds, the square, the subtraction), and d(invstd) =
              invstd * dv / (2 (var + eps));
      running_mean (from 0) = fl(mom) * fl(mean): three roundings, 3 * 2^-24 * |value|, plus mom * the mean's fold;
      running_var (from 1) = (1 - mom) * 1 + mom * var_unbiased: three roundings in each term (fl(mom), the
              subtraction or fl(var), the product) and the last add: 4 * 2^-24 * (|t1| + |t2|), plus mom * dv * P/(P-1);
      y: the margin of _dx_yardstick over the statistics-pass forward (ReLU is 1-Lipschitz); the returned bit mask is
              (y > 0) of the kernel's own y; y is zero at the padding channels."""
    T = ops.require()
    c = _bn_case(C, cr, G, str(cuda))
    x, P, mom = c["x"], P_ROWS, 0.1
    x64 = x.double()
    pre = _tile_pre(torch.stack([x64, x64 * x64], 1), c["tile"], G)
    mean64, var64 = x64.mean(0), x64.var(0, unbiased=False)
    is64 = (var64 + EPS).rsqrt()
    rm64, rv64 = torch.zeros(cr, dtype=torch.float64, device=cuda), torch.ones(cr, dtype=torch.float64, device=cuda)
    y64 = torch.zeros_like(x64)
    y64[:, :cr] = F.batch_norm(x64[:, :cr], rm64, rv64, c["gamma"].double(), c["beta"].double(), True, mom, EPS)
    s, q = pre.abs().sum(0)
    dv = 2.0 ** -48 * (q / P + mean64 ** 2)
    for act in (0, 1):
        outs = []
        for p in (pre, None):
            rm, rv = torch.zeros(cr, device=cuda), torch.ones(cr, device=cuda)
            y, mean, invstd, mk = T.bn_train_fwd(x, c["gamma"], c["beta"], rm, rv, EPS, mom, pre=p, cr=cr, act=act)
            outs.append((y, mean, invstd, mk, rm, rv))
        y, mean, invstd, mk, rm, rv = outs[0]
        assert tuple(mean.shape) == tuple(invstd.shape) == (C,) and y.shape == x.shape
        r_m = _ratio((mean.double() - mean64).abs(), U24 * mean64.abs() + FOLD * s / P)
        r_i = _ratio((invstd.double() - is64).abs(), U24 * is64 + is64 * dv / (2 * (var64 + EPS)))
        r_rm = _ratio((rm.double() - rm64).abs(), 3 * U24 * rm64.abs() + mom * FOLD * s[:cr] / P)
        t1, t2 = (1 - mom) * torch.ones_like(rv64), rv64 - (1 - mom)
        r_rv = _ratio((rv.double() - rv64).abs(), 4 * U24 * (t1 + t2.abs()) + mom * dv[:cr] * P / (P - 1))
        want = y64.clamp_min(0) if act else y64
        e_pre, e_none = _dx_yardstick((act, G, C, cr), y, outs[1][0], want)
        assert not bool(y[:, cr:].any())
        if act:
            assert torch.equal(unpack_bits(mk, P, C), y > 0)
        else:
            assert mk.numel() == 0
        print(f"bwd_fusions fold_fwd G={G} C={C} cr={cr} act={act} mean={r_m:.4f} invstd={r_i:.4f} "
              f"running_mean={r_rm:.4f} running_var={r_rv:.4f} y_err_pre={e_pre:.3e} y_err_none={e_none:.3e}")


# --------------------------------------------------------------------------------- the chain of _BNLink
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [0, 1, 2, CFG_SB | 2])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=lambda s: "x".join(map(str, s)))
def test_bn_link_chain(cuda, shape, cfg):
    """The three calls as engine/train.py chains them: bn_train_fwd(x, act=1) -> y, mean, invstd, mk;
    conv_gen_bwd_bn(g, wt, res, 1, res_bits, x, mean, invstd, mk, cfg) -> dxh, part;
    bn_train_bwd(dxh, x, gamma, mean, invstd, mask=mk, pre=part). Against bn_bwd_ref on the fp64 dxh with the
    kernel's own mk unpacked (the decisions are replayed, as engine/oracle.py does) and its fp32 mean / invstd, and
    against the same bn_train_bwd call with pre=None.

    dgamma / dbeta: the per-tile bounds of test_conv_gen_bwd_bn_every_tile_config summed over the tiles (= over all
    rows), plus the fold's 2^-24 * |value| + 2^-50 * sum_t |part_ref[t]|. dx: the margin of _dx_yardstick (both
    paths read the same fp32 dxh). dres = dxh masked by mk, the same bits from both paths."""
    T = ops.require()
    B, H, W, C, N = shape
    M = B * H * W
    o = _operands(shape, False, str(cuda))
    gen = torch.Generator().manual_seed(M + N)
    gamma, beta = (torch.rand(N, generator=gen) + 0.5).to(cuda), torch.randn(N, generator=gen).to(cuda)
    x = o["y"]  # the BN's input
    y, mean, invstd, mk = T.bn_train_fwd(x, gamma, beta, None, None, EPS, 0.1, act=1)
    bits = unpack_bits(mk, M, N)
    assert torch.equal(bits, y.view(M, N) > 0) and 0.2 < float(bits.double().mean()) < 0.8
    dxh, part = T.conv_gen_bwd_bn(o["g"], o["wt"], o["res"], 1, o["rbytes"], x, mean, invstd, mk, cfg)
    cref = _reference(shape, False, "res_rbits", str(cuda))  # dx = g @ wt^T + res * res_bits and its bound E
    _ratio((dxh.view(M, N).double() - cref["dx"]).abs(), cref["E"])
    x2, g2 = x.view(M, N), dxh.view(M, N)
    ref = bn_bwd_ref(cref["dx"], x2, gamma, mean, invstd, bits, N)
    xhat = (x2.double() - mean.double()) * invstd.double()
    terms = torch.stack([ref["gm"], ref["gm"] * xhat])
    e_terms = torch.stack([bits * cref["E"], bits * cref["E"] * xhat.abs()])
    assert tuple(part.shape) == (-(-M // _tile_m(cfg)), 2, N)
    fold = FOLD * _tile_sums(terms, _tile_m(cfg)).abs().sum(0)
    bound = e_terms.sum(1) + (RPT_MAX + 4) * U24 * terms.abs().sum(1) + fold
    dx, dgamma, dbeta, dres = T.bn_train_bwd(g2, x2, gamma, mean, invstd, True, None, True, mk, N, part, 1)
    dx0, dgamma0, dbeta0, dres0 = T.bn_train_bwd(g2, x2, gamma, mean, invstd, True, None, True, mk, N, None, 1)
    r_b = _ratio((dbeta.double() - ref["dbeta"]).abs(), bound[0] + U24 * ref["dbeta"].abs())
    r_g = _ratio((dgamma.double() - ref["dgamma"]).abs(), bound[1] + U24 * ref["dgamma"].abs())
    # the statistics pass (bn_partial) sums the same fp32 dxh with the same three roundings per term and at most
    # ceil(rows_per_group / 16) <= 8 fp32 adds per thread for P >= 64 rows (bn_groups gives groups of < 128 rows):
    # it meets the same bound, so the two paths are at most twice the bound apart
    assert M >= 64
    _ratio((dbeta - dbeta0).double().abs(), 2 * (bound[0] + U24 * ref["dbeta"].abs()))
    _ratio((dgamma - dgamma0).double().abs(), 2 * (bound[1] + U24 * ref["dgamma"].abs()))
    e_pre, e_none = _dx_yardstick((shape, cfg), dx, dx0, ref["dx"])
    assert torch.equal(dres, dres0) and torch.equal(dres, g2 * bits)
    print(f"bwd_fusions chain shape={'x'.join(map(str, shape))} cfg={cfg} dbeta={r_b:.4f} dgamma={r_g:.4f} "
          f"dx_err_pre={e_pre:.3e} dx_err_none={e_none:.3e}")
