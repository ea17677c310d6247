"""The training BatchNorm kernels of csrc/kernels/batchnorm.hip, called directly (``bn_train_fwd``,
``bn_train_bwd``, their ``pre=`` forms, and the Hardswish / SiLU unit tails) at the edges of their row walk,
column blocks, carried widths, masks and statistics, against the hand-written fp64 reference and the a-priori
bounds of tests/bn_reference.py (checked on the CPU by tests/test_bn_reference.py).

Every comparison is split in two: (a) the returned fp32 mean / invstd / running statistics against fp64 from
x; (b) y, the mask, dx, dgamma, dbeta and dres against fp64 evaluated from the kernel's own returned mean and
invstd. Every tolerance is a bound function of bn_reference (or of this file, for the unit tails' activation
arithmetic) with its derivation at its definition; none is fitted to what the kernels give. Bit masks and
dres are compared exactly. Every test prints its largest err / bound."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_reference as R

pytestmark = pytest.mark.gpu

U = R.U
RPT_MAX = 16  # rows a thread of a conv epilogue adds in fp32 into a tile statistic (tests/test_bwd_fusions_gpu.py)


# ----------------------------------------------------------------------------------------- operands
def _inputs(P, C, cr, seed, dev, fam="std", res=False):
    """x, gamma, beta, res, g: x zero and g = 1.0 in the padding channels c >= cr."""
    crr = cr or C
    gen = torch.Generator().manual_seed(seed)
    if fam == "std":
        x = torch.randn(P, C, generator=gen) * 3 + 1
    else:
        x = torch.randn(P, C, generator=gen) + float(fam)
    gamma, beta = torch.rand(crr, generator=gen) * 1.5 + 1.5, torch.rand(crr, generator=gen) * 4 + 1
    rs = torch.randn(P, C, generator=gen) if res else None
    g = torch.randn(P, C, generator=gen)
    x[:, crr:] = 0
    g[:, crr:] = 1.0
    if res:
        rs[:, crr:] = 0
    return tuple(t.to(dev) if t is not None else None for t in (x, gamma, beta, rs, g))


def _running0(n, dev):
    gen = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=gen).to(dev), (torch.rand(n, generator=gen) + 0.5).to(dev)


def _bits(mk, P, C):
    bits, rest = R.unpack_bits(mk, P * C)
    assert not bool(rest.any()), "a bit past the last element (or in a high nibble) is set"
    return bits.view(P, C)


def _same_bits(a, b):
    """fp32 tensors equal bit for bit (-0.0 != +0.0, NaN == the same NaN)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_fwd(T, x, out, gamma, beta, res, act, cr, rows, what, run=None):
    """Checks (a) and (b) of one forward call; returns the kernel's keep bits (None without an activation) and
    the worst ratios. ``run``: (old mean, old var, new mean, new var, momentum) of the running statistics.
    ``rows``: R of the statistics' bound."""
    y, mean_k, invstd_k, mk = out
    P, C = x.shape
    crr = cr or C
    assert y.shape == x.shape and mean_k.shape == invstd_k.shape == (C,)
    mean, var, em, ev = R.check_stats(x, mean_k, invstd_k, rows, what=what)
    w = {}
    if run is not None:
        rm0, rv0, rm, rv, mom = run
        rrm, rrv, vstat = R.running(rm0, rv0, mean[:crr], var[:crr], P, mom)
        scale = P / (P - 1) if P > 1 else 1.0
        w["rm"] = R.check((rm.double() - rrm).abs(), R.e_running(em[:crr], mom, rm0, rrm), what + " running_mean")
        w["rv"] = R.check((rv.double() - rrv).abs(), R.e_running(ev[:crr] * scale + U * vstat.abs(), mom, rv0, rrv),
                          what + " running_var")
    fw = R.fwd_from_stats(x, mean_k, invstd_k, gamma, beta, res, act, cr)
    w["y"] = R.check((y.double() - fw["y"]).abs(), R.e_y(x, fw, res), what + " y")
    assert not bool(y[:, crr:].any()), "y is not zero in the padding"
    keep = None
    if act:
        assert mk.dtype == torch.uint8 and mk.numel() == (P * C + 3) // 4
        keep = _bits(mk, P, C)
        assert torch.equal(keep, R.act_bit(y, act)), f"{what}: mask bits differ from bn_act_bit of the kernel's own y"
        assert not bool(keep[:, crr:].any())
    else:
        assert mk.numel() == 0
    return keep, w


def _check_bwd(x, g, outs, gamma, mean_k, invstd_k, keep, cr, rows, what, e_sums=None):
    """Check (b) of one backward call. ``e_sums``: (E_sg, E_sgx) when the sums come from tile statistics."""
    dx, dgamma, dbeta, dres = outs
    P, C = x.shape
    crr = cr or C
    bw = R.bwd_from_stats(g, x, mean_k, invstd_k, gamma, keep, cr)
    assert dgamma.shape == dbeta.shape == (crr,)
    if e_sums is None:
        e0, e1 = R.e_sum(bw["abs0"], rows), R.e_sum(bw["abs1"], rows)
        s0, s1 = e0, e1
    else:
        e0, e1 = e_sums
        s0, s1 = e0 + U * bw["abs0"], e1 + U * bw["abs1"]  # the fp32 store: u |sum| <= u sum|term|
    w = {"dbeta": R.check((dbeta.double() - bw["dbeta"]).abs(), s0[:crr], what + " dbeta"),
         "dgamma": R.check((dgamma.double() - bw["dgamma"]).abs(), s1[:crr], what + " dgamma")}
    if dx is not None:
        w["dx"] = R.check((dx.double() - bw["dx"]).abs(), R.e_dx(x, bw, P, e0, e1), what + " dx")
        assert not bool(dx[:, crr:].any()), "dx is not zero in the padding"
    if dres is not None:
        ref = g if keep is None else torch.where(keep, g, torch.zeros_like(g))
        assert _same_bits(dres, ref), f"{what}: dres is not the masked g bit for bit"
    return w


def _fmt(*ws):
    return " ".join(f"{k}={v:.3f}" for w in ws for k, v in w.items())


# ------------------------------------------------------------------------------- rows and columns
@pytest.mark.parametrize("P,C", R.GEOMETRY, ids=[f"{p}x{c}" for p, c in R.GEOMETRY])
def test_geometry(cuda, P, C):
    """Forward and backward at every row / column geometry of R.GEOMETRY, ReLU6 (even P) or ReLU (odd P) with the
    bit mask, running statistics, then the backward with dres."""
    from torchpruner_amd import ops
    T = ops.require()
    act = 2 if P % 2 == 0 else 1
    x, gamma, beta, _, g = _inputs(P, C, 0, P * 131 + C, cuda)
    rows = R.rows_per_thread(P, C, T)
    rm0, rv0 = _running0(C, cuda)
    rm, rv = rm0.clone(), rv0.clone()
    out = T.bn_train_fwd(x, gamma, beta, rm, rv, R.EPS, 0.1, None, False, None, None, 0, act)
    what = f"bn {P}x{C} act{act}"
    keep, w1 = _check_fwd(T, x, out, gamma, beta, None, act, 0, rows, what, (rm0, rv0, rm, rv, 0.1))
    assert P == 1 or 0.05 < float(keep.double().mean()) < 0.95
    outs = T.bn_train_bwd(g, x, gamma, out[1], out[2], True, None, True, out[3], 0, None, act)
    w2 = _check_bwd(x, g, outs, gamma, out[1], out[2], keep, 0, rows, what)
    print(f"{what} groups={R.bn_groups(P, C, T)} R={rows}: {_fmt(w1, w2)}")


# ---------------------------------------------------------------------------------------- options
OPTION_WIDTHS = [(16, 0), (16, 13), (67, 0), (72, 0), (72, 67)]


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("C,cr", OPTION_WIDTHS, ids=[f"{c}cr{r}" for c, r in OPTION_WIDTHS])
@pytest.mark.parametrize("P", [60, 200])
def test_options(cuda, P, C, cr, act, res):
    """Activation codes, residual, gamma / beta None, running statistics None, momentum 0.1 then 1.0 on the same
    buffers, num_batches + 1 per call, carried widths; the backward by the bit mask, by ym (ReLU: the same bits),
    with want_dx False (dgamma / dbeta bit-identical) and with dres."""
    from torchpruner_amd import ops
    T = ops.require()
    crr = cr or C
    x, gamma, beta, rs, g = _inputs(P, C, cr, P * 977 + C * 13 + cr + act, cuda, res=res)
    rows = R.rows_per_thread(P, C, T)
    what = f"bn {P}x{C} cr{cr} act{act}{' res' if res else ''}"
    rm0, rv0 = _running0(crr, cuda)
    rm, rv, nbt = rm0.clone(), rv0.clone(), torch.zeros((), dtype=torch.int64, device=cuda)
    out = T.bn_train_fwd(x, gamma, beta, rm, rv, R.EPS, 0.1, rs, False, None, nbt, cr, act)
    keep, w1 = _check_fwd(T, x, out, gamma, beta, rs, act, cr, rows, what, (rm0, rv0, rm, rv, 0.1))
    assert int(nbt) == 1 and rm.shape == (crr,)
    rm1, rv1 = rm.clone(), rv.clone()
    out2 = T.bn_train_fwd(x, gamma, beta, rm, rv, R.EPS, 1.0, rs, False, None, nbt, cr, act)
    _, w1b = _check_fwd(T, x, out2, gamma, beta, rs, act, cr, rows, what + " momentum 1", (rm1, rv1, rm, rv, 1.0))
    assert int(nbt) == 2
    assert all(_same_bits(a, b) for a, b in zip(out[:3], out2[:3])) and torch.equal(out[3], out2[3])
    out3 = T.bn_train_fwd(x, None, None, None, None, R.EPS, 0.1, rs, False, None, None, cr, act)
    keep3, w3 = _check_fwd(T, x, out3, None, None, rs, act, cr, rows, what + " no affine")
    assert _same_bits(out3[1], out[1]) and _same_bits(out3[2], out[2])

    mean_k, invstd_k, mk = out[1], out[2], out[3] if act else None
    outs = T.bn_train_bwd(g, x, gamma, mean_k, invstd_k, True, None, res, mk, cr, None, act)
    assert (outs[3] is not None) == res
    w2 = _check_bwd(x, g, outs, gamma, mean_k, invstd_k, keep, cr, rows, what)
    if act and res:
        assert not bool(outs[3][:, crr:].any()), "dres is not zero in the padding (mask bits are 0 there)"
    # want_dx False, with and without dres: the same dgamma / dbeta bits, the same dres bits
    for want_dres in (True, False):
        o = T.bn_train_bwd(g, x, gamma, mean_k, invstd_k, False, None, want_dres, mk, cr, None, act)
        assert o[0] is None and (o[3] is not None) == want_dres
        assert _same_bits(o[1], outs[1]) and _same_bits(o[2], outs[2])
        _check_bwd(x, g, o, gamma, mean_k, invstd_k, keep, cr, rows, what + " no dx")
    if act == 1:  # ym = the forward's y gives the mask's decisions: every output the same bits
        o = T.bn_train_bwd(g, x, gamma, mean_k, invstd_k, True, out[0], True, None, cr, None, 1)
        assert _same_bits(o[0], outs[0]) and _same_bits(o[1], outs[1]) and _same_bits(o[2], outs[2])
        _check_bwd(x, g, o, gamma, mean_k, invstd_k, keep, cr, rows, what + " ym")
    # gamma None in the backward
    o = T.bn_train_bwd(g, x, None, out3[1], out3[2], True, None, False, out3[3] if act else None, cr, None, act)
    w4 = _check_bwd(x, g, o, None, out3[1], out3[2], keep3, cr, rows, what + " no affine")
    print(f"{what}: {_fmt(w1, w1b, w2)} | no affine {_fmt(w3, w4)}")


YM_VALUES = [1.0, -1.0, 0.0, -0.0, float("nan"), 1.1754943508222875e-38]  # the last: the smallest normal fp32


@pytest.mark.parametrize("P,C", [(60, 16), (200, 16), (60, 13), (200, 67)])
def test_ym_special_values(cuda, P, C):
    """The ``ym`` masking mode at its special values, element e holding YM_VALUES[e % 6]: the gradient passes
    where ym > 0 (1 and the smallest normal) and nowhere else (-1, +0.0, -0.0, NaN); dres = g there and +0.0
    elsewhere, bit for bit, and the sums and dx follow that mask."""
    from torchpruner_amd import ops
    T = ops.require()
    x, gamma, _, _, g = _inputs(P, C, 0, P + C, cuda)
    ym = torch.tensor(YM_VALUES, device=cuda).repeat(-(-P * C // 6))[:P * C].view(P, C).contiguous()
    keep = (torch.arange(P * C, device=cuda) % 6).view(P, C)
    keep = (keep == 0) | (keep == 5)
    mean, var, invstd = R.stats(x)
    mean_k, invstd_k = mean.float(), invstd.float()
    outs = T.bn_train_bwd(g, x, gamma, mean_k, invstd_k, True, ym, True, None, 0, None, 1)
    w = _check_bwd(x, g, outs, gamma, mean_k, invstd_k, keep, 0, R.rows_per_thread(P, C, T), f"ym {P}x{C}")
    assert not bool(torch.signbit(outs[3][~keep]).any())
    print(f"ym {P}x{C}: {_fmt(w)}")


@pytest.mark.parametrize("P,C,cr", [(60, 16, 13), (200, 72, 67), (200, 67, 60)])
def test_dres_in_padding_without_a_mask(cuda, P, C, cr):
    """No activation, no mask: dres is g unchanged, padding included (g = 1.0 there comes back as 1.0), while
    dx is zero in the padding. The contract is written at tp_bn_bwd_train: callers keep g zero in the padding
    (the only caller that asks for dres without a mask, the MobileNet project BN, runs at cr == C)."""
    from torchpruner_amd import ops
    T = ops.require()
    x, gamma, beta, _, g = _inputs(P, C, cr, P + C + cr, cuda)
    out = T.bn_train_fwd(x, gamma, beta, None, None, R.EPS, 0.1, None, False, None, None, cr, 0)
    outs = T.bn_train_bwd(g, x, gamma, out[1], out[2], True, None, True, None, cr, None, 0)
    assert _same_bits(outs[3], g) and bool((outs[3][:, cr:] == 1.0).all())
    w = _check_bwd(x, g, outs, gamma, out[1], out[2], None, cr, R.rows_per_thread(P, C, T), f"dres {P}x{C} cr{cr}")
    print(f"dres {P}x{C} cr{cr}: {_fmt(w)}")


# ----------------------------------------------------------------------------------- pre launchers
def _tiles(P, G, gen):
    """Tile index of every row for an uneven partition of P rows into G non-empty contiguous tiles."""
    cuts = (torch.randperm(P - 1, generator=gen)[:G - 1] + 1).sort().values
    tid = torch.zeros(P, dtype=torch.int64)
    tid[cuts] = 1
    tid = tid.cumsum(0)
    sizes = torch.bincount(tid, minlength=G)
    assert int(tid[-1]) == G - 1 and int(sizes.min()) >= 1 and (G == 1 or G * int(sizes.max()) > P)
    return tid


def _tile_sums(tid, G, a, b):
    """(G, 2, C) fp64 sums of the rows of a and b per tile"""
    pre = torch.zeros(G, 2, a.shape[1], dtype=torch.float64, device=a.device)
    pre[:, 0].index_add_(0, tid, a)
    pre[:, 1].index_add_(0, tid, b)
    return pre.contiguous()


@pytest.mark.parametrize("C", [8, 67])
@pytest.mark.parametrize("G", [1, 5, 256, 257, 700])
def test_pre_launchers(cuda, G, C):
    """tp_bn_fwd_train_pre / tp_bn_bwd_train_pre on tile statistics built here in fp64 over an uneven partition of
    P = 2100 rows: G <= 256 folds tile by tile, G = 257 and 700 fold ``per`` = 2 and 3 tiles per group with a ragged
    last group. The sums are exact to fp64, so mean / invstd meet the statistics bound with R = 0, dgamma / dbeta
    are the fp64 total within e_fold plus the fp32 store, and y and dx meet the apply bounds."""
    from torchpruner_amd import ops
    T = ops.require()
    P = 2100
    x, gamma, beta, _, g = _inputs(P, C, 0, G * 7 + C, cuda)
    tid = _tiles(P, G, torch.Generator().manual_seed(G + C)).to(cuda)
    x64 = x.double()
    pre = _tile_sums(tid, G, x64, x64 * x64)
    rm0, rv0 = _running0(C, cuda)
    rm, rv = rm0.clone(), rv0.clone()
    out = T.bn_train_fwd(x, gamma, beta, rm, rv, R.EPS, 0.1, None, False, pre, None, 0, 1)
    what = f"pre G={G} C={C}"
    keep, w1 = _check_fwd(T, x, out, gamma, beta, None, 1, 0, 0, what, (rm0, rv0, rm, rv, 0.1))
    mean_k, invstd_k = out[1], out[2]
    gm = torch.where(keep, g, torch.zeros_like(g)).double()
    xhat = (x64 - mean_k.double()) * invstd_k.double()
    preb = _tile_sums(tid, G, gm, gm * xhat)
    es = (R.e_fold(preb[:, 0], G), R.e_fold(preb[:, 1], G))
    outs = T.bn_train_bwd(g, x, gamma, mean_k, invstd_k, True, None, True, out[3], 0, preb, 1)
    w2 = _check_bwd(x, g, outs, gamma, mean_k, invstd_k, keep, 0, 0, what, es)
    # against the totals of the very tile sums handed in
    for k, got in ((0, outs[2]), (1, outs[1])):
        tot = preb[:, k].sum(0)
        R.check((got.double() - tot).abs(), es[k] + U * tot.abs(), what + " total of the tiles")
    print(f"{what}: {_fmt(w1, w2)}")


def test_pre_from_the_conv_epilogues(cuda):
    """The real producers: conv_gen_stats (forward tile statistics of a 1x1 conv, cfg 2) into bn_train_fwd(pre=),
    conv_gen_bwd_bn (backward tile statistics of the 1x1 data gradient) into bn_train_bwd(pre=), against fp64 of
    the conv outputs the kernels returned. A thread of either epilogue adds at most RPT_MAX = 16 rows in fp32
    before the fp64 tile sum, so the statistics bounds hold with R = 16."""
    from torchpruner_amd import ops
    T = ops.require()
    B, H, W, Cin, Cout, cfg = 3, 14, 14, 64, 36, 2
    P = B * H * W
    gen = torch.Generator().manual_seed(36)
    xin = torch.randn(B, H, W, Cin, generator=gen).to(cuda)
    w = (torch.randn(Cout, Cin, generator=gen) * 0.2).to(cuda)
    gamma, beta = (torch.rand(Cout, generator=gen) + 0.5).to(cuda), torch.randn(Cout, generator=gen).to(cuda)
    y4, part = T.conv_gen_stats(xin, w, None, 1, 1, 0, cfg)
    assert part.shape == (-(-P // 64), 2, Cout) and part.dtype == torch.float64
    x = y4.view(P, Cout)
    out = T.bn_train_fwd(x, gamma, beta, None, None, R.EPS, 0.1, None, False, part, None, 0, 1)
    keep, w1 = _check_fwd(T, x, out, gamma, beta, None, 1, 0, RPT_MAX, "conv_gen_stats")
    gup = torch.randn(B, H, W, Cin, generator=gen).to(cuda)
    dxh, partb = T.conv_gen_bwd_bn(gup, w, None, 1, None, y4, out[1], out[2], out[3], cfg)
    assert partb.shape == part.shape
    g = dxh.view(P, Cout)
    bw = R.bwd_from_stats(g, x, out[1], out[2], gamma, keep)
    es = (R.e_sum(bw["abs0"], RPT_MAX), R.e_sum(bw["abs1"], RPT_MAX))
    outs = T.bn_train_bwd(g, x, gamma, out[1], out[2], True, None, True, out[3], 0, partb, 1)
    w2 = _check_bwd(x, g, outs, gamma, out[1], out[2], keep, 0, 0, "conv_gen_bwd_bn", es)
    print(f"conv epilogues: {_fmt(w1, w2)}")


# ------------------------------------------------------------------------------------ conditioning
def _rel_var(T, x):
    """Relative error of the batch variance (through running_var at momentum 1: the unbiased variance in fp32) of
    the kernel and of F.batch_norm in fp32 on the same device and input."""
    P, C = x.shape
    ref = x.double().var(0, unbiased=True)
    rm, rv = torch.zeros(C, device=x.device), torch.ones(C, device=x.device)
    T.bn_train_fwd(x, None, None, rm, rv, R.EPS, 1.0, None, False, None, None, 0, 0)
    tm, tv = torch.zeros(C, device=x.device), torch.ones(C, device=x.device)
    F.batch_norm(x, tm, tv, None, None, True, 1.0, R.EPS)
    return float(((rv.double() - ref).abs() / ref).max()), float(((tv.double() - ref).abs() / ref).max())


@pytest.mark.parametrize("P", [200, 3136])
@pytest.mark.parametrize("ratio", ["0.3333333333333333", "10", "100"], ids=["third", "10", "100"])
def test_conditioning(cuda, ratio, P):
    """x = randn + ratio (mean / std = ratio): the fp32 sums of x and x^2 lose (R + 2) u mean(x^2) / var of the
    variance, which check (a) allows and no more; check (b) is unaffected. Prints the observed relative error of the
    variance next to that of F.batch_norm in fp32 (a reference point, not asserted)."""
    from torchpruner_amd import ops
    T = ops.require()
    C = 8
    x, gamma, beta, _, g = _inputs(P, C, 0, P + 5, cuda, fam=ratio)
    rows = R.rows_per_thread(P, C, T)
    out = T.bn_train_fwd(x, gamma, beta, None, None, R.EPS, 0.1, None, False, None, None, 0, 0)
    what = f"ratio {float(ratio):.3g} P={P}"
    _, w1 = _check_fwd(T, x, out, gamma, beta, None, 0, 0, rows, what)
    outs = T.bn_train_bwd(g, x, gamma, out[1], out[2], True, None, False, None, 0, None, 0)
    w2 = _check_bwd(x, g, outs, gamma, out[1], out[2], None, 0, rows, what)
    mean, var, _ = R.stats(x)
    bound = float(((rows + 2) * U * (x.double() ** 2).mean(0) / var).max())
    ours, aten = _rel_var(T, x)
    print(f"conditioning {what} R={rows}: rel var err kernel {ours:.2e}  F.batch_norm fp32 {aten:.2e}  "
          f"bound (R+2) u mean(x^2)/var {bound:.2e} | {_fmt(w1, w2)}")


@pytest.mark.parametrize("C", [8, 13])
def test_constant_channels(cuda, C):
    """Channel 0 all zeros (every partial sum exactly 0: var = 0, invstd = 1/sqrt(eps), y = beta, dgamma = -+0),
    channel 1 all 7.0 (y = x * a + b cancels two terms of about 2200 * gamma: inside the apply bound of beta),
    P = 200; dx finite and inside its bound."""
    from torchpruner_amd import ops
    T = ops.require()
    P = 200
    x, gamma, beta, _, g = _inputs(P, C, 0, C, cuda)
    x[:, 0], x[:, 1] = 0.0, 7.0
    rows = R.rows_per_thread(P, C, T)
    out = T.bn_train_fwd(x, gamma, beta, None, None, R.EPS, 0.1, None, False, None, None, 0, 0)
    _, w1 = _check_fwd(T, x, out, gamma, beta, None, 0, 0, rows, f"const C={C}")
    assert float(out[1][0]) == 0.0 and float(out[2][0]) == float(torch.tensor(1.0 / math.sqrt(R.EPS), dtype=torch.float32))
    assert bool((out[0][:, 0] == beta[0]).all())
    outs = T.bn_train_bwd(g, x, gamma, out[1], out[2], True, None, False, None, 0, None, 0)
    w2 = _check_bwd(x, g, outs, gamma, out[1], out[2], None, 0, rows, f"const C={C}")
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[1][0]) == 0.0
    print(f"const C={C}: {_fmt(w1, w2)}")


# -------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("C", [8, 13])
def test_non_finite_input(cuda, C, bad):
    """One NaN, or one +inf, in one element of channel 2 (P = 130, two row groups): that channel's invstd, y, dx
    and running variance are NaN everywhere and its mask bits 0; its mean and running mean are NaN for the NaN
    and not finite for the +inf (the mean of a column holding +inf is +inf in any arithmetic); every other channel
    has the bits of the same call with that element replaced by 0."""
    from torchpruner_amd import ops
    T = ops.require()
    P, ch = 130, 2
    x0, gamma, beta, _, g = _inputs(P, C, 0, C + 1, cuda)
    x0[37, ch] = 0.0
    x = x0.clone()
    x[37, ch] = bad
    other = torch.arange(C, device=cuda) != ch
    res = []
    for xx in (x, x0):
        rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        y, mean, invstd, mk = T.bn_train_fwd(xx, gamma, beta, rm, rv, R.EPS, 0.1, None, False, None, None, 0, 1)
        dx, dgamma, dbeta, _ = T.bn_train_bwd(g, xx, gamma, mean, invstd, True, None, False, mk, 0, None, 1)
        res.append((y, mean, invstd, rm, rv, dx, dgamma, dbeta, _bits(mk, P, C)))
    (y, mean, invstd, rm, rv, dx, dgamma, dbeta, bits), clean = res
    only_nan = bad != bad
    for name, t in (("mean", mean), ("running_mean", rm)):
        assert bool(torch.isnan(t[ch])) if only_nan else not bool(torch.isfinite(t[ch])), f"{name}: {float(t[ch])}"
    for name, t in (("invstd", invstd), ("running_var", rv)):
        assert bool(torch.isnan(t[ch])), f"{name} of the channel is {float(t[ch])}, not NaN"
    assert bool(torch.isnan(y[:, ch]).all()) and bool(torch.isnan(dx[:, ch]).all()) and not bool(bits[:, ch].any())
    for a, b in zip(res[0][:8], clean[:8]):
        assert _same_bits(a[..., other], b[..., other])
    assert torch.equal(bits[:, other], clean[8][:, other])


# ------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("P,C", [(4481, 64), (2112, 2052)])
def test_two_calls_give_the_same_bits(cuda, P, C):
    from torchpruner_amd import ops
    T = ops.require()
    x, gamma, beta, rs, g = _inputs(P, C, 0, 3, cuda, res=True)
    runs = []
    for _ in range(2):
        rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        y, mean, invstd, mk = T.bn_train_fwd(x, gamma, beta, rm, rv, R.EPS, 0.1, rs, False, None, None, 0, 1)
        dx, dgamma, dbeta, dres = T.bn_train_bwd(g, x, gamma, mean, invstd, True, None, True, mk, 0, None, 1)
        runs.append((y, mean, invstd, rm, rv, dx, dgamma, dbeta, dres, mk))
    for a, b in zip(*runs):
        assert torch.equal(a, b) if a.dtype == torch.uint8 else _same_bits(a, b)


# ----------------------------------------------------------------- the Hardswish and SiLU unit tails
# Their statistics pass (act_partial_body) has the row walk of bn_partial. tests/test_bn_hswish_gpu.py and
# test_bn_silu_gpu.py already run P = 200 (three row groups, the last one ragged), so only the empty-group
# shape runs here, on the per-element kernels.
TAIL_SHAPE = R.TAIL_SHAPE
KINK_BAND = R.KINK_BAND  # tests/test_bn_reference.py: at most 0.5 % of the fp64 pre-activations within twice the band


def _hswish64(v):
    return v * (v + 3).clamp(0, 6) / 6


def _tail_inputs(dev):
    return tuple(t.to(dev) for t in R.tail_inputs(*TAIL_SHAPE))


def _tail_factor(kind, v, g):
    """fp64 gradient factor act'(v) at the fp64 pre-activation v, and the bound of the kernel's fp32 gm = g * act'(v_k)
    against g * act'(v), v_k = fma(x, a, b) within u |v| of v (one rounding).
    Hardswish (0 below -3, v/3 + 1/2 up to 3, 1 above): the outer branches return 0 or g exactly; inside, the error
    of v moves the factor by u |v| / 3, the division, the addition and the product by g round once each:
    4u |g| (|v|/3 + 1/2). Within KINK_BAND of a kink the kernel may take the other branch, a jump of at most 1/2
    plus the above: 1.5 |g| there (those elements are excluded, not bounded tightly).
    SiLU, s (1 + v (1 - s)) with s = 1 / (1 + expf(-v)): s is within 4u s (expf 2 ulp, one addition, one correctly
    rounded division); 1 - s within 4u; v (1 - s) within 5u |v|; 1 + v (1 - s) within 6u (1 + |v|); the product
    with s within 11u (1 + |v|); the error of v moves the factor (slope at most 1/2) by u |v| / 2; the product by g
    rounds once: 12u |g| (1 + |v|), rounded up to 13 for the second order."""
    if kind == "hswish":
        f = torch.where(v < -3, torch.zeros_like(v), torch.where(v <= 3, v / 3 + 0.5, torch.ones_like(v)))
        inside = (v > -3) & (v < 3)
        e = torch.where(inside, 4 * U * g.abs() * (v.abs() / 3 + 0.5), torch.zeros_like(v))
        near = ((v + 3).abs() <= KINK_BAND) | ((v - 3).abs() <= KINK_BAND)
        return f, torch.where(near, 1.5 * g.abs(), e), near
    s = torch.sigmoid(v)
    return s * (1 + v * (1 - s)), 13 * U * g.abs() * (1 + v.abs()), torch.zeros_like(v, dtype=torch.bool)


def _tail_y(kind, v):
    """fp64 y = act(v) and the bound of the kernel's fp32 y at v_k within u |v| of v.
    Hardswish, v * t / 6 with t = clamp(v + 3, 0, 6): t is within u |v| + u |v + 3|, so v * t within
    u |v| (t + |v| + |v + 3|), and the product and the division round once each, 2u |y|; 3u |y| with the second order.
    SiLU, v * s: s within 4u s + u |v| / 4 (its slope is at most 1/4), so y within u |y| (v) + 4u |y| + u v^2 / 4
    + u |y| (the product): 6u |y| + u v^2 / 4; 7u |y| with the second order."""
    if kind == "hswish":
        y = _hswish64(v)
        return y, U * v.abs() * ((v + 3).clamp(0, 6) + v.abs() + (v + 3).abs()) / 6 + 3 * U * y.abs()
    y = v * torch.sigmoid(v)
    return y, 7 * U * y.abs() + 0.25 * U * v * v


@pytest.mark.parametrize("kind", ["hswish", "silu"])
def test_unit_tails_with_an_empty_group(cuda, kind):
    """bn_hswish_fwd/bwd and bn_silu_fwd/bwd at (4481, 13): 70 row groups, the last one empty. The split check,
    with the fp64 pre-activation recomputed from the returned ``ab`` and the fp64 derivative at it."""
    from torchpruner_amd import ops
    T = ops.require()
    P, C = TAIL_SHAPE
    x, gamma, beta, g = _tail_inputs(cuda)
    rows = R.rows_per_thread(P, C, T)
    fwd, bwd = (T.bn_hswish_fwd, T.bn_hswish_bwd) if kind == "hswish" else (T.bn_silu_fwd, T.bn_silu_bwd)
    rm0, rv0 = _running0(C, cuda)
    rm, rv, nbt = rm0.clone(), rv0.clone(), torch.zeros((), dtype=torch.int64, device=cuda)
    y, mean_k, invstd_k, ab = fwd(x, gamma, beta, rm, rv, R.EPS, 0.1, nbt, 0)
    assert int(nbt) == 1 and ab.shape == (2, C)
    what = f"bn_{kind} {P}x{C}"
    # (a), and the folded affine against the plain forward's bound on (a, b): one and three roundings
    mean, var, em, ev = R.check_stats(x, mean_k, invstd_k, rows, what=what)
    rrm, rrv, vstat = R.running(rm0, rv0, mean, var, P, 0.1)
    R.check((rm.double() - rrm).abs(), R.e_running(em, 0.1, rm0, rrm), what + " running_mean")
    R.check((rv.double() - rrv).abs(), R.e_running(ev * P / (P - 1) + U * vstat.abs(), 0.1, rv0, rrv), what + " running_var")
    fw = R.fwd_from_stats(x, mean_k, invstd_k, gamma, beta)
    R.check((ab[0].double() - fw["a"]).abs(), U * fw["a"].abs(), what + " a")
    R.check((ab[1].double() - fw["b"]).abs(), 3 * U * fw["bmag"], what + " b")
    # (b) from the returned ab
    v = x.double() * ab[0].double() + ab[1].double()
    yref, ey = _tail_y(kind, v)
    f, e_gm, near = _tail_factor(kind, v, g.double())
    assert float(near.double().mean()) <= 0.005
    wy = R.check((y.double() - yref).abs()[~near], ey[~near], what + " y")
    dx, dgamma, dbeta = bwd(g, x, gamma, mean_k, invstd_k, ab, True, 0)
    bw = R.bwd_from_stats(None, x, mean_k, invstd_k, gamma, gm=g.double() * f)
    e0 = R.e_sum(bw["abs0"], rows, e_gm.sum(0))
    e1 = R.e_sum(bw["abs1"], rows, (e_gm * bw["xhat"].abs()).sum(0))
    w = {"y": wy, "dbeta": R.check((dbeta.double() - bw["dbeta"]).abs(), e0, what + " dbeta"),
         "dgamma": R.check((dgamma.double() - bw["dgamma"]).abs(), e1, what + " dgamma"),
         "dx": R.check((dx.double() - bw["dx"]).abs(), R.e_dx(x, bw, P, e0, e1, e_gm), what + " dx")}
    o = bwd(g, x, gamma, mean_k, invstd_k, ab, False, 0)
    assert o[0] is None and _same_bits(o[1], dgamma) and _same_bits(o[2], dbeta)
    print(f"{what}: {_fmt(w)}")
