"""The forward and data-gradient convs held to EQUALITY with fp64 on integer operands: the stride-1 implicit GEMM
(conv_fwd / conv_dgrad), the general / strided / transposed kernel (conv_gen / conv_gen_bwd) and Winograd F(2x2)
(conv_wino_fwd / conv_wino_dgrad), on every tile config 0..6, at shapes chosen for their partial tiles, with split
counts that leave the last K range shorter or are clamped; and F(4x4) (wino4.hip), which cannot be exact, held per
element to the a-priori bound ``wino4_bound``. References, operand generators and case tables are in
tests/test_conv_exact_math.py, which asserts on the CPU that with these operands every intermediate of a correct
kernel is an integer below 2^24 (an exact fp32 number) and that every reference survives float32: so ``torch.equal``
is the whole comparison, for outputs, APoZ counts, pool maxima, argmax bytes and Taylor sums alike.

What each equality rules out (every non-zero operand has magnitude >= 1, every product is an integer):
- one term of one output element dropped, doubled or taken from a neighbouring pixel / channel / K slice: that
  element moves by an integer >= 1 unless the term is 0, and among the hundreds of terms per element and thousands
  of elements per case almost all are not;
- one pixel counted for the wrong image in an APoZ count or a Taylor sum: two (image, channel) entries move by a
  count of 1 or by the pixel's integer term, and B = 3, 5 and 7 with tiles straddling images put such pixels in
  every cfg's tile;
- a last partial tile writing one row or quad too many or too few: a missing row leaves the output buffer's fill in
  place of an integer result; an extra row lands in the next rows of the same tensor, which are compared too, or
  past its end, which the split workspaces and the neighbouring allocations make visible in the other outputs of
  the same test (the counts and sums read the same rows); the N edges 12, 36 and 132 put the last quad inside a
  32-column wave tile.

The F(2x2) U images are not compared with G w G^T on their own: their XOR-arranged LDS layout is described in
winograd.hip only in prose, so the end-to-end equality stands for them.

F(4x4) has no exact case: G holds 1/6, 1/12 and 1/24, so even a centre-tap-only integer weight gives inexact U
(test_conv_exact_math.py::test_wino4_centre_tap_is_not_exact). Every element is held to ``wino4_bound`` instead,
(C + 15) roundings counted from the kernel's transform code, and nothing is skipped at the ReLU: max(., 0) and the
pool maximum are 1-Lipschitz, so a zeroed output obeys its pre-activation's bound (share skipped: 0)."""
import pytest
import torch

from test_conv_exact_math import (CFGS, GEN_BWD_CASES, GEN_FWD_CASES, IGEMM_SHAPES, IGEMM_SPLITS, LINEAR_SHAPES, SLOPE,
                                  WINO2_EVEN, WINO2_ODD, WINO4_BAND, WINO4_SHAPES, case_id, gen_bwd_case,
                                  gen_fwd_case, gen_w, gen_wt, igemm_bwd_case, igemm_fwd_case, igemm_w, igemm_wt,
                                  ref_apoz, ref_bwd_out, ref_dgrad, ref_fwd, ref_pool, ref_taylor, res_scatter,
                                  taylor_bound, unpool, wino2_bwd_case, wino2_fwd_case, wino4_bwd_case,
                                  wino4_fwd_case)

pytestmark = pytest.mark.gpu

FILL = 5.0  # the padding columns of a GEN weight operand: the kernels read zeros past Cin on the activation side


def _ops():
    from torchpruner_amd import ops
    return ops.require()


def _eq(got, ref, what):
    """got (a GPU fp32 / uint8 tensor) == ref (fp64 on the CPU), every element."""
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, (what, tuple(g.shape), tuple(ref.shape))
    if not torch.equal(g, ref.double()):
        bad = (g != ref.double()).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at {i}: "
                             f"got {g[i].item()} want {ref.double()[i].item()}")


def _dev(cuda, *ts):
    return [t.to(cuda) if t is not None else None for t in ts]


def _check_pooled(y, am, pre, what):
    best, arg, ok = ref_pool(pre)
    _eq(y, best, what + " pooled")
    assert int(am.max()) <= 3
    assert torch.equal(am.cpu()[ok], arg[ok]), what + " argmax"


# ================================================================== 2. the stride-1 implicit GEMM (conv_mfma.hip)
@pytest.mark.parametrize("shape", IGEMM_SHAPES, ids=case_id)
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("splits", IGEMM_SPLITS)
def test_igemm_fwd_exact(cuda, shape, cfg, splits):
    """conv_fwd, 3x3: out, APoZ counts, pooled out and argmax bytes (pooled M order) == fp64, ReLU on and off, and
    LeakyReLU slope 0.25. splits = 4 on the three-slice shape leaves the last K range shorter (27 slices: 7, 7, 7,
    6); 1000 is clamped to one slice per split."""
    T = _ops()
    B, H, W, Cin, Cout = shape
    x, w, sc, sh = igemm_fwd_case(shape, 3)
    xd, wd, scd, shd = _dev(cuda, x, igemm_w(w), sc, sh)
    n = 0
    for relu in (False, True):
        pre = ref_fwd(x, w, sc, sh, None, relu)
        cnt = ref_apoz(pre)
        what = f"conv_fwd {case_id(shape)} cfg={cfg} splits={splits} relu={relu}"
        ap = torch.zeros(B, Cout, device=cuda)
        out, _ = T.conv_fwd(xd, wd, scd, shd, relu, False, 3, cfg, splits, ap)
        _eq(out, pre, what)
        _eq(ap, cnt, what + " apoz")
        ap = torch.zeros(B, Cout, device=cuda)
        yp, am = T.conv_fwd(xd, wd, scd, shd, relu, True, 3, cfg, splits, ap)
        _check_pooled(yp, am, pre, what)
        _eq(ap, cnt, what + " pooled apoz")
        n += 2
    out, _ = T.conv_fwd(xd, wd, scd, shd, True, False, 3, cfg, splits, None, SLOPE)
    _eq(out, ref_fwd(x, w, sc, sh, None, True, SLOPE), "conv_fwd slope")
    # no scale / shift operands: the epilogue's defaults 1 and 0
    out, _ = T.conv_fwd(xd, wd, None, None, False, False, 3, cfg, splits)
    _eq(out, ref_fwd(x, w), "conv_fwd raw")
    print(f"conv exact igemm fwd {case_id(shape)} cfg={cfg} splits={splits}: {n + 2} launches all equal")


@pytest.mark.parametrize("bkn", LINEAR_SHAPES, ids=case_id)
@pytest.mark.parametrize("cfg", CFGS)
def test_linear_fwd_exact(cuda, bkn, cfg):
    """ks = 1 as a linear layer: N = 12 (no multiple of 32, three quads) and 132 (one quad past a 128 tile)."""
    T = _ops()
    Bn, K, N = bkn
    shape = (Bn, 1, 1, K, N)
    x, w, sc, sh = igemm_fwd_case(shape, 1)
    xd, wd, scd, shd = _dev(cuda, x, igemm_w(w), sc, sh)
    for splits in (1, 2, 1000):
        for relu in (False, True):
            pre = ref_fwd(x, w, sc, sh, None, relu)
            ap = torch.zeros(Bn, N, device=cuda)
            out, _ = T.conv_fwd(xd, wd, scd, shd, relu, False, 1, cfg, splits, ap)
            _eq(out, pre, f"linear {case_id(bkn)} cfg={cfg} splits={splits} relu={relu}")
            _eq(ap, ref_apoz(pre), "linear apoz")
    print(f"conv exact igemm linear {case_id(bkn)} cfg={cfg}: 6 launches all equal")


def _tay_slab(ref_t, group):
    """(B, N) reference sums in the (N / group, B, group) layout conv_dgrad's tay_group documents."""
    if not group:
        return ref_t
    B, N = ref_t.shape
    return ref_t.view(B, N // group, group).permute(1, 0, 2).contiguous()


def _igemm_dgrad(T, cuda, shape, ks, cfg, splits):
    B, H, W, Cin, Cout = shape
    g, wf, act, sc, gp, am = igemm_bwd_case(shape, ks)
    wtd, actd, scd = _dev(cuda, igemm_wt(wf), act, sc)
    n = 0
    for pooled in ((False, True) if gp is not None else (False,)):
        gfull = unpool(gp, am) if pooled else g
        gd, amd = _dev(cuda, gp if pooled else g, am if pooled else None)
        dx = ref_dgrad(gfull, wf, (H, W))
        what = f"conv_dgrad {case_id(shape)} ks={ks} cfg={cfg} splits={splits} unpool={pooled}"
        half = Cout // 2  # a non-default tay_group: any divisor of the output width (two slots of Cout / 2 columns)
        for mode, group, want_out, slope in ((0, 0, True, 0.0), (1, 0, True, 0.0), (0, half, True, 0.0),
                                             (1, half, False, 0.0), (0, 0, False, 0.0), (1, 0, True, SLOPE)):
            tay = torch.zeros(B, Cout, device=cuda)
            out = T.conv_dgrad(gd, amd, wtd, actd, scd, tay, want_out, ks, cfg, splits, group, mode, slope)
            w2 = f"{what} mode={mode} group={group} out={want_out} slope={slope}"
            if want_out:
                _eq(out, ref_bwd_out(dx, act, sc, slope), w2)
            _eq(tay.view(-1), _tay_slab(ref_taylor(dx, act, mode), group).reshape(-1), w2 + " taylor")
            n += 1
        # no Taylor slab, no bn_scale; and a second call returns the same bits
        o1 = T.conv_dgrad(gd, amd, wtd, actd, None, None, True, ks, cfg, splits)
        o2 = T.conv_dgrad(gd, amd, wtd, actd, None, None, True, ks, cfg, splits)
        _eq(o1, ref_bwd_out(dx, act, torch.ones(Cout)), what + " unscaled")
        assert torch.equal(o1, o2)
        n += 2
    return n


@pytest.mark.parametrize("shape", IGEMM_SHAPES, ids=case_id)
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("splits", IGEMM_SPLITS)
def test_igemm_dgrad_exact(cuda, shape, cfg, splits):
    """conv_dgrad, 3x3, with and without the fused unpool: the masked / scaled gradient and the Taylor (mode 0) and
    Sensitivity (mode 1) sums == fp64, tay_group 0 and Cout / 2, want_out both ways, LeakyReLU slope. The gradient
    has the shape's Cin channels (the K side), the output its Cout (the N side)."""
    n = _igemm_dgrad(_ops(), cuda, shape, 3, cfg, splits)
    print(f"conv exact igemm dgrad {case_id(shape)} cfg={cfg} splits={splits}: {n} launches all equal")


@pytest.mark.parametrize("bkn", LINEAR_SHAPES, ids=case_id)
@pytest.mark.parametrize("cfg", CFGS)
def test_linear_dgrad_exact(cuda, bkn, cfg):
    n = 0
    for splits in (1, 2, 1000):
        n += _igemm_dgrad(_ops(), cuda, (bkn[0], 1, 1, bkn[1], bkn[2]), 1, cfg, splits)
    print(f"conv exact igemm linear dgrad {case_id(bkn)} cfg={cfg}: {n} launches all equal")


# ============================================================================= 3. conv_gen and conv_gen_bwd
@pytest.mark.parametrize("case", GEN_FWD_CASES, ids=case_id)
@pytest.mark.parametrize("cfg", CFGS)
def test_gen_fwd_exact(cuda, case, cfg):
    """conv_gen: out and APoZ counts == fp64, with and without the residual, ReLU both ways, one K pass and three
    (the launcher combines split slabs for APoZ too; only Taylor partials need one pass). The weight operand's
    padding columns hold 5, not 0: conv_mfma.hip documents that the last slice of a tap is zero-filled past Cin in
    the activation loads, so the result must not depend on them."""
    T = _ops()
    H, W, Cin, Cout, ks, stride, pad = case
    x, w, sc, sh, res = gen_fwd_case(case)
    wk = gen_w(w, FILL)
    assert wk.shape[1] == T.conv_gen_k(ks, Cin)
    xd, wd, scd, shd, resd = _dev(cuda, x, wk, sc, sh, res)
    n = 0
    for splits in (1, 3):
        for with_res in (False, True):
            for relu in (False, True):
                ref = ref_fwd(x, w, sc, sh, res if with_res else None, relu, 0.0, stride, pad)
                ap = torch.zeros(3, Cout, device=cuda)
                out = T.conv_gen(xd, wd, scd, shd, relu, resd if with_res else None, ap, ks, stride, pad, cfg, splits)
                what = f"conv_gen {case_id(case)} cfg={cfg} splits={splits} res={with_res} relu={relu}"
                _eq(out, ref, what)
                _eq(ap, ref_apoz(ref), what + " apoz")
                n += 1
    print(f"conv exact gen fwd {case_id(case)} cfg={cfg}: {n} launches all equal")


@pytest.mark.parametrize("case", GEN_BWD_CASES, ids=case_id)
@pytest.mark.parametrize("cfg", CFGS)
def test_gen_bwd_exact(cuda, case, cfg):
    """conv_gen_bwd: transposed 3x3 / 1x1 stride 2 at even and odd sizes, stride-1 1x1 and flipped 3x3; residual
    dense and stride-2 scattered, mask on and off; three K passes on the stride-1 kernels. Taylor partials in both
    modes wherever the binding takes them (a mask, a 1x1 stride-1 or an even-sized transposed 3x3 stride-2 dgrad,
    conv_gen_tay_slots > 0): the slot sum == fp64, and every slot has one writer that stores (a slab pre-filled with
    1000 comes back with each slot either equal to the zero-filled run's or still 1000 where that run left 0)."""
    T = _ops()
    ih, iw, C, N, ks, stride, transposed = case
    pad = ks // 2
    g, wf, res1, res2, mask = gen_bwd_case(case)
    dx = ref_dgrad(g, wf, (ih, iw), stride)
    gd, wtd, r1d, r2d, md = _dev(cuda, g, gen_wt(wf, transposed, FILL), res1, res2, mask)
    t3 = transposed and ks == 3 and stride == 2 and ih % 2 == 0 and iw % 2 == 0
    R = 4 * T.conv_gen_tay_slots(cfg, ih * iw // 4) if t3 else T.conv_gen_tay_slots(cfg, ih * iw)
    tay_ok = ((not transposed and ks == 1) or t3) and R > 0
    n = 0
    for rs, resd, full in ((0, None, 0.0), (1, r1d, res1.double()), (2, r2d, res_scatter(res2, ih, iw, 2))):
        for with_mask in (False, True):
            ref = dx + full
            if with_mask:
                ref = torch.where(mask.double() > 0, ref, torch.zeros((), dtype=torch.float64))
            what = f"conv_gen_bwd {case_id(case)} cfg={cfg} res_stride={rs} mask={with_mask}"
            for splits in ((1,) if transposed else (1, 3)):
                out = T.conv_gen_bwd(gd, wtd, resd, max(rs, 1), md if with_mask else None, ks, stride, pad, ih, iw,
                                     transposed, cfg, splits)
                _eq(out, ref, f"{what} splits={splits}")
                n += 1
            if not (with_mask and tay_ok):
                continue
            for mode in (0, 1):
                want = (-(ref * mask.double()) if mode == 0 else ref.abs()).sum((1, 2))
                t0 = torch.zeros(R, 3, N, device=cuda)
                out = T.conv_gen_bwd(gd, wtd, resd, max(rs, 1), md, ks, stride, pad, ih, iw, transposed, cfg, 1, t0,
                                     mode)
                _eq(out, ref, f"{what} with partials")
                _eq(t0.sum(0), want, f"{what} partials mode={mode}")
                t1 = torch.full((R, 3, N), 1000.0, device=cuda)
                T.conv_gen_bwd(gd, wtd, resd, max(rs, 1), md, ks, stride, pad, ih, iw, transposed, cfg, 1, t1, mode)
                assert bool(((t1 == t0) | ((t1 == 1000.0) & (t0 == 0.0))).all()), what + " slot owners"
                n += 2
    print(f"conv exact gen bwd {case_id(case)} cfg={cfg}: {n} launches all equal"
          f"{'' if tay_ok else ' (no Taylor partials for this case / cfg)'}")


# ================================================================================== 4. F(2x2) (winograd.hip)
def _staged_modes(T, H, W, unpool=False):
    """Odd maps run direct loads whatever ``staged`` says: one run. Even maps: both, the staged one taking the
    LDS-staged region where wino_staged_ok allows it and the row-span image or direct loads elsewhere."""
    return (False,) if (H % 2 or W % 2) else (False, True)


@pytest.mark.parametrize("shape", WINO2_ODD + WINO2_EVEN, ids=case_id)
@pytest.mark.parametrize("splits", [1, 3])
def test_wino2_fwd_exact(cuda, shape, splits):
    """conv_wino_fwd on multiples-of-4 weights: out, APoZ counts, pooled out and argmax bytes == fp64, direct and
    staged input paths, one channel pass and three (64 channels: chunks 3 + 3 + 2, the last range shorter)."""
    T = _ops()
    B, H, W, Cin, Cout = shape
    x, w, sc, sh = wino2_fwd_case(shape)
    xd, scd, shd = _dev(cuda, x, sc, sh)
    u = T.wino_weights(w.to(cuda), False)
    n = 0
    for staged in _staged_modes(T, H, W):
        for relu in (False, True):
            pre = ref_fwd(x, w, sc, sh, None, relu)
            what = f"conv_wino_fwd {case_id(shape)} splits={splits} staged={staged} relu={relu}"
            ap = torch.zeros(B, Cout, device=cuda)
            out, _ = T.conv_wino_fwd(xd, u, scd, shd, relu, False, splits, staged, ap)
            _eq(out, pre, what)
            _eq(ap, ref_apoz(pre), what + " apoz")
            n += 1
            if H % 2 == 0 and W % 2 == 0:
                ap = torch.zeros(B, Cout, device=cuda)
                yp, am = T.conv_wino_fwd(xd, u, scd, shd, relu, True, splits, staged, ap)
                _check_pooled(yp, am, pre, what)
                _eq(ap, ref_apoz(pre), what + " pooled apoz")
                n += 1
    print(f"conv exact wino2 fwd {case_id(shape)} splits={splits} staged_ok={bool(T.wino_staged_ok(H, W, False))}: "
          f"{n} launches all equal")


@pytest.mark.parametrize("shape", WINO2_ODD + WINO2_EVEN, ids=case_id)
@pytest.mark.parametrize("splits", [1, 3])
def test_wino2_dgrad_exact(cuda, shape, splits):
    """conv_wino_dgrad: the masked / scaled gradient and the partial slots' sum (Taylor and Sensitivity) == fp64,
    with and without the fused unpool, direct and staged; a second call returns the same slots bit for bit."""
    T = _ops()
    B, H, W, Cin, Cout = shape
    g, wf, act, sc, gp, am = wino2_bwd_case(shape)
    ut = T.wino_weights(wf.flip(2, 3).transpose(0, 1).contiguous().to(cuda), False)
    actd, scd = _dev(cuda, act, sc)
    R = T.wino_taylor_slots(H, W)
    n = 0
    for pooled in ((False, True) if gp is not None else (False,)):
        gfull = unpool(gp, am) if pooled else g
        gd, amd = _dev(cuda, gp if pooled else g, am if pooled else None)
        dx = ref_dgrad(gfull, wf, (H, W))
        for staged in _staged_modes(T, H, W, pooled):
            what = f"conv_wino_dgrad {case_id(shape)} splits={splits} unpool={pooled} staged={staged}"
            for mode, want_out in ((0, True), (1, True), (0, False)):
                tay = torch.zeros(R, B, Cout, device=cuda)
                out = T.conv_wino_dgrad(gd, amd, ut, actd, scd, tay, want_out, splits, staged, mode)
                if want_out:
                    _eq(out, ref_bwd_out(dx, act, sc), f"{what} mode={mode}")
                _eq(tay.sum(0), ref_taylor(dx, act, mode), f"{what} mode={mode} out={want_out} partials")
                n += 1
            tay2 = torch.zeros(R, B, Cout, device=cuda)
            T.conv_wino_dgrad(gd, amd, ut, actd, scd, tay2, False, splits, staged, 0)
            assert torch.equal(tay, tay2), what + " second call"
            n += 1
    print(f"conv exact wino2 dgrad {case_id(shape)} splits={splits}: {n} launches all equal")


# ========================================================================= 5. F(4x4) (wino4.hip), per element
def _bounded(got, ref, E, what):
    """|got - ref| <= E for every element, exactly 0 where E is 0; returns the worst err / E."""
    err = (got.detach().cpu().double() - ref).abs()
    zero = E == 0
    assert bool((err[zero] == 0).all()), what + ": not exactly 0 where the bound is 0"
    ratio = float((err[~zero] / E[~zero]).max()) if bool((~zero).any()) else 0.0
    assert ratio <= 1.0, f"{what}: worst err / E {ratio:.3f}"
    return ratio


def _pool4(t):
    B, H, W, C = t.shape
    return t.unfold(1, 2, 2).unfold(2, 2, 2).reshape(B, H // 2, W // 2, C, 4).max(-1).values


@pytest.mark.parametrize("shape,variant", [(s, v) for s in WINO4_SHAPES for v in (0, 3)] + [(WINO4_BAND, 3)],
                         ids=lambda v: case_id(v) if isinstance(v, tuple) else f"v{v}")
def test_wino4_fwd_bounded(cuda, shape, variant):
    """conv_wino4_fwd on randn operands: every element within wino4_bound of fp64, ReLU on and off, plain and
    pooled (the band geometry has no pooled kernel), pruned output widths (ko) included. Nothing is skipped at the
    ReLU (1-Lipschitz); a pooled element is held to the largest bound of its window."""
    T = _ops()
    S, C, K, B, ko = shape
    x, w, sc, sh, ref, E = wino4_fwd_case(shape)
    xd, scd, shd = _dev(cuda, x, sc, sh)
    u = T.wino4_weights(w.to(cuda), False, K, C)
    worst = 0.0
    for relu in (False, True):
        r = torch.relu(ref) if relu else ref
        out, _ = T.conv_wino4_fwd(xd, u, scd, shd, relu, False, None, 1, variant, ko)
        worst = max(worst, _bounded(out, r, E, f"wino4 fwd {case_id(shape)} v={variant} relu={relu}"))
        if S % 2 == 0:
            yp, _ = T.conv_wino4_fwd(xd, u, scd, shd, relu, True, None, 1, variant, ko)
            worst = max(worst, _bounded(yp, _pool4(r), _pool4(E), f"wino4 pooled {case_id(shape)} v={variant}"))
    print(f"conv exact wino4 fwd {case_id(shape)} variant={variant}: worst err / E {worst:.4f} (skipped 0)")


def _wino4_dgrad(T, cuda, shape, variant, mode, fused_unpool):
    S, C, K, B, ko = shape
    kw = ko or K
    g, wf, act, sc, am, dx, E = wino4_bwd_case(shape)
    gd, actd, scd, amd = _dev(cuda, g, act, sc, am)
    ut = T.wino4_weights(wf.to(cuda), True, K, C)
    R = T.wino4_taylor_slots(S)
    tay = torch.zeros(R, B, kw, device=cuda)
    out = T.conv_wino4_dgrad(gd, ut, actd, scd, tay, True, mode, 1, variant, amd if fused_unpool else None)
    live = act.double() > 0
    zero = torch.zeros((), dtype=torch.float64)
    ref_out = torch.where(live, dx * sc.double(), zero)
    E_out = torch.where(live, E * sc.double(), zero)  # masked elements: the bound is 0, the output exactly 0
    what = f"wino4 dgrad {case_id(shape)} v={variant} mode={mode} unpool={fused_unpool}"
    if fused_unpool:
        ref_out, E_out = unpool(ref_out, am), unpool(E_out, am)
    worst = _bounded(out, ref_out, E_out, what)
    worst_t = _bounded(tay.double().sum(0), ref_taylor(dx, act, mode), taylor_bound(E, dx, act, mode),
                       what + " partials")
    print(f"conv exact {what}: worst err / E out {worst:.4f} partials {worst_t:.4f}")


@pytest.mark.parametrize("shape", WINO4_SHAPES, ids=case_id)
@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("fused_unpool", [False, True])
def test_wino4_dgrad_bounded(cuda, shape, variant, mode, fused_unpool):
    """conv_wino4_dgrad: the masked / scaled gradient (plain and written through the fused unpool) per element within
    the bound, exactly 0 where the activation is not positive and at a window's three other positions; the partial
    slots' sum (Taylor, Sensitivity, masked Sensitivity) within ``taylor_bound``."""
    _wino4_dgrad(_ops(), cuda, shape, variant, mode, fused_unpool)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_wino4_band_dgrad_bounded(cuda, mode):
    _wino4_dgrad(_ops(), cuda, WINO4_BAND, 3, mode, False)
