"""Every specialisation of the F(4x4) epilogue (csrc/kernels/wino4.hip, ``epi_phase2``) on the
block shapes it distinguishes: forward with / without ReLU and APoZ counts, pooled forward, and the
data gradient with Taylor / Sensitivity / masked-Sensitivity partials, with / without the masked
output and the fused unpooling — against fp64 references (tolerances of test_wino4_gpu.py), plus the
exact properties the specialisations must keep: a call without the partial-sum buffer returns the
same bits, repeated calls are bitwise equal, masked and non-argmax outputs are exactly 0, NaNs
propagate, and Taylor slots a shape does not use stay 0."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (S, C, K, B, ko): two half-image blocks (both Taylor slots); two images; two images per block with
# a half-empty last block; eight images per block, ragged; one tile per image with a second block
# of one tile; pruned widths ko < K
SHAPES = [(32, 8, 32, 1, 0), (32, 16, 64, 2, 0), (16, 8, 64, 3, 0), (8, 16, 32, 5, 0), (4, 8, 32, 33, 0),
          (16, 8, 64, 3, 36), (16, 8, 64, 3, 60)]
BAND = (7, 8, 32, 3, 0)
VARIANTS = [0, 3]
TOL = 2e-5


def _ops():
    from torchpruner_amd import ops
    return ops.require()


def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


@functools.lru_cache(maxsize=None)
def _fwd_case(S, C, K, B, ko):
    """Forward operands and fp64 references (pre-activation), computed once per shape."""
    T = _ops()
    dev = torch.device("cuda")
    kw = ko or K
    g = torch.Generator(device=dev).manual_seed(S * 1000 + C + K + B + ko)
    x = torch.randn(B, S, S, C, device=dev, generator=g)
    w = torch.randn(kw, C, 3, 3, device=dev, generator=g) / (3 * C ** 0.5)
    sc = torch.rand(kw, device=dev, generator=g) + 0.5
    sh = torch.randn(kw, device=dev, generator=g) * 0.1
    u = T.wino4_weights(w, False, K, C)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1)
    y = (y * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    return x, w, sc, sh, u, y


@functools.lru_cache(maxsize=None)
def _bwd_case(S, C, K, B, ko):
    """Data-gradient operands (conv Cin = K -> Cout = C) and the fp64 input gradient."""
    T = _ops()
    dev = torch.device("cuda")
    kw = ko or K
    g = torch.Generator(device=dev).manual_seed(S * 7 + C * 3 + K + B + ko)
    w = torch.randn(C, kw, 3, 3, device=dev, generator=g) / (3 * kw ** 0.5)
    go = torch.randn(B, S, S, C, device=dev, generator=g)
    act = torch.relu(torch.randn(B, S, S, kw, device=dev, generator=g))
    sc = torch.rand(kw, device=dev, generator=g) + 0.5
    am = torch.randint(0, 4, (B, S, S, kw), device=dev, generator=g, dtype=torch.uint8)
    ut = T.wino4_weights(w, True, K, C)
    dx = torch.nn.grad.conv2d_input((B, kw, S, S), w.double(), go.double().permute(0, 3, 1, 2), padding=1)
    return w, go, act, sc, am, ut, dx.permute(0, 2, 3, 1)


def _unpool(v, am):
    """v (B, S, S, K) placed at its argmax position of each 2x2 window, exact zeros elsewhere."""
    B, S, _, K = v.shape
    out = torch.zeros(B, 2 * S, 2 * S, K, device=v.device, dtype=v.dtype)
    for w in range(4):
        out[:, (w >> 1)::2, (w & 1)::2, :] = torch.where(am == w, v, torch.zeros((), device=v.device, dtype=v.dtype))
    return out


@pytest.mark.parametrize("S,C,K,B,ko", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("relu", [True, False])
def test_forward_specialisations(cuda, S, C, K, B, ko, variant, relu):
    T = _ops()
    x, w, sc, sh, u, y64 = _fwd_case(S, C, K, B, ko)
    kw = ko or K
    ref = torch.relu(y64) if relu else y64
    cnt = (ref > 0).sum((1, 2)).float()
    apoz_tol = max(2.0, 1e-3 * S * S)
    # plain epilogue, with and without the APoZ buffer
    a1, a2 = torch.zeros(B, kw, device=cuda), torch.zeros(B, kw, device=cuda)
    y_a, _ = T.conv_wino4_fwd(x, u, sc, sh, relu, False, a1, 1, variant, ko)
    y_n, _ = T.conv_wino4_fwd(x, u, sc, sh, relu, False, None, 1, variant, ko)
    y_b, _ = T.conv_wino4_fwd(x, u, sc, sh, relu, False, a2, 1, variant, ko)
    err = _rel(y_a, ref)
    print(f"fwd S={S} ko={ko} v={variant} relu={relu}: err {err:.2e} apoz {(a1 - cnt).abs().max().item()}")
    assert err < TOL, err
    assert (a1 - cnt).abs().max().item() <= apoz_tol
    assert torch.equal(y_a, y_n) and torch.equal(y_a, y_b) and torch.equal(a1, a2)
    if relu:
        assert (y_a >= 0).all()
    # pooled epilogue
    p1, p2 = torch.zeros(B, kw, device=cuda), torch.zeros(B, kw, device=cuda)
    yp_a, am_a = T.conv_wino4_fwd(x, u, sc, sh, relu, True, p1, 1, variant, ko)
    yp_n, am_n = T.conv_wino4_fwd(x, u, sc, sh, relu, True, None, 1, variant, ko)
    yp_b, am_b = T.conv_wino4_fwd(x, u, sc, sh, relu, True, p2, 1, variant, ko)
    r4 = ref.permute(0, 3, 1, 2)
    pooled, idx = F.max_pool2d(r4, 2, return_indices=True)
    pooled = pooled.permute(0, 2, 3, 1)
    errp = _rel(yp_a, pooled)
    assert errp < TOL, errp
    assert (p1 - cnt).abs().max().item() <= apoz_tol
    assert torch.equal(yp_a, yp_n) and torch.equal(am_a, am_n)
    assert torch.equal(yp_a, yp_b) and torch.equal(am_a, am_b) and torch.equal(p1, p2)
    # the pooled values are the window maxima of the plain epilogue's own outputs, bit for bit
    assert torch.equal(yp_a, F.max_pool2d(y_a.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    # argmax byte = (dy << 1) | dx of the window, where the fp64 maximum is clear
    ii = idx.permute(0, 2, 3, 1)
    want = (((ii // S) % 2) * 2 + (ii % S) % 2).to(torch.uint8)
    top2 = r4.unfold(2, 2, 2).unfold(3, 2, 2).reshape(B, kw, S // 2, S // 2, 4).sort(-1).values
    clear = ((top2[..., 3] - top2[..., 2]) > 1e-4 * pooled.abs().max()).permute(0, 2, 3, 1)
    assert (am_a <= 3).all()
    assert torch.equal(am_a[clear], want[clear])


def _dgrad_checks(T, cuda, S, C, K, B, ko, variant, mode, unpool):
    w, go, act, sc, am, ut, dx = _bwd_case(S, C, K, B, ko)
    kw = ko or K
    zero = torch.zeros((), dtype=torch.float64, device=cuda)
    ref_out = torch.where(act.double() > 0, dx * sc.double(), zero)
    part = {0: -(dx * act.double()), 1: dx.abs(), 2: torch.where(act.double() > 0, dx.abs(), zero)}[mode]
    ref_t = part.sum((1, 2))
    R = T.wino4_taylor_slots(S)
    unp = am if unpool else None

    def run(want_out, want_tay):
        tay = torch.zeros(R + 1, B, kw, device=cuda) if want_tay else None
        return T.conv_wino4_dgrad(go, ut, act, sc, tay, want_out, mode, 1, variant, unp if want_out else None), tay

    o_t, t_o = run(True, True)
    o_n, _ = run(True, False)
    o_t2, t_o2 = run(True, True)
    pooled_out = T.conv_wino4_dgrad(go, ut, act, sc, None, True, mode, 1, variant) if unpool else o_t
    err = _rel(pooled_out, ref_out)
    errt = _rel(t_o.sum(0), ref_t)
    print(f"dgrad S={S} ko={ko} v={variant} mode={mode} unpool={unpool}: out {err:.2e} partials {errt:.2e}")
    assert err < TOL, err
    assert errt < TOL, errt
    # same bits without the partial-sum buffer, and from a second identical call
    assert torch.equal(o_t, o_n) and torch.equal(o_t, o_t2) and torch.equal(t_o, t_o2)
    # masked-out elements are exact zeros; the unpooled output holds each value at its argmax
    # position and exact zeros at the window's three other positions
    assert (pooled_out[act <= 0] == 0).all()
    if unpool:
        assert o_t.shape == (B, 2 * S, 2 * S, kw)
        assert torch.equal(o_t, _unpool(pooled_out, am))
    # slots this shape does not use stay 0 (32-pixel maps: one slot per half image)
    assert t_o[R].abs().max().item() == 0.0
    if S == 32:
        assert t_o[0].abs().min().item() > 0 and t_o[1].abs().min().item() > 0
    elif S in (4, 8, 16):
        assert R == 1
    # the partials alone (no output)
    _, t_n = run(False, True)
    assert torch.equal(t_n, t_o)


@pytest.mark.parametrize("S,C,K,B,ko", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("unpool", [False, True])
def test_dgrad_specialisations(cuda, S, C, K, B, ko, variant, mode, unpool):
    _dgrad_checks(_ops(), cuda, S, C, K, B, ko, variant, mode, unpool)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_band_dgrad_specialisations(cuda, mode):
    """Band geometry (7-pixel maps, partial tiles, bands straddling images): one slot per tile."""
    S, C, K, B, ko = BAND
    _dgrad_checks(_ops(), cuda, S, C, K, B, ko, 3, mode, False)


@pytest.mark.parametrize("S,C,K,B", [(16, 8, 64, 3), (8, 16, 32, 5)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_nan_reaches_outputs(cuda, S, C, K, B, variant):
    """A NaN in one input pixel: NaN on (at least) its 3x3 output neighbourhood in every channel,
    through the ReLU; finite outputs in the other images; it wins its pooling windows with the
    argmax byte of the first NaN position; the data gradient carries it into the masked output
    (kept exactly 0 where the activation is not positive) and into that image's partials."""
    T = _ops()
    x, w, sc, sh, u, _ = _fwd_case(S, C, K, B, 0)
    b, py, px = 1, 5, 2
    xn = x.clone()
    xn[b, py, px, 3] = float("nan")
    y, _ = T.conv_wino4_fwd(xn, u, sc, sh, True, False, None, 1, variant)
    nb = y[b, py - 1:py + 2, px - 1:px + 2, :]
    assert torch.isnan(nb).all()
    others = [i for i in range(B) if i != b]
    assert torch.isfinite(y[others]).all()
    yp, am = T.conv_wino4_fwd(xn, u, sc, sh, True, True, None, 1, variant)
    win = y.unfold(1, 2, 2).unfold(2, 2, 2).reshape(B, S // 2, S // 2, K, 4)  # window order (dy, dx)
    isn = torch.isnan(win)
    has = isn.any(-1)
    assert has.any()
    assert torch.isnan(yp[has]).all() and torch.isfinite(yp[~has]).all()
    first = isn.float().argmax(-1).to(torch.uint8)
    assert torch.equal(am[has], first[has])
    assert torch.equal(yp[~has], win.max(-1).values[~has])
    # data gradient
    wd, go, act, scp, amx, ut, _ = _bwd_case(S, C, K, B, 0)
    gn = go.clone()
    gn[b, py, px, 3] = float("nan")
    for mode in (0, 1, 2):
        tay = torch.zeros(1, B, K, device=cuda)
        out = T.conv_wino4_dgrad(gn, ut, act, scp, tay, True, mode, 1, variant)
        nbo, nba = out[b, py - 1:py + 2, px - 1:px + 2, :], act[b, py - 1:py + 2, px - 1:px + 2, :]
        assert torch.isnan(nbo[nba > 0]).all()
        assert (out[act <= 0] == 0).all()
        assert torch.isfinite(out[others]).all() and torch.isfinite(tay[0, others]).all()
        if mode < 2:
            assert torch.isnan(tay[0, b]).all()
        else:  # masked |g|: NaN where the neighbourhood has a positive activation
            assert torch.isnan(tay[0, b][(nba > 0).any(0).any(0)]).all()
        up = T.conv_wino4_dgrad(gn, ut, act, scp, None, True, mode, 1, variant, amx)
        exp = _unpool(out, amx)
        assert torch.equal(torch.isnan(up), torch.isnan(exp))
        assert torch.equal(torch.nan_to_num(up), torch.nan_to_num(exp))
