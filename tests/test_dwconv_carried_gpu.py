"""Depthwise-conv kernels on carried (padded) widths: the activations hold Cp >= Cw channels per
pixel, the parameter Cw (csrc/kernels/dwconv.hip, the CARRY kernels behind tp_dwconv_* at Cw < C).

The real channels are checked against the fp64 references of tests/test_dwconv_gpu.py with its
derived bounds (fp32 accumulation of n terms: error <= n * 2^-24 * sum|terms|; see that file). The
padding channels of x and g are filled with 1e30, not zeros: no output may depend on them, and the
padding channels of y and dx must be exact zeros (0 * 1e30 is fine, a kernel that multiplied the
padding of x by the padding of g, or read weights past the parameter, would show)."""
import pytest
import torch

from test_dwconv_gpu import _case, _nchw64, _nhwc, _within

pytestmark = pytest.mark.gpu

# (Cw, Cp, H, W, k, stride, pad, B)
CASES = [
    (13, 16, 7, 9, 3, 1, 1, 2),     # boundary quad with one real channel
    (22, 24, 15, 13, 3, 2, 1, 3),   # two real channels, stride 2
    (5, 8, 6, 5, 5, 1, 2, 2),       # one whole padding quad plus a boundary quad
    (67, 72, 9, 9, 5, 2, 2, 1),
    (8, 8, 8, 8, 3, 2, 0, 2),       # no padding: today's path
    (99, 104, 48, 50, 3, 1, 1, 1),  # many wgrad chunks
]
IDS = ["cw%d_cp%d_%dx%d_k%d_s%d_p%d_b%d" % c for c in CASES]
HUGE = 1e30


def _carried(t, Cp, dev):
    """NCHW CPU tensor -> contiguous NHWC on ``dev`` at Cp channels, the padding filled with 1e30."""
    th = _nhwc(t, dev)
    out = torch.full(th.shape[:3] + (Cp,), HUGE, device=dev)
    out[..., :th.shape[3]] = th
    return out


def _ref(case):
    Cw, Cp, H, W, k, s, p, B = case
    return _case((Cw, H, W, k, s, p, B))  # fp64 references / bounds on the real channels, computed once


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_carried_kernels_match_fp64(cuda, case, bias):
    from torchpruner_amd import ops
    T = ops.require()
    Cw, Cp, H, W, k, s, p, B = case
    r = _ref(case)
    xh, gh, w = _carried(r["x"], Cp, cuda), _carried(r["g"], Cp, cuda), r["w"].to(cuda)
    b = r["b"].to(cuda) if bias else None
    y = T.dwconv_fwd(xh, w, b, s, p)
    assert y.shape == gh.shape and y.shape[3] == Cp
    _within(_nchw64(y[..., :Cw]), r["yb" if bias else "y"], r["yb_bound" if bias else "y_bound"], "forward")
    assert (y[..., Cw:] == 0).all()
    dx = T.dwconv_dgrad(gh, w, H, W, s, p)
    assert dx.shape == xh.shape
    _within(_nchw64(dx[..., :Cw]), r["dx"], r["dx_bound"], "dgrad")
    assert (dx[..., Cw:] == 0).all()
    outs = []
    for _ in range(2):
        dw = torch.empty(Cw, 1, k, k, device=cuda)
        db = T.dwconv_wgrad(gh, xh, k, s, p, dw, bias)
        outs.append((dw, db))
    dw, db = outs[0]
    _within(dw.double().cpu(), r["dw"], r["dw_bound"], "wgrad")
    assert torch.equal(outs[0][0], outs[1][0])  # deterministic
    if bias:
        assert db.shape == (Cw,)
        _within(db.double().cpu(), r["db"], r["db_bound"], "bias grad")
        assert torch.equal(outs[0][1], outs[1][1])
    else:
        assert db is None
    # taps transposed and channels two slots apart: written where the strides say, nothing else
    sw = torch.full((Cw * 2 * k * k,), 7.0, device=cuda).as_strided((Cw, 1, k, k), (2 * k * k, 1, 1, k))
    T.dwconv_wgrad(gh, xh, k, s, p, sw, False)
    assert torch.equal(sw, dw)
    assert (sw.as_strided((Cw, 2, k * k), (2 * k * k, k * k, 1))[:, 1] == 7.0).all()
    if Cp == Cw:  # equal widths: the launch of an unpadded activation, bit for bit
        xr, gr = _nhwc(r["x"], cuda), _nhwc(r["g"], cuda)
        assert torch.equal(xr, xh) and torch.equal(T.dwconv_fwd(xr, w, b, s, p), y)
        assert torch.equal(T.dwconv_dgrad(gr, w, H, W, s, p), dx)


def test_carried_width_rules(cuda):
    """The bindings take x / g wider than the weight only at a multiple of 4, never narrower."""
    from torchpruner_amd import ops
    T = ops.require()
    w = torch.randn(5, 1, 3, 3, device=cuda)
    for C in (6, 7, 4, 3):
        with pytest.raises(RuntimeError):
            T.dwconv_fwd(torch.zeros(1, 4, 4, C, device=cuda), w, None, 1, 1)
        with pytest.raises(RuntimeError):
            T.dwconv_dgrad(torch.zeros(1, 4, 4, C, device=cuda), w, 4, 4, 1, 1)
        with pytest.raises(RuntimeError):
            T.dwconv_wgrad(torch.zeros(1, 4, 4, C, device=cuda), torch.zeros(1, 4, 4, C, device=cuda), 3, 1, 1,
                           torch.empty(5, 1, 3, 3, device=cuda), False)
    with pytest.raises(RuntimeError):  # the bias has the weight's channel count
        T.dwconv_fwd(torch.zeros(1, 4, 4, 8, device=cuda), w, torch.zeros(8, device=cuda), 1, 1)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=[IDS[0], IDS[1], IDS[4]])
def test_autograd_on_a_carried_input(cuda, case):
    """_NativeDWConv2d takes a carried channels_last input and returns a carried output; the
    parameter gradients have the parameter's shapes and strides."""
    from torchpruner_amd.engine.train import DW_COUNTS, FUSE_COUNTS, _NativeDWConv2d
    Cw, Cp, H, W, k, s, p, B = case
    r = _ref(case)
    weight = r["w"].to(cuda).requires_grad_(True)
    bias = r["b"].to(cuda).requires_grad_(True)
    x = _carried(r["x"], Cp, cuda).permute(0, 3, 1, 2).requires_grad_(True)  # (B, Cp, H, W) channels_last
    assert x.is_contiguous(memory_format=torch.channels_last)
    before, fbefore = dict(DW_COUNTS), FUSE_COUNTS["dw_carried"]
    y = _NativeDWConv2d.apply(x, weight, bias, s, p)
    assert y.shape[1] == Cp and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(_carried(r["g"], Cp, cuda).permute(0, 3, 1, 2))
    assert all(DW_COUNTS[n] == before[n] + 1 for n in before)
    assert FUSE_COUNTS["dw_carried"] - fbefore == (1 if Cp > Cw else 0)
    _within(y[:, :Cw].double().cpu(), r["yb"], r["yb_bound"], "forward")
    assert (y[:, Cw:] == 0).all()
    assert x.grad.shape == x.shape and (x.grad[:, Cw:] == 0).all()
    _within(x.grad[:, :Cw].double().cpu(), r["dx"], r["dx_bound"], "dgrad")
    assert weight.grad.shape == weight.shape and weight.grad.stride() == weight.stride()
    _within(weight.grad.double().cpu(), r["dw"], r["dw_bound"], "wgrad")
    assert bias.grad.shape == (Cw,)
    _within(bias.grad.double().cpu(), r["db"], r["db_bound"], "bias grad")
