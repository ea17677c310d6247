"""Depthwise-conv kernels (csrc/kernels/dwconv.hip: forward, input gradient, weight + bias
gradient) against fp64 CPU references, with derived tolerances.

fp32 accumulation of n terms in any order has error <= n * 2^-24 * sum|terms| (first order), so
every bound is computed in fp64 from the absolute values of the operands:

  forward   |y  - ref| <= (k^2 + 2) * 2^-24 * (|x| conv |w| + |b|)      elementwise
  dgrad     |dx - ref| <= (k^2 + 2) * 2^-24 * conv2d_input(|g|, |w|)    elementwise
  wgrad     |dW - ref| <= (P + 2)   * 2^-24 * conv2d_weight(|x|, |g|)   P = B * Ho * Wo (any chunking)
  bias      |db - ref| <= (P + 2)   * 2^-24 * sum|g|

A violation is a bug, not noise."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# (C, H, W, k, stride, pad, B)
CASES = [
    (4, 7, 9, 3, 1, 1, 1),      # one quad
    (24, 15, 13, 3, 2, 1, 3),   # odd sizes, stride 2
    (24, 8, 8, 3, 2, 0, 2),     # last input row / column covered by no window: dx exactly 0 there
    (67, 6, 5, 3, 1, 1, 2),     # C % 4 != 0: per-element path
    (103, 9, 9, 5, 2, 2, 1),    # C % 4 != 0, k = 5
    (40, 1, 5, 3, 1, 1, 2),     # map smaller than the kernel
    (8, 2, 3, 5, 1, 2, 1),      # map smaller than the kernel, k = 5
    (144, 14, 14, 5, 1, 4, 2),  # pad = k - 1
    (8, 48, 50, 3, 1, 1, 2),    # 18 wgrad chunks: every lane of the chunk fold, and a second pass
    (6, 80, 72, 3, 2, 1, 4),    # 22 chunks on the per-element path
]
IDS = ["c%d_%dx%d_k%d_s%d_p%d_b%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs (fp32, NCHW on the CPU) and the fp64 references / error bounds, computed once."""
    C, H, W, k, s, p, B = case
    gen = torch.Generator().manual_seed(1000 * C + 10 * H + k + s + p)
    x = torch.randn(B, C, H, W, generator=gen)
    w = torch.randn(C, 1, k, k, generator=gen)
    b = torch.randn(C, generator=gen)
    x64, w64, b64 = x.double(), w.double(), b.double()
    y = F.conv2d(x64, w64, None, s, p, groups=C)
    g = torch.randn(y.shape, generator=gen)
    g64 = g.double()
    P = B * y.shape[2] * y.shape[3]
    r = {"x": x, "w": w, "b": b, "g": g, "y": y, "yb": y + b64.view(1, C, 1, 1)}
    r["y_bound"] = (k * k + 2) * U * F.conv2d(x64.abs(), w64.abs(), None, s, p, groups=C)
    r["yb_bound"] = r["y_bound"] + (k * k + 2) * U * b64.abs().view(1, C, 1, 1)
    r["dx"] = torch.nn.grad.conv2d_input(x.shape, w64, g64, s, p, groups=C)
    r["dx_bound"] = (k * k + 2) * U * torch.nn.grad.conv2d_input(x.shape, w64.abs(), g64.abs(), s, p, groups=C)
    r["dw"] = torch.nn.grad.conv2d_weight(x64, w.shape, g64, s, p, groups=C)
    r["dw_bound"] = (P + 2) * U * torch.nn.grad.conv2d_weight(x64.abs(), w.shape, g64.abs(), s, p, groups=C)
    r["db"] = g64.sum((0, 2, 3))
    r["db_bound"] = (P + 2) * U * g64.abs().sum((0, 2, 3))
    return r


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def _within(got, ref, bound, what):
    err = (got - ref).abs()
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max bound {bound.max().item():.3e}, worst margin {worst:.3e}")
    assert (err <= bound).all(), f"{what}: error exceeds the derived bound by {worst:.3e}"


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_kernels_match_fp64(cuda, case, bias):
    from torchpruner_amd import ops
    T = ops.require()
    C, H, W, k, s, p, B = case
    r = _case(case)
    xh, gh, w = _nhwc(r["x"], cuda), _nhwc(r["g"], cuda), r["w"].to(cuda)
    b = r["b"].to(cuda) if bias else None
    y = T.dwconv_fwd(xh, w, b, s, p)
    assert y.shape == gh.shape
    _within(_nchw64(y), r["yb" if bias else "y"], r["yb_bound" if bias else "y_bound"], "forward")
    dx = T.dwconv_dgrad(gh, w, H, W, s, p)
    assert dx.shape == xh.shape
    _within(_nchw64(dx), r["dx"], r["dx_bound"], "dgrad")
    if (C, H, W, k, s, p) == (24, 8, 8, 3, 2, 0):  # input row 7 / column 7 lie in no window
        assert (dx[:, 7] == 0).all() and (dx[:, :, 7] == 0).all()
        assert (r["dx_bound"][:, :, 7] == 0).all() and (r["dx_bound"][:, :, :, 7] == 0).all()
    dw = torch.empty_like(w)
    db = T.dwconv_wgrad(gh, xh, k, s, p, dw, bias)
    _within(dw.double().cpu(), r["dw"], r["dw_bound"], "wgrad")
    if bias:
        _within(db.double().cpu(), r["db"], r["db_bound"], "bias grad")
    else:
        assert db is None


@pytest.mark.parametrize("case", [CASES[1], CASES[8], CASES[9]], ids=[IDS[1], IDS[8], IDS[9]])
def test_dwconv_wgrad_is_deterministic(cuda, case):
    """The issue's 24-channel stride-2 case (one chunk), and the 18- and 22-chunk cases, where
    the chunk fold's order is in play."""
    from torchpruner_amd import ops
    T = ops.require()
    C, H, W, k, s, p, B = case
    r = _case(case)
    xh, gh = _nhwc(r["x"], cuda), _nhwc(r["g"], cuda)
    outs = []
    for _ in range(2):
        dw = torch.empty(C, 1, k, k, device=cuda)
        db = T.dwconv_wgrad(gh, xh, k, s, p, dw, True)
        outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
def test_dwconv_weight_grad_keeps_parameter_strides(cuda, channels_last):
    """dW comes back with exactly the parameter's strides (DDP bucket views expect them), through
    the autograd path; the op itself honours any strides of the tensor it is handed."""
    from torchpruner_amd import ops
    from torchpruner_amd.engine.train import DW_COUNTS, dw_eligible, native_convs
    case = CASES[1]
    C, H, W, k, s, p, B = case
    r = _case(case)
    conv = torch.nn.Conv2d(C, C, k, s, p, groups=C).to(cuda)
    with torch.no_grad():
        conv.weight.copy_(r["w"])
        conv.bias.copy_(r["b"])
    if channels_last:
        conv = conv.to(memory_format=torch.channels_last)
    assert dw_eligible(conv)
    x = r["x"].to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    before = dict(DW_COUNTS)
    with native_convs(conv) as switched:
        assert switched == [conv]
        y = conv(x)
        y.backward(r["g"].to(cuda).contiguous(memory_format=torch.channels_last))
    assert all(DW_COUNTS[n] == before[n] + 1 for n in ("fwd", "dgrad", "wgrad")), (before, DW_COUNTS)
    assert conv.weight.grad.stride() == conv.weight.stride()
    _within(y.double().cpu(), r["yb"], r["yb_bound"], "forward")
    _within(x.grad.double().cpu(), r["dx"], r["dx_bound"], "dgrad")
    _within(conv.weight.grad.double().cpu(), r["dw"], r["dw_bound"], "wgrad")
    _within(conv.bias.grad.double().cpu(), r["db"], r["db_bound"], "bias grad")
    # taps transposed and channels two slots apart: written where the strides say, nothing else
    dw = torch.full((C * 2 * k * k,), 7.0, device=cuda).as_strided((C, 1, k, k), (2 * k * k, 1, 1, k))
    ops.require().dwconv_wgrad(_nhwc(r["g"], cuda), _nhwc(r["x"], cuda), k, s, p, dw, False)
    assert dw.stride() == (2 * k * k, 1, 1, k)
    _within(dw.double().cpu(), r["dw"], r["dw_bound"], "wgrad (strided)")
    base = dw.as_strided((C, 2, k * k), (2 * k * k, k * k, 1))
    assert (base[:, 1] == 7.0).all()
