"""The fused BatchNorm + Hardswish kernels (``tpamd.bn_hswish_fwd`` / ``bn_hswish_bwd``,
csrc/kernels/batchnorm.hip) against float64 autograd through F.batch_norm + F.hardswish, at the
module's width (C % 4 != 0: the per-element kernels) and carried at ``_act_w(C)`` (float4 kernels,
``cr=C``, zeros in the padding, the gradient's padding filled with 1.0 so that a leak into dx shows).

Inputs and cases: tests/test_bn_hswish.py (x = randn * 2 + 0.5, gamma ~ U(1.5, 3), beta ~ U(-3, 3);
11-20 % of the pre-activations below -3, 15-22 % above +3, none within 2e-5 of a kink in float64, so
no element is excluded). Tolerances are those tests/test_bn_relu6_gpu.py uses for the same
quantities: y and dx rtol = atol = 1e-4, running statistics 1e-5, dgamma / dbeta rtol 1e-4, atol 1e-3.
Largest observed error / bound per quantity on an MI355X: profiles/numerics/bn_hswish.txt."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_bn_hswish import CASES, EPS, IDS, MOM, inputs, nhwc, reference

pytestmark = pytest.mark.gpu


def _operands(shape, C, carried, dev):
    from torchpruner_amd.engine.train import _act_w
    x, gamma, beta, g = inputs(shape, C)
    Cp = _act_w(C) if carried else C
    return nhwc(x, Cp).to(dev), gamma.to(dev), beta.to(dev), nhwc(g, Cp, fill=1.0).to(dev)


def _ratio(got, want, rtol, atol):
    """Largest error over its bound atol + rtol * |want| (<= 1 passes assert_close)."""
    got, want = got.double().cpu(), want.double()
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


@pytest.mark.parametrize("carried", [False, True], ids=["module_width", "carried"])
@pytest.mark.parametrize("shape,C", CASES, ids=IDS)
def test_bn_hswish_matches_fp64(cuda, shape, C, carried):
    from torchpruner_amd import ops
    T = ops.require()
    ref = reference(shape, C)
    xh, gamma, beta, gh = _operands(shape, C, carried, cuda)
    Cp = xh.shape[-1]
    rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    nbt = torch.zeros((), dtype=torch.int64, device=cuda)
    y, mean, invstd, ab = T.bn_hswish_fwd(xh, gamma, beta, rm, rv, EPS, MOM, nbt, C)
    assert y.shape == xh.shape and mean.shape == invstd.shape == (Cp,) and ab.shape == (2, Cp) and int(nbt) == 1
    dx, dgamma, dbeta = T.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab, True, C)
    assert dx.shape == xh.shape and dgamma.shape == dbeta.shape == (C,)

    checks = [("y", y[..., :C], ref["y"], 1e-4, 1e-4), ("dx", dx[..., :C], ref["dx"], 1e-4, 1e-4),
              ("running_mean", rm, ref["rm"], 1e-5, 1e-5), ("running_var", rv, ref["rv"], 1e-5, 1e-5),
              ("dgamma", dgamma, ref["dgamma"], 1e-4, 1e-3), ("dbeta", dbeta, ref["dbeta"], 1e-4, 1e-3)]
    print(f"bn_hswish {shape} C={C} {'carried' if carried else 'module_width'} "
          + " ".join(f"{k}={_ratio(a, b, rt, at):.2g}" for k, a, b, rt, at in checks))
    for k, a, b, rt, at in checks:
        assert torch.isfinite(a).all(), k
        torch.testing.assert_close(a.double().cpu(), b, rtol=rt, atol=at, msg=lambda m, k=k: f"{k}: {m}")
    # the padding: exact zeros forward and backward (the gradient holds 1.0 there)
    assert (y[..., C:] == 0).all() and (dx[..., C:] == 0).all() and (ab[:, C:] == 0).all()

    # the statistics path is bn_train_fwd's: the same mean / invstd / running statistics bit for bit
    rm0, rv0 = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    v0, mean0, invstd0, _ = T.bn_train_fwd(xh, gamma, beta, rm0, rv0, EPS, MOM, None, False, None, None, C, 0)
    assert torch.equal(mean, mean0) and torch.equal(invstd, invstd0) and torch.equal(rm, rm0) and torch.equal(rv, rv0)

    # dgamma / dbeta alone
    none, dgamma2, dbeta2 = T.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab, False, C)
    assert none is None and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)

    # two calls are bit-identical
    y2, mean2, invstd2, ab2 = T.bn_hswish_fwd(xh, gamma, beta, None, None, EPS, MOM, None, C)
    dx2, dgamma3, dbeta3 = T.bn_hswish_bwd(gh, xh, gamma, mean2, invstd2, ab2, True, C)
    assert torch.equal(y2, y) and torch.equal(ab2, ab) and torch.equal(dx2, dx)
    assert torch.equal(dgamma3, dgamma) and torch.equal(dbeta3, dbeta)


@pytest.mark.parametrize("C,carried", [(13, False), (13, True), (40, False)])
def test_python_layer_runs_the_kernels(cuda, C, carried):
    """ops.bn_hswish_fwd / bn_hswish_bwd on GPU tensors are the registered ops (bit for bit), with
    ``dx`` None when not wanted."""
    from torchpruner_amd import ops
    T = ops.require()
    shape = CASES[0][0]
    xh, gamma, beta, gh = _operands(shape, C, carried, cuda)
    y, mean, invstd, ab = ops.bn_hswish_fwd(xh, gamma, beta, None, None, EPS, MOM, None, C)
    y0, mean0, invstd0, ab0 = T.bn_hswish_fwd(xh, gamma, beta, None, None, EPS, MOM, None, C)
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(invstd, invstd0) and torch.equal(ab, ab0)
    dx, dgamma, dbeta = ops.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab, True, C)
    dx0, dgamma0, dbeta0 = T.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab, True, C)
    assert torch.equal(dx, dx0) and torch.equal(dgamma, dgamma0) and torch.equal(dbeta, dbeta0)
    assert ops.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab, False, C)[0] is None


@pytest.mark.parametrize("C", [13, 40])
def test_nan_propagates_like_the_modules(cuda, C):
    """One NaN in x: its channel's statistics, and so y, are NaN over the whole channel, as
    F.hardswish(bn(x)) gives; the other channels are untouched."""
    from torchpruner_amd import ops
    T = ops.require()
    shape = CASES[0][0]
    x, gamma, beta, _ = inputs(shape, C)
    x[1, 5, 2, 3] = float("nan")
    want = F.hardswish(F.batch_norm(x, None, None, gamma, beta, True, MOM, EPS)).permute(0, 2, 3, 1)
    y = T.bn_hswish_fwd(nhwc(x, C).to(cuda), gamma.to(cuda), beta.to(cuda), None, None, EPS, MOM, None, C)[0].cpu()
    assert torch.isnan(want[..., 5]).all() and torch.isnan(y[..., 5]).all()
    assert torch.equal(torch.isnan(y), torch.isnan(want))
    keep = [c for c in range(C) if c != 5]
    torch.testing.assert_close(y[..., keep], want[..., keep], rtol=1e-4, atol=1e-4)


def test_rejections(cuda):
    from torchpruner_amd import ops
    from torchpruner_amd.ops._native import _LIB
    T = ops.require()
    shape, C = CASES[0][0], 13
    xh, gamma, beta, gh = _operands(shape, C, True, cuda)  # carried at 16
    y, mean, invstd, ab = T.bn_hswish_fwd(xh, gamma, beta, None, None, EPS, MOM, None, C)
    for bad in (ab[:, :12], ab[:1], ab.t(), ab.reshape(-1), ab.cpu(), ab.double()):  # the wrong shape, device, dtype
        with pytest.raises(RuntimeError):
            T.bn_hswish_bwd(gh, xh, gamma, mean, invstd, bad, True, C)
    with pytest.raises(RuntimeError):  # cr > C
        T.bn_hswish_fwd(xh, None, None, None, None, EPS, MOM, None, 17)
    with pytest.raises(RuntimeError):
        T.bn_hswish_bwd(gh, xh, None, mean, invstd, ab, True, 17)
    with pytest.raises(RuntimeError):  # an empty batch
        T.bn_hswish_fwd(xh[:0], gamma, beta, None, None, EPS, MOM, None, C)
    with pytest.raises(RuntimeError):
        T.bn_hswish_bwd(gh[:0], xh[:0], gamma, mean, invstd, ab, True, C)
    with pytest.raises(RuntimeError):  # the running statistics come as a pair
        T.bn_hswish_fwd(xh, gamma, beta, torch.zeros(C, device=cuda), None, EPS, MOM, None, C)
    with pytest.raises(RuntimeError):  # gamma of the carried width, not the module's
        T.bn_hswish_fwd(xh, torch.ones(16, device=cuda), None, None, None, EPS, MOM, None, C)
    with pytest.raises(RuntimeError):  # g and x of one shape
        T.bn_hswish_bwd(gh[:1], xh, gamma, mean, invstd, ab, True, C)
    with pytest.raises(ValueError):  # the Python layer checks before it dispatches
        ops.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab[:, :12], True, C)
    with pytest.raises(ValueError):
        ops.bn_hswish_fwd(xh, None, None, None, None, EPS, MOM, None, 17)
    with pytest.raises(ValueError):
        ops.bn_hswish_fwd(xh[:0], gamma, beta, None, None, EPS, MOM, None, C)
    # the launchers refuse before they look at any pointer (hipErrorInvalidValue = 1)
    lib = ctypes.CDLL(str(_LIB))
    ptr, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fwd, bwd = lib.tp_bn_hswish_fwd_train, lib.tp_bn_hswish_bwd_train
    fwd.argtypes = [ptr, ptr, i32, i32, i32, ptr, ptr, f32, f32] + [ptr] * 9
    bwd.argtypes = [ptr, ptr, ptr, i32, i32, i32] + [ptr] * 12
    fwd.restype = bwd.restype = i32
    for P, Cc, Cr in ((0, 16, 13), (60, 0, 0), (60, 16, 0), (60, 16, 17), (1 << 16, 1 << 16, 4)):
        assert fwd(None, None, P, Cc, Cr, None, None, EPS, MOM, *[None] * 9) == 1
        assert bwd(None, None, None, P, Cc, Cr, *[None] * 12) == 1
    assert bwd(None, None, None, 60, 16, 13, *[None] * 12) == 1  # no af / bf
