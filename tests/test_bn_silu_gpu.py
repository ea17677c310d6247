"""tpamd.bn_silu_fwd / bn_silu_bwd (csrc/kernels/batchnorm.hip) against float64 autograd, at the module's width
and carried at _act_w(C) (the gradient's padding filled with 1.0). Cases, inputs and tolerances of
tests/test_bn_hswish_gpu.py. Largest error / bound on an MI355X: profiles/numerics/bn_silu.txt."""
import pytest
import torch
import torch.nn.functional as F

from test_bn_hswish import CASES, EPS, IDS, MOM, inputs, nhwc
from test_bn_hswish_gpu import _ratio
from test_bn_silu import reference, saturated

pytestmark = pytest.mark.gpu


def _run_and_check(cuda, shape, C, carried, saturate=False):
    """Forward and backward on one case against float64; returns the op namespace, operands and results."""
    from torchpruner_amd import ops
    from torchpruner_amd.engine.train import _act_w
    T, ref = ops.require(), reference(shape, C, saturate)
    x, gamma, beta, g = inputs(shape, C)
    if saturate:
        gamma, beta = saturated(gamma, beta)
    Cp = _act_w(C) if carried else C
    xh, gamma, beta, gh = nhwc(x, Cp).to(cuda), gamma.to(cuda), beta.to(cuda), nhwc(g, Cp, fill=1.0).to(cuda)
    rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    nbt = torch.zeros((), dtype=torch.int64, device=cuda)
    y, mean, invstd, ab = T.bn_silu_fwd(xh, gamma, beta, rm, rv, EPS, MOM, nbt, C)
    dx, dgamma, dbeta = T.bn_silu_bwd(gh, xh, gamma, mean, invstd, ab, True, C)
    assert mean.shape == (Cp,) and ab.shape == (2, Cp) and dgamma.shape == (C,) and int(nbt) == 1
    checks = [("y", y[..., :C], ref["y"], 1e-4, 1e-4), ("dx", dx[..., :C], ref["dx"], 1e-4, 1e-4),
              ("running_mean", rm, ref["rm"], 1e-5, 1e-5), ("running_var", rv, ref["rv"], 1e-5, 1e-5),
              ("dgamma", dgamma, ref["dgamma"], 1e-4, 1e-3), ("dbeta", dbeta, ref["dbeta"], 1e-4, 1e-3)]
    print(f"bn_silu {shape} C={C} {'carried' if carried else 'module_width'}{' saturated' if saturate else ''} "
          + " ".join(f"{k}={_ratio(a, b, rt, at):.2g}" for k, a, b, rt, at in checks))
    for k, a, b, rt, at in checks:
        assert torch.isfinite(a).all(), k
        torch.testing.assert_close(a.double().cpu(), b, rtol=rt, atol=at, msg=lambda m, k=k: f"{k}: {m}")
    assert (y[..., C:] == 0).all() and (dx[..., C:] == 0).all() and (ab[:, C:] == 0).all()  # the padding
    return T, (xh, gamma, beta, gh), (y, mean, invstd, ab, rm, rv), (dx, dgamma, dbeta)


@pytest.mark.parametrize("carried", [False, True], ids=["module_width", "carried"])
@pytest.mark.parametrize("shape,C", CASES, ids=IDS)
def test_bn_silu_matches_fp64(cuda, shape, C, carried):
    T, (xh, gamma, beta, gh), (y, mean, invstd, ab, rm, rv), (dx, dgamma, dbeta) = _run_and_check(cuda, shape, C, carried)
    # the statistics path is bn_train_fwd's, bit for bit
    rm0, rv0 = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    _, mean0, invstd0, _ = T.bn_train_fwd(xh, gamma, beta, rm0, rv0, EPS, MOM, None, False, None, None, C, 0)
    assert torch.equal(mean, mean0) and torch.equal(invstd, invstd0) and torch.equal(rm, rm0) and torch.equal(rv, rv0)
    none, dgamma2, dbeta2 = T.bn_silu_bwd(gh, xh, gamma, mean, invstd, ab, False, C)  # dgamma / dbeta alone
    assert none is None and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)
    y2, mean2, invstd2, ab2 = T.bn_silu_fwd(xh, gamma, beta, None, None, EPS, MOM, None, C)  # a second call
    dx2, dgamma3, dbeta3 = T.bn_silu_bwd(gh, xh, gamma, mean2, invstd2, ab2, True, C)
    assert torch.equal(y2, y) and torch.equal(ab2, ab) and torch.equal(dx2, dx)
    assert torch.equal(dgamma3, dgamma) and torch.equal(dbeta3, dbeta)


@pytest.mark.parametrize("C,carried", [(13, False), (13, True), (40, False)])
def test_saturation(cuda, C, carried):
    """Pre-activations of +100 and -100: y = v and -0, all finite (exp(v) / (1 + exp(v)) gives NaN at +100)."""
    y = _run_and_check(cuda, CASES[0][0], C, carried, True)[2][0]
    assert (y[..., 1] > 99).all() and (y[..., 2] == 0).all()


@pytest.mark.parametrize("C", [13, 40])
def test_nan_propagates_like_the_modules(cuda, C):
    from torchpruner_amd import ops
    x, gamma, beta, _ = inputs(CASES[0][0], C)
    x[1, 5, 2, 3] = float("nan")
    want = F.silu(F.batch_norm(x, None, None, gamma, beta, True, MOM, EPS)).permute(0, 2, 3, 1)
    y = ops.require().bn_silu_fwd(nhwc(x, C).to(cuda), gamma.to(cuda), beta.to(cuda), None, None, EPS, MOM, None, C)[0]
    assert torch.isnan(want[..., 5]).all() and torch.equal(torch.isnan(y.cpu()), torch.isnan(want))


def test_rejections(cuda):
    import ctypes
    from torchpruner_amd.ops._native import _LIB
    from torchpruner_amd import ops
    T = ops.require()
    x, gamma, _, g = inputs(CASES[0][0], 13)
    xh, gamma, gh = nhwc(x, 16).to(cuda), gamma.to(cuda), nhwc(g, 16).to(cuda)
    y, mean, invstd, ab = T.bn_silu_fwd(xh, gamma, None, None, None, EPS, MOM, None, 13)
    for bad in (ab[:, :12], ab.cpu(), ab.double()):  # the wrong shape, device, dtype
        with pytest.raises(RuntimeError):
            T.bn_silu_bwd(gh, xh, gamma, mean, invstd, bad, True, 13)
    with pytest.raises(RuntimeError):  # cr > C
        T.bn_silu_fwd(xh, None, None, None, None, EPS, MOM, None, 17)
    with pytest.raises(ValueError):  # the Python layer checks before it dispatches
        ops.bn_silu_bwd(gh, xh, gamma, mean, invstd, ab[:, :12], True, 13)
    # the launchers refuse before they look at any pointer (hipErrorInvalidValue = 1)
    lib, ptr, i32, f32 = ctypes.CDLL(str(_LIB)), ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fwd, bwd = lib.tp_bn_silu_fwd_train, lib.tp_bn_silu_bwd_train
    fwd.argtypes = [ptr, ptr, i32, i32, i32, ptr, ptr, f32, f32] + [ptr] * 9
    bwd.argtypes = [ptr, ptr, ptr, i32, i32, i32] + [ptr] * 12
    for P, Cc, Cr in ((0, 16, 13), (60, 0, 0), (60, 16, 0), (60, 16, 17), (1 << 16, 1 << 16, 4)):
        assert fwd(None, None, P, Cc, Cr, None, None, EPS, MOM, *[None] * 9) == 1 == bwd(None, None, None, P, Cc, Cr, *[None] * 12)
    assert bwd(None, None, None, 60, 16, 13, *[None] * 12) == 1  # no af / bf
