"""(CPU) The PyTorch bodies of ops.bn_hswish_fwd / ops.bn_hswish_bwd in float64 (the oracle of the
kernel tests in test_bn_hswish_gpu.py) against autograd through F.batch_norm(training=True) +
F.hardswish, and the inputs of the kernel tests: in float64 no pre-activation of any case lies
within 2e-5 of a kink of the Hardswish (-3, +3), so the fp32 kernels (pre-activation error about
1e-6) take the reference's branch at every element and no element is ever excluded, and all three
branches are busy (at least 5 % of the elements below -3, at least 5 % above +3).

Measured with this recipe over the eight (shape, C) pairs: smallest distance to a kink 7.7e-5 (shape
(2, 10, 10), C = 67), 11-20 % of the elements below -3, 15-22 % above +3."""
import functools

import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops

EPS, MOM = 1e-5, 0.1  # as tests/test_bn_relu6_gpu.py
# (B, H, W): P = 60 is one row group of the statistics kernels, their tail loop only; P = 200 three
# groups, the unrolled loop plus the tail
SHAPES = [(2, 6, 5), (2, 10, 10)]
WIDTHS = [13, 22, 40, 67]  # 67 spans two 64-channel column blocks; 13, 22, 67: the per-element kernels
CASES = [(s, c) for s in SHAPES for c in WIDTHS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{c}" for s, c in CASES]


def inputs(shape, C):
    """x, gamma, beta, g (NCHW / per channel, float32 CPU), drawn in this order."""
    gen = torch.manual_seed(C + 11)
    x = torch.randn(shape[0], C, *shape[1:], generator=gen) * 2 + 0.5
    gamma = torch.rand(C, generator=gen) * 1.5 + 1.5
    beta = torch.rand(C, generator=gen) * 6 - 3
    g = torch.randn(shape[0], C, *shape[1:], generator=gen)
    return x, gamma, beta, g


def nhwc(t, Cp, fill=0.0):
    """(B, C, H, W) -> contiguous (B, H, W, Cp), the channels past C filled with ``fill``."""
    th = t.permute(0, 2, 3, 1)
    out = torch.full(th.shape[:3] + (Cp,), fill, dtype=t.dtype)
    out[..., :th.shape[3]] = th
    return out.contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, C):
    """float64 autograd through F.batch_norm + F.hardswish: NHWC y, v, dx and dgamma, dbeta, running
    statistics. Computed once per case and shared (never modified)."""
    x, gamma, beta, g = (t.double() for t in inputs(shape, C))
    x.requires_grad_(True)
    gamma.requires_grad_(True)
    beta.requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    v = F.batch_norm(x, rm, rv, gamma, beta, True, MOM, EPS)
    y = F.hardswish(v)
    (y * g).sum().backward()
    return dict(y=nhwc(y.detach(), C), v=nhwc(v.detach(), C), dx=nhwc(x.grad, C), dgamma=gamma.grad, dbeta=beta.grad,
                rm=rm, rv=rv)


@pytest.mark.parametrize("shape,C", CASES, ids=IDS)
def test_reference_stays_clear_of_the_kinks(shape, C):
    v = reference(shape, C)["v"]
    dist = torch.minimum((v + 3).abs(), (v - 3).abs()).min().item()
    below, above = (v < -3).double().mean().item(), (v > 3).double().mean().item()
    print(f"{shape} C={C}: distance {dist:.2e}, below -3 {below:.3f}, above +3 {above:.3f}")
    assert dist > 2e-5
    assert below >= 0.05 and above >= 0.05


@pytest.mark.parametrize("carried", [False, True], ids=["module_width", "carried"])
@pytest.mark.parametrize("shape,C", CASES, ids=IDS)
def test_torch_bodies_match_autograd(shape, C, carried):
    from torchpruner_amd.engine.train import _act_w
    ref = reference(shape, C)
    x, gamma, beta, g = (t.double() for t in inputs(shape, C))
    Cp = _act_w(C) if carried else C
    xh, gh = nhwc(x, Cp), nhwc(g, Cp, fill=1.0)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    nbt = torch.zeros((), dtype=torch.int64)
    y, mean, invstd, ab = ops.bn_hswish_fwd(xh, gamma, beta, rm, rv, EPS, MOM, nbt, C)
    assert y.shape == xh.shape and mean.shape == invstd.shape == (Cp,) and ab.shape == (2, Cp) and int(nbt) == 1
    tight = dict(rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(y[..., :C], ref["y"], **tight)
    torch.testing.assert_close(rm, ref["rm"], **tight)
    torch.testing.assert_close(rv, ref["rv"], **tight)
    assert (y[..., C:] == 0).all() and (ab[:, C:] == 0).all()
    dx, dgamma, dbeta = ops.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab, True, C)
    torch.testing.assert_close(dx[..., :C], ref["dx"], **tight)
    assert (dx[..., C:] == 0).all()
    assert dgamma.shape == dbeta.shape == (C,)
    torch.testing.assert_close(dgamma, ref["dgamma"], **tight)
    torch.testing.assert_close(dbeta, ref["dbeta"], **tight)
    none, dgamma2, dbeta2 = ops.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab, False, C)
    assert none is None and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)


def test_torch_bodies_without_affine_and_running_statistics():
    shape, C = SHAPES[0], 13
    x, _, _, g = (t.double() for t in inputs(shape, C))
    xh, gh = nhwc(x, C), nhwc(g, C)
    y, mean, invstd, ab = ops.bn_hswish_fwd(xh, None, None, None, None, EPS, MOM)
    x64 = x.clone().requires_grad_(True)
    want = F.hardswish(F.batch_norm(x64, None, None, None, None, True, MOM, EPS))
    (want * g).sum().backward()
    torch.testing.assert_close(y, nhwc(want.detach(), C), rtol=1e-11, atol=1e-11)
    dx, _, _ = ops.bn_hswish_bwd(gh, xh, None, mean, invstd, ab)
    torch.testing.assert_close(dx, nhwc(x64.grad, C), rtol=1e-11, atol=1e-11)


def test_nan_and_rejections_on_the_torch_path():
    shape, C = SHAPES[0], 13
    x, gamma, beta, g = inputs(shape, C)
    xh, gh = nhwc(x, C), nhwc(g, C)
    bad = xh.clone()
    bad[0, 0, 0, 5] = float("nan")
    y = ops.bn_hswish_fwd(bad, gamma, beta, None, None, EPS, MOM)[0]
    assert torch.isnan(y[..., 5]).all() and not torch.isnan(y[..., :5]).any() and not torch.isnan(y[..., 6:]).any()
    y, mean, invstd, ab = ops.bn_hswish_fwd(xh, gamma, beta, None, None, EPS, MOM)
    with pytest.raises(ValueError):
        ops.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab[:, :12])
    with pytest.raises(ValueError):
        ops.bn_hswish_bwd(gh, xh, gamma, mean, invstd, ab.t())
    with pytest.raises(ValueError):
        ops.bn_hswish_fwd(xh, None, None, None, None, EPS, MOM, None, 14)
    with pytest.raises(ValueError):
        ops.bn_hswish_fwd(xh[:0], gamma, beta, None, None, EPS, MOM)
    with pytest.raises(ValueError):
        ops.bn_hswish_bwd(gh[:0], xh[:0], gamma, mean, invstd, ab)


def test_training_module_exports():
    """The public pieces of the training path exist on any machine (no GPU needed to import them)."""
    from torchpruner_amd.engine import train
    assert "bn_hswish" in train.FUSE_COUNTS and callable(train.bn_hswish) and isinstance(train._HS_FUSE, bool)
    assert issubclass(train._NativeBNHswish, torch.autograd.Function)
    # on the CPU the helper is the modules' own ops
    bn = torch.nn.BatchNorm2d(5).train()
    x = torch.randn(2, 5, 3, 3)
    before = train.FUSE_COUNTS["bn_hswish"]
    want = F.hardswish(torch.nn.BatchNorm2d(5).train()(x))
    torch.testing.assert_close(train.bn_hswish(bn, x), want)
    assert train.FUSE_COUNTS["bn_hswish"] == before
