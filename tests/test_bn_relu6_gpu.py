"""The training BatchNorm's fused ReLU6 tail (``bn_train_fwd(..., act=2)``, csrc/kernels/batchnorm.hip):
y = min(max(BN(x) (+ res), 0), 6), the bit mask "the gradient passes" (0 < v < 6, strict, ATen's
hardtanh_backward) and the backward that consumes it, at the module's width (C % 4 != 0: the
per-element kernels) and carried at ``_act_w(C)`` (float4 kernels, ``cr=C``, zeros in the padding).

Inputs: x = randn * 2 + 0.5, gamma ~ U(1.5, 3), beta ~ U(1, 5), res = randn, so that both clamps
are busy (10-13 % of the elements at 0, 13-18 % at 6). Tolerances are those of
tests/test_pruned_widths_gpu.py::test_bn_on_padded_activation. The mask is compared with the fp64
pre-activation outside a band of 1e-4 around either kink (the fp32 pre-activation error is about
1e-6; the band may hold at most 0.5 % of the elements); the backward is compared with an fp64
reference that takes the kernel's own bits as the ReLU6 decision, as engine/oracle.py does."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
SHAPE = (2, 6, 5)  # B, H, W


def _inputs(C, with_res):
    gen = torch.manual_seed(C + 11)
    x = torch.randn(SHAPE[0], C, *SHAPE[1:], generator=gen) * 2 + 0.5
    gamma = torch.rand(C, generator=gen) * 1.5 + 1.5
    beta = torch.rand(C, generator=gen) * 4 + 1
    res = torch.randn(SHAPE[0], C, *SHAPE[1:], generator=gen)
    g = torch.randn(SHAPE[0], C, *SHAPE[1:], generator=gen)
    return x, gamma, beta, (res if with_res else None), g


def _nhwc(t, Cp, dev, fill=0.0):
    th = t.permute(0, 2, 3, 1)
    out = torch.full(th.shape[:3] + (Cp,), fill)
    out[..., :th.shape[3]] = th
    return out.contiguous().to(dev)


def _bits(mk, n):
    """The mask bytes unpacked: flat element e is bit e & 3 of byte e >> 2."""
    b = (mk.cpu().to(torch.int32)[:, None] >> torch.arange(4, dtype=torch.int32)) & 1
    return b.reshape(-1)[:n].bool()


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("carried", [False, True], ids=["module_width", "carried"])
@pytest.mark.parametrize("C", [13, 22, 40, 67])
def test_bn_relu6_matches_fp64(cuda, C, carried, with_res):
    from torchpruner_amd import ops
    from torchpruner_amd.engine.train import _act_w
    T = ops.require()
    x, gamma, beta, res, g = _inputs(C, with_res)
    Cp = _act_w(C) if carried else C
    xh = _nhwc(x, Cp, cuda)
    rh = _nhwc(res, Cp, cuda) if with_res else None
    gh = _nhwc(g, Cp, cuda, fill=1.0)  # (a gradient on the padding must not reach dx / dres)
    rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    y, mean, invstd, mk = T.bn_train_fwd(xh, gamma.to(cuda), beta.to(cuda), rm, rv, EPS, MOM, rh, False, None, None, C,
                                         2)
    n = xh.numel()
    assert y.shape == xh.shape and mk.dtype == torch.uint8 and mk.numel() == (n + 3) // 4

    # fp64 reference
    x64 = x.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True) if with_res else None
    ga64, be64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    v = F.batch_norm(x64, rm64, rv64, ga64, be64, True, MOM, EPS)
    if with_res:
        v = v + r64
    vh = v.detach().permute(0, 2, 3, 1)
    at0, at6 = (vh <= 0).double().mean().item(), (vh >= 6).double().mean().item()
    print(f"C {C}: clamped at 0 {at0:.3f}, at 6 {at6:.3f}")
    assert at0 > 0.05 and at6 > 0.05  # both clamps are exercised

    # forward
    torch.testing.assert_close(y[..., :C].double().cpu(), vh.clamp(0, 6), rtol=1e-4, atol=1e-4)
    assert (y[..., C:] == 0).all()
    torch.testing.assert_close(rm.double().cpu(), rm64, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rv.double().cpu(), rv64, rtol=1e-5, atol=1e-5)

    # mask: bit == (0 < v < 6) wherever v is farther than 1e-4 from both kinks; padding bits 0
    bits = _bits(mk, n).reshape(xh.shape)
    sure = (vh.abs() > 1e-4) & ((vh - 6).abs() > 1e-4)
    print(f"elements within 1e-4 of a kink: {(~sure).sum().item()} of {sure.numel()}")
    assert (~sure).double().mean().item() <= 0.005
    assert torch.equal(bits[..., :C][sure], ((vh > 0) & (vh < 6))[sure])
    assert not bits[..., C:].any()
    assert (_bits(mk, 4 * mk.numel())[n:] == 0).all()  # the tail bits of the last byte

    # backward, the kernel's own bits as the ReLU6 decision
    dx, dgamma, dbeta, dres = T.bn_train_bwd(gh, xh, gamma.to(cuda), mean, invstd, True, None, with_res, mk, C, None, 2)
    keep = bits[..., :C].permute(0, 3, 1, 2).double()
    (v * keep * g.double()).sum().backward()
    torch.testing.assert_close(dx[..., :C].double().cpu(), x64.grad.permute(0, 2, 3, 1), rtol=1e-4, atol=1e-4)
    assert (dx[..., C:] == 0).all()
    if with_res:
        torch.testing.assert_close(dres[..., :C].double().cpu(), r64.grad.permute(0, 2, 3, 1), rtol=1e-5, atol=1e-5)
        assert (dres[..., C:] == 0).all()
    assert dgamma.shape == dbeta.shape == (C,)
    torch.testing.assert_close(dgamma.double().cpu(), ga64.grad, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(dbeta.double().cpu(), be64.grad, rtol=1e-4, atol=1e-3)


def test_relu_flag_and_act_code_agree(cuda):
    """``relu=True`` keeps meaning act=1, a non-zero ``act`` wins over ``relu``, and the ReLU mask
    is bit for bit what it was."""
    from torchpruner_amd import ops
    T = ops.require()
    x, gamma, beta, _, _ = _inputs(22, False)
    xh = _nhwc(x, 24, cuda)
    args = (xh, gamma.to(cuda), beta.to(cuda), None, None, EPS, MOM, None)
    y1, _, _, m1 = T.bn_train_fwd(*args, True, None, None, 22)
    y2, _, _, m2 = T.bn_train_fwd(*args, False, None, None, 22, 1)
    y3, _, _, m3 = T.bn_train_fwd(*args, True, None, None, 22, 2)
    y0, _, _, m0 = T.bn_train_fwd(*args, False, None, None, 22)
    assert torch.equal(y1, y2) and torch.equal(m1, m2) and torch.equal(y1, y0.clamp_min(0)) and m0.numel() == 0
    assert torch.equal(_bits(m1, xh.numel()).reshape(xh.shape), (y1 > 0).cpu())
    assert torch.equal(y3, y1.clamp_max(6)) and y3.max().item() == 6.0 and y1.max().item() > 6.0


def test_relu6_rejections(cuda):
    from torchpruner_amd import ops
    from torchpruner_amd.ops._native import _LIB
    T = ops.require()
    x, gamma, beta, _, g = _inputs(13, False)
    xh, gh = _nhwc(x, 16, cuda), _nhwc(g, 16, cuda)
    args = (xh, gamma.to(cuda), beta.to(cuda), None, None, EPS, MOM, None, False, None, None, 13)
    y, mean, invstd, mk = T.bn_train_fwd(*args, 2)
    with pytest.raises(RuntimeError):  # "y > 0" is no ReLU6 mask
        T.bn_train_bwd(gh, xh, gamma.to(cuda), mean, invstd, True, y, False, None, 13, None, 2)
    with pytest.raises(RuntimeError):  # ... not even next to the bits
        T.bn_train_bwd(gh, xh, gamma.to(cuda), mean, invstd, True, y, False, mk, 13, None, 2)
    with pytest.raises(RuntimeError):  # no bits at all
        T.bn_train_bwd(gh, xh, gamma.to(cuda), mean, invstd, True, None, False, None, 13, None, 2)
    for bad in (3, -1):
        with pytest.raises(RuntimeError):
            T.bn_train_fwd(*args, bad)
        with pytest.raises(RuntimeError):
            T.bn_train_bwd(gh, xh, gamma.to(cuda), mean, invstd, True, None, False, mk, 13, None, bad)
    # a ReLU6 forward asked not to return a mask: the op always returns one, so this can only be
    # asked of the launcher, which refuses before it looks at any pointer (hipErrorInvalidValue = 1)
    fwd = ctypes.CDLL(str(_LIB)).tp_bn_fwd_train
    ptr, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fwd.argtypes = [ptr, ptr, i32, i32, i32, ptr, ptr, f32, f32] + [ptr] * 8 + [i32, ptr, ptr, ptr]
    fwd.restype = i32
    null = [None] * 8
    assert fwd(None, None, 60, 16, 13, None, None, EPS, MOM, *null, 2, None, None, None) == 1
    assert fwd(None, None, 60, 16, 13, None, None, EPS, MOM, *null, 3, None, None, None) == 1
