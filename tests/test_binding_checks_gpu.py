"""Operand checks of the engine bindings (csrc/engine_bindings.cpp on csrc/include/tp_bind.h): calls
that used to reach a kernel with a bad operand are rejected.

Every case first makes the valid call at the smallest shape the op accepts and checks the output's
shape, then the bad call under ``pytest.raises``. The bad operands are harmless should a check be
missing (the test then fails by not raising, the GPU does not fault): "not on the GPU" operands are
pinned host tensors, which the device can read, and short vectors are views of a full-length
buffer. Operands on a second GPU are rejected by the same ``like`` comparison; that needs two devices
and is not run here."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    from torchpruner_amd import ops
    return ops.require()


def _pinned(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).pin_memory()


def _dgrad_operands(cuda):
    """act (2,4,4,32), the 2x2-pooled grad (2,2,2,32) + its argmax bytes, and a 3x3 weight (32,32,3,3)"""
    gen = torch.Generator(device=cuda).manual_seed(11)
    act = torch.relu(torch.randn(2, 4, 4, 32, device=cuda, generator=gen))
    g = torch.randn(2, 2, 2, 32, device=cuda, generator=gen)
    am = torch.randint(0, 4, (2, 2, 2, 32), device=cuda, generator=gen, dtype=torch.uint8)
    w = torch.randn(32, 32, 3, 3, device=cuda, generator=gen) / 17
    return act, g, am, w


def test_conv_dgrad_rejects_host_argmax(cuda):
    T = _ops()
    act, g, am, w = _dgrad_operands(cuda)
    wt = w.flip(2, 3).permute(1, 2, 3, 0).reshape(32, 288).contiguous()  # (Cin, (kh, kw, co))
    out = T.conv_dgrad(g, am, wt, act, None, None, True, 3, 0, 1)
    assert out.shape == (2, 4, 4, 32)
    with pytest.raises(RuntimeError):
        T.conv_dgrad(g, _pinned(2, 2, 2, 32, dtype=torch.uint8), wt, act, None, None, True, 3, 0, 1)


def test_conv_wino_dgrad_rejects_host_argmax(cuda):
    T = _ops()
    act, g, am, w = _dgrad_operands(cuda)
    ut = T.wino_weights(w, True)
    out = T.conv_wino_dgrad(g, am, ut, act, None, None, True, 1)
    assert out.shape == (2, 4, 4, 32)
    with pytest.raises(RuntimeError):
        T.conv_wino_dgrad(g, _pinned(2, 2, 2, 32, dtype=torch.uint8), ut, act, None, None, True, 1)


def test_unpool2_rejects_host_argmax(cuda):
    T = _ops()
    g = torch.randn(2, 2, 2, 4, device=cuda)
    out = T.unpool2_nhwc(g, torch.zeros(2, 2, 2, 4, device=cuda, dtype=torch.uint8))
    assert out.shape == (2, 4, 4, 4)
    with pytest.raises(RuntimeError):
        T.unpool2_nhwc(g, _pinned(2, 2, 2, 4, dtype=torch.uint8))


def test_conv_first_rejects_short_scale_and_shift(cuda):
    T = _ops()
    x = torch.randn(2, 3, 8, 8, device=cuda)
    w = torch.randn(16, 3, 3, 3, device=cuda)
    scale, shift = torch.ones(16, device=cuda), torch.zeros(16, device=cuda)
    out = T.conv_first(x, w, scale, shift, True)
    assert out.shape == (2, 8, 8, 16)
    with pytest.raises(RuntimeError):
        T.conv_first(x, w, scale[:12], shift, True)
    with pytest.raises(RuntimeError):
        T.conv_first(x, w, scale, shift[:12], True)


def test_bn_train_fwd_rejects_running_mean_without_var(cuda):
    T = _ops()
    x = torch.randn(8, 4, device=cuda)
    mean, var = torch.zeros(4, device=cuda), torch.ones(4, device=cuda)
    y = T.bn_train_fwd(x, None, None, mean, var, 1e-5, 0.1)[0]
    assert y.shape == (8, 4)
    with pytest.raises(RuntimeError):
        T.bn_train_fwd(x, None, None, mean, None, 1e-5, 0.1)


def test_conv_fwd_and_conv_gen_reject_host_operands(cuda):
    T = _ops()
    x = torch.randn(2, 4, 4, 32, device=cuda)
    w = torch.randn(32, 288, device=cuda) / 17
    out, _ = T.conv_fwd(x, w, None, None, True, False, 3, 0, 1, torch.zeros(2, 32, device=cuda))
    assert out.shape == (2, 4, 4, 32)
    with pytest.raises(RuntimeError):
        T.conv_fwd(x, w, None, None, True, False, 3, 0, 1, _pinned(2, 32))
    assert T.conv_gen_k(3, 32) == 288
    out = T.conv_gen(x, w, None, None, True, torch.zeros(2, 4, 4, 32, device=cuda), None, 3, 1, 1, 0, 1)
    assert out.shape == (2, 4, 4, 32)
    with pytest.raises(RuntimeError):
        T.conv_gen(x, w, None, None, True, _pinned(2, 4, 4, 32), None, 3, 1, 1, 0, 1)


def test_wgrads_reject_zero_stride_out(cuda):
    T = _ops()
    g = torch.randn(2, 4, 4, 32, device=cuda)
    x = torch.randn(2, 4, 4, 32, device=cuda)
    overlapping = torch.zeros(1, 1, 3, 3, device=cuda).expand(32, 32, 3, 3)
    out = torch.full((32, 32, 3, 3), float("nan"), device=cuda)
    assert T.conv_wgrad(g, x, 3, 1, 1, 0, 1, out).numel() == 0  # the result is in ``out``
    assert out.shape == (32, 32, 3, 3) and torch.isfinite(out).all()
    with pytest.raises(RuntimeError):
        T.conv_wgrad(g, x, 3, 1, 1, 0, 1, overlapping)
    out2 = torch.full((32, 32, 3, 3), float("nan"), device=cuda)
    T.wino_wgrad(g, x, 0, 1, out2)
    assert out2.shape == (32, 32, 3, 3) and torch.isfinite(out2).all()
    with pytest.raises(RuntimeError):
        T.wino_wgrad(g, x, 0, 1, overlapping)


def test_dgrads_reject_bad_tay_mode(cuda):
    """None of the four launchers checks tay_mode (tp_conv_igemm, tp_conv_wino, tp_conv_wino4 and
    tp_conv_gen store it in the kernel arguments as given), so all four are rejected by the binding."""
    T = _ops()
    act, g, am, w = _dgrad_operands(cuda)
    wt = w.flip(2, 3).permute(1, 2, 3, 0).reshape(32, 288).contiguous()
    assert T.conv_dgrad(g, am, wt, act, None, None, True, 3, 0, 1, 0, 2).shape == (2, 4, 4, 32)
    with pytest.raises(RuntimeError):
        T.conv_dgrad(g, am, wt, act, None, None, True, 3, 0, 1, 0, 7)
    ut = T.wino_weights(w, True)
    assert T.conv_wino_dgrad(g, am, ut, act, None, None, True, 1, True, 2).shape == (2, 4, 4, 32)
    with pytest.raises(RuntimeError):
        T.conv_wino_dgrad(g, am, ut, act, None, None, True, 1, True, 7)
    # F(4x4): the (K, C) = (32, 8) weight of test_wino4_rejects_bad_shapes, on a valid 4-pixel map
    w4 = torch.randn(8, 32, 3, 3, device=cuda) / 17
    g4 = torch.randn(2, 4, 4, 8, device=cuda)
    ut4 = T.wino4_weights(w4, True, 0, 0)
    assert T.conv_wino4_dgrad(g4, ut4, act, None, None, True, 2).shape == (2, 4, 4, 32)
    with pytest.raises(RuntimeError):
        T.conv_wino4_dgrad(g4, ut4, act, None, None, True, 7)
    # GEN 1x1 data gradient with a mask
    gg = torch.randn(2, 4, 4, 32, device=cuda)
    wg = torch.randn(32, 32, device=cuda) / 6
    assert T.conv_gen_bwd(gg, wg, None, 1, act, 1, 1, 0, 4, 4, False, 0, 1, None, 1).shape == (2, 4, 4, 32)
    with pytest.raises(RuntimeError):
        T.conv_gen_bwd(gg, wg, None, 1, act, 1, 1, 0, 4, 4, False, 0, 1, None, 7)
