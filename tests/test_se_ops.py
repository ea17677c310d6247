"""The PyTorch references of the ``se_*`` ops (what CPU tensors run, and the oracle of the kernel
tests) against autograd of the plain module expression in float64, and the wrappers' argument
validation."""
import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops


def _case(B, H, W, C, Cs, seed, conv_weights):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = r(B, H, W, C)
    w1, b1, w2, b2 = r(Cs, C) / C ** 0.5, r(Cs), r(C, Cs) * (3.0 / Cs ** 0.5), r(C)
    if conv_weights:
        w1, w2 = w1.reshape(Cs, C, 1, 1), w2.reshape(C, Cs, 1, 1)
    return x, w1, b1, w2, b2, r(B, H, W, C)


def _module_expr(x, w1, b1, w2, b2, gate):
    """torchvision's SqueezeExcitation on an NCHW view, with 1x1 convs."""
    xn = x.permute(0, 3, 1, 2)
    p = F.adaptive_avg_pool2d(xn, 1)
    z = F.conv2d(F.relu(F.conv2d(p, w1.reshape(*w1.shape[:2], 1, 1), b1)), w2.reshape(*w2.shape[:2], 1, 1), b2)
    # Hardsigmoid written out: ATen's hardsigmoid_backward multiplies by a float32 1/6 in every
    # dtype, so autograd of F.hardsigmoid is not a float64 oracle (its forward is, see below)
    s = torch.clamp(z + 3.0, 0.0, 6.0) / 6.0 if gate == 0 else torch.sigmoid(z)
    if gate == 0:
        torch.testing.assert_close(s, F.hardsigmoid(z), rtol=0, atol=1e-15)
    return (s * xn).permute(0, 2, 3, 1)


@pytest.mark.parametrize("gate", [0, 1])
@pytest.mark.parametrize("shape, conv_weights", [((3, 5, 7, 12, 4), True), ((2, 1, 1, 5, 1), False),
                                                 ((1, 4, 4, 9, 16), True)])
def test_reference_ops_match_autograd(shape, conv_weights, gate):
    B, H, W, C, Cs = shape
    x, w1, b1, w2, b2, g = _case(B, H, W, C, Cs, 3, conv_weights)
    leaves = [t.clone().requires_grad_() for t in (x, w1, b1, w2, b2)]
    want = _module_expr(*leaves, gate)
    want.backward(g)

    p = ops.se_pool(x)
    h, s = ops.se_gate_fwd(p, w1, b1, w2, b2, gate)
    out = ops.se_scale(x, s)
    torch.testing.assert_close(out, want.detach(), rtol=1e-12, atol=1e-12)
    if gate == 0:  # the test means something only when the gate is not saturated everywhere
        assert ((s > 0) & (s < 1)).any()

    ds = ops.se_bwd_reduce(g, x)
    dz2, dz1, dp = ops.se_gate_bwd(ds, s, h, w1, w2, gate)
    dx = ops.se_bwd_dx(g, s, dp)
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    db1 = ops.se_wgrad(dz1, p, dw1, True)
    db2 = ops.se_wgrad(dz2, h, dw2, True)
    assert ops.se_wgrad(dz2, h, dw2, False) is None
    for got, leaf in zip((dx, dw1, db1, dw2, db2), leaves):
        assert got.shape == leaf.shape
        torch.testing.assert_close(got, leaf.grad, rtol=1e-11, atol=1e-12)


def test_wgrad_writes_the_given_strides():
    a, m = torch.randn(4, 6, dtype=torch.float64), torch.randn(4, 3, dtype=torch.float64)
    store = torch.zeros(3, 6, dtype=torch.float64)
    dw = store.t()  # (6, 3) with strides (1, 6)
    ops.se_wgrad(a, m, dw)
    torch.testing.assert_close(store, m.t() @ a)


def test_argument_validation():
    x = torch.randn(2, 3, 3, 8)
    p, s, h = torch.randn(2, 8), torch.rand(2, 8), torch.rand(2, 4)
    w1, w2, b1, b2 = torch.randn(4, 8), torch.randn(8, 4), torch.randn(4), torch.randn(8)
    with pytest.raises(ValueError):
        ops.se_pool(torch.randn(2, 8))
    with pytest.raises(ValueError):
        ops.se_pool(torch.randn(0, 3, 3, 8))
    with pytest.raises(ValueError):
        ops.se_scale(x, torch.rand(2, 7))
    with pytest.raises(ValueError):
        ops.se_scale(x, torch.rand(3, 8))
    with pytest.raises(ValueError):
        ops.se_bwd_reduce(x, torch.randn(2, 3, 3, 4))
    with pytest.raises(ValueError):
        ops.se_bwd_dx(x, s, torch.randn(2, 4))
    with pytest.raises(ValueError, match="gate"):
        ops.se_gate_fwd(p, w1, b1, w2, b2, 2)
    with pytest.raises(ValueError, match="w2"):
        ops.se_gate_fwd(p, w1, b1, torch.randn(8, 5), b2)
    with pytest.raises(ValueError, match="w1"):
        ops.se_gate_fwd(p, torch.randn(4, 8, 3, 3), b1, w2, b2)
    with pytest.raises(ValueError, match="b1"):
        ops.se_gate_fwd(p, w1, b2, w2, b2)
    with pytest.raises(ValueError, match="exceed"):
        ops.se_gate_fwd(torch.randn(1, 12288), torch.randn(1, 12288), None, torch.randn(12288, 1), None)
    with pytest.raises(ValueError, match="h"):
        ops.se_gate_bwd(p, s, torch.rand(3, 4), w1, w2)
    with pytest.raises(ValueError, match="gate"):
        ops.se_gate_bwd(p, s, h, w1, w2, -1)
    with pytest.raises(ValueError, match="dw"):
        ops.se_wgrad(torch.randn(2, 8), torch.randn(2, 4), torch.empty(4, 8))
    with pytest.raises(ValueError):
        ops.se_wgrad(torch.randn(2, 8), torch.randn(3, 4), torch.empty(8, 4))
    # biases are optional, Linear- and Conv2d-shaped weights are the same operands
    h0, s0 = ops.se_gate_fwd(p, w1, None, w2, None)
    h1, s1 = ops.se_gate_fwd(p, w1.reshape(4, 8, 1, 1), None, w2.reshape(8, 4, 1, 1), None)
    assert torch.equal(h0, h1) and torch.equal(s0, s1)
    assert ops.SE_GATES == {"hardsigmoid": 0, "sigmoid": 1}
