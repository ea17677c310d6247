"""Training-mode BatchNorm fused with SiLU on channels-last rows x (..., C), the tail of an
EfficientNet ``Conv2d -> BatchNorm2d -> SiLU`` unit:

    forward   y, mean, invstd, ab = bn_silu_fwd(x, gamma, beta, running_mean, running_var, eps, momentum)
                  v = x * a[c] + b[c],  a = gamma * invstd,  b = beta - mean * a     (ab = rows a, b)
                  y = v * s,  s = 1 / (1 + exp(-v))
    backward  dx, dgamma, dbeta = bn_silu_bwd(g, x, gamma, mean, invstd, ab, want_dx)
                  gm = g * s * (1 + v * (1 - s)), then the BatchNorm backward on gm

The contract is that of :mod:`.bn_hswish`: the backward recomputes v from x and the forward's ``ab``
(neither v nor y is kept), ``cr`` (0 = C) channels carry parameters and channels c >= cr are zero
padding (y = 0 and dx = 0 there, no statistic written), the running statistics and ``num_batches``
are updated in place. The sigmoid is formed as 1 / (1 + exp(-v)), which saturates to 0 and 1 without
an inf / inf: at v = -100 y is -0 and the derivative 0, at v = +100 y is v and the derivative 1.
GPU tensors run the gfx950 kernels of ``csrc/kernels/batchnorm.hip`` (fp32; every sum in a fixed
order); CPU tensors (and ``TORCHPRUNER_BACKEND=torch``) run the PyTorch bodies below in the tensors'
own dtype, which in float64 are the oracle of the kernel tests.
"""
from __future__ import annotations

import torch

from ._native import require, use_native
from .bn_hswish import _c, _dims, _vec

__all__ = ["bn_silu_fwd", "bn_silu_bwd"]


def bn_silu_fwd(x: torch.Tensor, gamma, beta, running_mean, running_var, eps: float, momentum: float,
                num_batches=None, cr: int = 0):
    """x (..., C) -> (y like x, mean (C,), invstd (C,), ab (2, C))."""
    C, P, cr = _dims(x, cr, "x")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _vec(t, cr, name)
    if running_mean is not None and running_var is None:
        raise ValueError("running_mean needs running_var")
    if use_native(x):
        return tuple(require().bn_silu_fwd(_c(x), _c(gamma), _c(beta), running_mean, running_var, float(eps),
                                           float(momentum), num_batches, cr))
    xr = x.reshape(P, C)
    mean = xr.mean(0)
    var = ((xr - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    a, b = torch.zeros_like(mean), torch.zeros_like(mean)
    a[:cr] = invstd[:cr] if gamma is None else gamma.to(x.dtype) * invstd[:cr]
    b[:cr] = -mean[:cr] * a[:cr] if beta is None else beta.to(x.dtype) - mean[:cr] * a[:cr]
    if running_mean is not None:
        unbiased = var[:cr] * (P / (P - 1)) if P > 1 else var[:cr]
        running_mean.mul_(1 - momentum).add_(momentum * mean[:cr].to(running_mean.dtype))
        running_var.mul_(1 - momentum).add_(momentum * unbiased.to(running_var.dtype))
    if num_batches is not None:
        num_batches.add_(1)
    v = x * a + b
    return v * torch.sigmoid(v), mean, invstd, torch.stack((a, b))


def bn_silu_bwd(g: torch.Tensor, x: torch.Tensor, gamma, mean: torch.Tensor, invstd: torch.Tensor,
                ab: torch.Tensor, want_dx: bool = True, cr: int = 0):
    """(dx like x or None, dgamma (cr,), dbeta (cr,)) of ``bn_silu_fwd``; ``ab``: its fourth output."""
    C, P, cr = _dims(x, cr, "x")
    if g.shape != x.shape:
        raise ValueError(f"g {tuple(g.shape)} and x {tuple(x.shape)} must have one shape")
    _vec(gamma, cr, "gamma")
    _vec(mean, C, "mean")
    _vec(invstd, C, "invstd")
    if tuple(ab.shape) != (2, C):
        raise ValueError(f"ab must be (2, {C}), got {tuple(ab.shape)}")
    if use_native(g):
        dx, dgamma, dbeta = require().bn_silu_bwd(_c(g), _c(x), _c(gamma), mean, invstd, ab, bool(want_dx), cr)
        return (dx if want_dx else None), dgamma, dbeta
    v = x * ab[0] + ab[1]
    s = torch.sigmoid(v)
    gm = g * s * (1.0 + v * (1.0 - s))
    xhat = (x - mean) * invstd
    sg, sgx = gm.reshape(P, C).sum(0), (gm * xhat).reshape(P, C).sum(0)
    dx = None
    if want_dx:
        ac = torch.zeros_like(mean)
        ac[:cr] = invstd[:cr] if gamma is None else gamma.to(x.dtype) * invstd[:cr]
        dx = ac * (gm - sg / P - xhat * (sgx / P))
        dx[..., cr:] = 0  # the padding: exact zeros whatever g holds there
    return dx, sgx[:cr].clone(), sg[:cr].clone()
