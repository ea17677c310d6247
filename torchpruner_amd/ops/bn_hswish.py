"""Training-mode BatchNorm fused with Hardswish on channels-last rows x (..., C), the tail of a
MobileNetV3 ``Conv2d -> BatchNorm2d -> Hardswish`` unit:

    forward   y, mean, invstd, ab = bn_hswish_fwd(x, gamma, beta, running_mean, running_var, eps, momentum)
                  v = x * a[c] + b[c],  a = gamma * invstd,  b = beta - mean * a     (ab = rows a, b)
                  y = v * min(max(v + 3, 0), 6) / 6                                  (ATen's expression)
    backward  dx, dgamma, dbeta = bn_hswish_bwd(g, x, gamma, mean, invstd, ab, want_dx)
                  gm = g * d(v),  d(v) = 0 if v < -3; v / 3 + 0.5 if v <= 3; else 1  (ATen's branch order)
                  then the BatchNorm backward on gm

The backward recomputes v from x and the forward's ``ab``: neither v, y nor a mask is kept.
``cr`` (0 = C): the channels carrying parameters; channels c >= cr are the zero padding of a pruned
width carried wider (a = b = 0: y = 0 and dx = 0 there, no statistic written). The running statistics
(momentum, unbiased variance) and ``num_batches`` are updated in place as ``bn_train_fwd`` does.
GPU tensors run the gfx950 kernels of ``csrc/kernels/batchnorm.hip`` (fp32; every sum in a fixed
order); CPU tensors (and ``TORCHPRUNER_BACKEND=torch``) run the PyTorch bodies below in the tensors'
own dtype, which in float64 are the oracle of the kernel tests.
"""
from __future__ import annotations

import torch

from ._native import require, use_native

__all__ = ["bn_hswish_fwd", "bn_hswish_bwd"]


def _dims(x: torch.Tensor, cr: int, name: str):
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"{name} must be a non-empty (..., C) tensor, got {tuple(x.shape)}")
    C = x.shape[-1]
    cr = int(cr) if cr else C
    if not 0 < cr <= C:
        raise ValueError(f"cr = {cr} must be in 1..C = {C}")
    return C, x.numel() // C, cr


def _vec(t, n: int, name: str) -> None:
    if t is not None and tuple(t.shape) != (n,):
        raise ValueError(f"{name} must be ({n},), got {tuple(t.shape)}")


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


def bn_hswish_fwd(x: torch.Tensor, gamma, beta, running_mean, running_var, eps: float, momentum: float,
                  num_batches=None, cr: int = 0):
    """x (..., C) -> (y like x, mean (C,), invstd (C,), ab (2, C))."""
    C, P, cr = _dims(x, cr, "x")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _vec(t, cr, name)
    if running_mean is not None and running_var is None:
        raise ValueError("running_mean needs running_var")
    if use_native(x):
        return tuple(require().bn_hswish_fwd(_c(x), _c(gamma), _c(beta), running_mean, running_var, float(eps),
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
    return v * torch.clamp(v + 3.0, 0.0, 6.0) / 6.0, mean, invstd, torch.stack((a, b))


def bn_hswish_bwd(g: torch.Tensor, x: torch.Tensor, gamma, mean: torch.Tensor, invstd: torch.Tensor,
                  ab: torch.Tensor, want_dx: bool = True, cr: int = 0):
    """(dx like x or None, dgamma (cr,), dbeta (cr,)) of ``bn_hswish_fwd``; ``ab``: its fourth output."""
    C, P, cr = _dims(x, cr, "x")
    if g.shape != x.shape:
        raise ValueError(f"g {tuple(g.shape)} and x {tuple(x.shape)} must have one shape")
    _vec(gamma, cr, "gamma")
    _vec(mean, C, "mean")
    _vec(invstd, C, "invstd")
    if tuple(ab.shape) != (2, C):
        raise ValueError(f"ab must be (2, {C}), got {tuple(ab.shape)}")
    if use_native(g):
        dx, dgamma, dbeta = require().bn_hswish_bwd(_c(g), _c(x), _c(gamma), mean, invstd, ab, bool(want_dx), cr)
        return (dx if want_dx else None), dgamma, dbeta
    v = x * ab[0] + ab[1]
    gm = torch.where(v < -3.0, torch.zeros_like(g), torch.where(v <= 3.0, g * (v / 3.0 + 0.5), g))
    xhat = (x - mean) * invstd
    sg, sgx = gm.reshape(P, C).sum(0), (gm * xhat).reshape(P, C).sum(0)
    dx = None
    if want_dx:
        ac = torch.zeros_like(mean)
        ac[:cr] = invstd[:cr] if gamma is None else gamma.to(x.dtype) * invstd[:cr]
        dx = ac * (gm - sg / P - xhat * (sgx / P))
        dx[..., cr:] = 0  # the padding: exact zeros whatever g holds there
    return dx, sgx[:cr].clone(), sg[:cr].clone()
