"""Depthwise convolution with SiLU on either side and the BN affine fused (the hidden layer of an
eval-mode EfficientNet MBConv block), NHWC:

    forward  v  = scale[c] * dwconv(in_act(x))[c] + shift[c],  y = v * sigmoid(v)
             (+ v into ``pre``, + APoZ counts, + partial sums of y over the map: the gate's pool)
    dgrad    dA = dwconv^T(g * scale[c] * silu'(v)),  silu'(v) = s * (1 + v * (1 - s)), s = sigmoid(v)
             tay += per-(image, channel) sums of -(dA * in_act(z)) (tay_mode 0) or |dA| (1)
             dz = dA * in_act'(z)

Activation codes: 0 none, 4 SiLU; ``in_act`` is one of them and ``out_act`` is 4 (codes 1..3 are
:mod:`.dwconv_hs`'s). SiLU is not monotonic, so the dgrad reads the stored pre-activation ``v``, which
the forward writes into ``pre`` in the same pass.

GPU tensors run the LDS-staged gfx950 kernels of ``csrc/kernels/dwconv_silu.hip``; CPU tensors (and
``TORCHPRUNER_BACKEND=torch``) run the PyTorch bodies below in the tensors' own dtype, which in
float64 are the oracle of the kernel tests. The partial slabs have one slot per (row band, column
band) of the kernels' finest split; the bodies put the whole sum into slot 0.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._native import require, use_native
from .dwconv_act import _nchw

__all__ = ["dwconv_silu_fwd", "dwconv_silu_dgrad", "dwconv_silu_tay_slots", "dwconv_silu_pool_slots"]

SILU = 4


def _check(in_act: int, out_act: int) -> None:
    if in_act not in (0, SILU) or out_act != SILU:
        raise ValueError(f"activation codes {in_act} / {out_act}: in_act is 0 (none) or 4 (SiLU), out_act is 4")


def _silu(t: torch.Tensor) -> torch.Tensor:
    return t * torch.sigmoid(t)


def _slope(t: torch.Tensor) -> torch.Tensor:
    s = torch.sigmoid(t)
    return s * (1.0 + t * (1.0 - s))


def dwconv_silu_tay_slots(H: int, W: int, C: int) -> int:
    """Slots R of the (R, B, C) score-partial slab of :func:`dwconv_silu_dgrad` for (H, W, C) inputs:
    (the finest row split: (H + 2) // 4 bands, at least one) x (column bands of at most 32 columns); 0 for a
    rejected shape."""
    if H < 1 or W < 1 or C < 4 or C % 4:
        return 0
    r = max(1, (H + 2) // 4) * -(-W // 32)
    return r if r < (1 << 24) else 0


def dwconv_silu_pool_slots(Ho: int, Wo: int, C: int) -> int:
    """Slots Rp of the (Rp, B, C) pool-partial slab of :func:`dwconv_silu_fwd` for (Ho, Wo, C) outputs."""
    return dwconv_silu_tay_slots(Ho, Wo, C)


def _slab(t: torch.Tensor, slots: int, B: int, C: int, name: str) -> None:
    if tuple(t.shape) != (slots, B, C):
        raise ValueError(f"{name} must be a ({slots}, {B}, {C}) slab (slots from dwconv_silu_*_slots), got "
                         f"{tuple(t.shape)}")


def dwconv_silu_fwd(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride: int, pad: int,
                    in_act: int, out_act: int = SILU, apoz: torch.Tensor | None = None,
                    pre: torch.Tensor | None = None, pool: torch.Tensor | None = None) -> torch.Tensor:
    """x (B, H, W, C), w (C, 1, k, k), scale / shift (C) -> y (B, Ho, Wo, C); ``apoz`` (B, C) receives
    ``+= count(y > 0)``, ``pre`` (the shape of y) the pre-activation, ``pool`` (a zeroed
    (``dwconv_silu_pool_slots(Ho, Wo, C)``, B, C) slab) partial sums of y over the map: sum its slots and
    divide by Ho * Wo for the gate's pooled mean."""
    if use_native(x):
        return require().dwconv_silu_fwd(x, w, scale, shift, int(stride), int(pad), int(in_act), int(out_act), apoz,
                                         pre, pool)
    _check(in_act, out_act)
    B, _, _, C = x.shape
    a = _silu(x) if in_act == SILU else x
    v = F.conv2d(_nchw(a), w.to(x.dtype), None, stride, pad, 1, C).permute(0, 2, 3, 1)
    v = v * scale.to(x.dtype) + shift.to(x.dtype)
    y = _silu(v).contiguous()
    if apoz is not None:
        apoz += (y > 0).sum((1, 2)).to(apoz.dtype)
    if pre is not None:
        if pre.shape != y.shape:
            raise ValueError("pre must have the shape of y, (B, Ho, Wo, C)")
        pre.copy_(v)
    if pool is not None:
        _slab(pool, dwconv_silu_pool_slots(y.shape[1], y.shape[2], C), B, C, "pool")
        pool[0] += y.sum((1, 2)).to(pool.dtype)
    return y


def dwconv_silu_dgrad(g: torch.Tensor, v: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, z: torch.Tensor, H: int,
                      W: int, stride: int, pad: int, in_act: int, out_act: int = SILU,
                      tay: torch.Tensor | None = None, tay_mode: int = 0) -> torch.Tensor:
    """g (unfactored dL/dy) and v (the forward's ``pre``) (B, Ho, Wo, C), z (the forward input)
    (B, H, W, C) -> dz. ``tay``: a zeroed (``dwconv_silu_tay_slots(H, W, C)``, B, C) slab that receives
    the score partials; sum its slots, or hand it to ``ops.score_fold_``."""
    if use_native(z):
        return require().dwconv_silu_dgrad(g, v, w, scale, z, int(H), int(W), int(stride), int(pad), int(in_act),
                                           int(out_act), tay, int(tay_mode))
    _check(in_act, out_act)
    B, _, _, C = z.shape
    if tuple(z.shape[1:3]) != (H, W):
        raise ValueError("z must be (B, H, W, C)")
    gm = g * scale.to(g.dtype) * _slope(v)
    dA = torch.nn.grad.conv2d_input((B, C, H, W), w.to(g.dtype), _nchw(gm).contiguous(), stride, pad, 1, C)
    dA = dA.permute(0, 2, 3, 1)
    if tay is not None:
        if tay_mode not in (0, 1):
            raise ValueError("tay_mode is 0 (Taylor) or 1 (Sensitivity)")
        _slab(tay, dwconv_silu_tay_slots(H, W, C), B, C, "tay")
        term = dA.abs() if tay_mode == 1 else -(dA * (_silu(z) if in_act == SILU else z))
        tay[0] += term.sum((1, 2)).to(tay.dtype)
    return (dA * _slope(z) if in_act == SILU else dA).contiguous()
