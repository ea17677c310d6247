"""Depthwise convolution with ReLU / ReLU6 / Hardswish on either side and the BN affine fused (the
hidden layer of an eval-mode MobileNetV3 inverted-residual block), NHWC:

    forward  v  = scale[c] * dwconv(in_act(x))[c] + shift[c],  y = out_act(v)   (+ APoZ counts, + v)
    dgrad    dA = dwconv^T(g * scale[c] * d_out)           (dL/d in_act(z), unfactored)
             tay += per-(image, channel) sums of -(dA * in_act(z)) (tay_mode 0) or |dA| (1)
             dz = dA * d_in(z)

Activation codes are those of :mod:`.dwconv_act` plus 3, Hardswish ``hs(v) = v * min(max(v + 3, 0),
6) / 6`` with the derivative ``d(v) = 0 if v < -3; v / 3 + 0.5 if v <= 3; else 1`` of
``ops.bn_hswish_bwd`` (ATen's branch order). For codes 0..2 ``d`` is the 0 / 1 mask of
``dwconv_act`` and is read from the stored output; Hardswish is not monotonic, so for ``out_act ==
3`` the dgrad's ``y`` operand is the stored pre-activation ``v``, which the forward writes into
``pre`` in the same pass. A zero factor gives an exact zero whatever the gradient holds.

GPU tensors run the gfx950 kernels of ``csrc/kernels/dwconv_act.hip`` (the ``tp_dwconv_hs_*`` entry
points); CPU tensors (and ``TORCHPRUNER_BACKEND=torch``) run the PyTorch bodies below in the tensors'
own dtype, which in float64 are the oracle of the kernel tests. Codes 0..2 give what
``ops.dwconv_act_*`` give, bit for bit, on both paths.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._native import require, use_native
from .dwconv_act import _act as _clamp_act
from .dwconv_act import _live, _nchw, dwconv_act_tay_slots

__all__ = ["dwconv_hs_fwd", "dwconv_hs_dgrad", "dwconv_hs_tay_slots"]

_CODES = "0 (none), 1 (ReLU), 2 (ReLU6) or 3 (Hardswish)"


def _check(code: int) -> None:
    if code not in (0, 1, 2, 3):
        raise ValueError(f"activation code {code}: {_CODES}")


def _act(code: int, t: torch.Tensor) -> torch.Tensor:
    _check(code)
    if code == 3:
        return t * torch.clamp(t + 3.0, 0.0, 6.0) / 6.0  # NaN passes through, as the clamps do
    return _clamp_act(code, t)


def _slope(code: int, t: torch.Tensor) -> torch.Tensor:
    """d act / d t as a factor; ``t`` is the pre-activation for Hardswish, and anything with the
    sign / saturation of the pre-activation (the stored output) for codes 0..2."""
    _check(code)
    one, zero = torch.ones((), dtype=t.dtype), torch.zeros((), dtype=t.dtype)
    if code == 3:
        return torch.where(t < -3.0, zero, torch.where(t <= 3.0, t / 3.0 + 0.5, one))
    return torch.where(_live(code, t), one, zero)


def dwconv_hs_tay_slots(H: int, W: int, C: int) -> int:
    """Slots R of the (R, B, C) score-partial slab of :func:`dwconv_hs_dgrad`: those of
    ``dwconv_act_tay_slots``."""
    return dwconv_act_tay_slots(H, W, C)


def dwconv_hs_fwd(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride: int, pad: int,
                  in_act: int, out_act: int, apoz: torch.Tensor | None = None,
                  pre: torch.Tensor | None = None) -> torch.Tensor:
    """x (B, H, W, C), w (C, 1, k, k), scale / shift (C) -> y (B, Ho, Wo, C); ``apoz`` (B, C)
    receives ``+= count(y > 0)`` per image and channel, ``pre`` (the shape of y) the output's
    pre-activation."""
    if use_native(x):
        return require().dwconv_hs_fwd(x, w, scale, shift, int(stride), int(pad), int(in_act), int(out_act), apoz,
                                       pre)
    _check(out_act)
    C = x.shape[3]
    v = F.conv2d(_nchw(_act(in_act, x)), w.to(x.dtype), None, stride, pad, 1, C).permute(0, 2, 3, 1)
    v = v * scale.to(x.dtype) + shift.to(x.dtype)
    y = _act(out_act, v).contiguous()
    if apoz is not None:
        apoz += (y > 0).sum((1, 2)).to(apoz.dtype)
    if pre is not None:
        if pre.shape != y.shape:
            raise ValueError("pre must have the shape of y, (B, Ho, Wo, C)")
        pre.copy_(v)
    return y


def dwconv_hs_dgrad(g: torch.Tensor, y: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, z: torch.Tensor, H: int,
                    W: int, stride: int, pad: int, in_act: int, out_act: int, tay: torch.Tensor | None = None,
                    tay_mode: int = 0) -> torch.Tensor:
    """g (unfactored dL/dy) (B, Ho, Wo, C), y the stored forward output (``out_act`` 1 / 2) or the
    stored pre-activation (``out_act`` 3), z (the forward input) (B, H, W, C) -> dz. ``tay``: a
    zeroed (``dwconv_hs_tay_slots(H, W, C)``, B, C) slab that receives the score partials (the
    reference puts the whole sum into slot 0); sum its slots, or hand it to ``ops.score_fold_``."""
    if use_native(z):
        return require().dwconv_hs_dgrad(g, y, w, scale, z, int(H), int(W), int(stride), int(pad), int(in_act),
                                         int(out_act), tay, int(tay_mode))
    _check(in_act)
    B, _, _, C = z.shape
    if tuple(z.shape[1:3]) != (H, W):
        raise ValueError("z must be (B, H, W, C)")
    zero = torch.zeros((), dtype=g.dtype)
    f = _slope(out_act, y)
    gm = torch.where(f != 0, g * scale.to(g.dtype) * f, zero)
    dA = torch.nn.grad.conv2d_input((B, C, H, W), w.to(g.dtype), _nchw(gm).contiguous(), stride, pad, 1, C)
    dA = dA.permute(0, 2, 3, 1)
    if tay is not None:
        if tay_mode not in (0, 1):
            raise ValueError("tay_mode is 0 (Taylor) or 1 (Sensitivity)")
        if tuple(tay.shape) != (dwconv_hs_tay_slots(H, W, C), B, C):
            raise ValueError("tay must be a (dwconv_hs_tay_slots(H, W, C), B, C) slab")
        term = dA.abs() if tay_mode == 1 else -(dA * _act(in_act, z))
        tay[0] += term.sum((1, 2)).to(tay.dtype)
    f = _slope(in_act, z)
    return torch.where(f != 0, dA * f, zero).contiguous()
