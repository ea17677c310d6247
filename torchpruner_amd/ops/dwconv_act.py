"""Depthwise convolution with the activations on both sides and the BN affine fused (the hidden
layer of an eval-mode MobileNet inverted-residual block), NHWC:

    forward  y  = out_act(scale[c] * dwconv(in_act(x))[c] + shift[c])        (+ APoZ counts)
    dgrad    dA = dwconv^T(mask_out(y) * g * scale[c])     (dL/d in_act(z), unmasked)
             tay += per-(image, channel) sums of -(dA * in_act(z)) (tay_mode 0) or |dA| (1)
             dz = mask_in(z) * dA

Activation codes are those of ``bn_train_fwd(act=)``: 0 none, 1 ReLU, 2 ReLU6. GPU tensors run the
gfx950 kernels of ``csrc/kernels/dwconv_act.hip``; CPU tensors (and ``TORCHPRUNER_BACKEND=torch``)
run the PyTorch bodies below in the tensors' own dtype, which in float64 are the oracle of the
kernel tests. Masks follow ``hardtanh_backward``: zero gradient at exactly 0 and exactly 6.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._native import require, use_native

__all__ = ["dwconv_act_fwd", "dwconv_act_dgrad", "dwconv_act_tay_slots"]

_SW = 4  # columns per thread of the kernels (DW_SW)


def _act(code: int, t: torch.Tensor) -> torch.Tensor:
    if code == 0:
        return t
    if code == 1:
        return torch.clamp(t, min=0.0)  # NaN passes through, as nan_relu
    if code == 2:
        return torch.clamp(t, 0.0, 6.0)
    raise ValueError(f"activation code {code}: 0 (none), 1 (ReLU) or 2 (ReLU6)")


def _live(code: int, t: torch.Tensor) -> torch.Tensor:
    """Where the activation passes the gradient (hardtanh_backward / threshold_backward: zero where
    t <= 0 or t >= 6, passed everywhere else, NaN included)."""
    if code == 0:
        return torch.ones_like(t, dtype=torch.bool)
    if code == 1:
        return ~(t <= 0)
    if code == 2:
        return ~((t <= 0) | (t >= 6))
    raise ValueError(f"activation code {code}: 0 (none), 1 (ReLU) or 2 (ReLU6)")


def dwconv_act_tay_slots(H: int, W: int, C: int) -> int:
    """Slots R of the (R, B, C) score-partial slab :func:`dwconv_act_dgrad` takes for (H, W, C)
    inputs: one per (input row, 256-wide slice of the row's 4-column strips x channel quads)."""
    if H < 1 or W < 1 or C < 4 or C % 4:
        return 0
    q = -(-W // _SW) * (C // 4)
    r = H * (-(-q // 256))
    return r if r < (1 << 24) else 0


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def dwconv_act_fwd(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride: int, pad: int,
                   in_act: int, out_act: int, apoz: torch.Tensor | None = None) -> torch.Tensor:
    """x (B, H, W, C), w (C, 1, k, k), scale / shift (C) -> y (B, Ho, Wo, C); ``apoz`` (B, C)
    receives ``+= count(y > 0)`` per image and channel."""
    if use_native(x):
        return require().dwconv_act_fwd(x, w, scale, shift, int(stride), int(pad), int(in_act), int(out_act), apoz)
    C = x.shape[3]
    pre = F.conv2d(_nchw(_act(in_act, x)), w.to(x.dtype), None, stride, pad, 1, C).permute(0, 2, 3, 1)
    y = _act(out_act, pre * scale.to(x.dtype) + shift.to(x.dtype)).contiguous()
    if apoz is not None:
        apoz += (y > 0).sum((1, 2)).to(apoz.dtype)
    return y


def dwconv_act_dgrad(g: torch.Tensor, y: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, z: torch.Tensor, H: int,
                     W: int, stride: int, pad: int, in_act: int, out_act: int, tay: torch.Tensor | None = None,
                     tay_mode: int = 0) -> torch.Tensor:
    """g (unmasked dL/dy) and y (the stored forward output) (B, Ho, Wo, C), z (the forward input)
    (B, H, W, C) -> dz. ``tay``: a zeroed (``dwconv_act_tay_slots(H, W, C)``, B, C) slab that
    receives the score partials (the reference puts the whole sum into slot 0); sum its slots, or
    hand it to ``ops.score_fold_``."""
    if use_native(z):
        return require().dwconv_act_dgrad(g, y, w, scale, z, int(H), int(W), int(stride), int(pad), int(in_act),
                                          int(out_act), tay, int(tay_mode))
    B, _, _, C = z.shape
    if tuple(z.shape[1:3]) != (H, W):
        raise ValueError("z must be (B, H, W, C)")
    gm = torch.where(_live(out_act, y), g * scale.to(g.dtype), torch.zeros((), dtype=g.dtype))
    dA = torch.nn.grad.conv2d_input((B, C, H, W), w.to(g.dtype), _nchw(gm).contiguous(), stride, pad, 1, C)
    dA = dA.permute(0, 2, 3, 1)
    if tay is not None:
        if tay_mode not in (0, 1):
            raise ValueError("tay_mode is 0 (Taylor) or 1 (Sensitivity)")
        if tuple(tay.shape) != (dwconv_act_tay_slots(H, W, C), B, C):
            raise ValueError("tay must be a (dwconv_act_tay_slots(H, W, C), B, C) slab")
        term = dA.abs() if tay_mode == 1 else -(dA * _act(in_act, z))
        tay[0] += term.sum((1, 2)).to(tay.dtype)
    return torch.where(_live(in_act, z), dA, torch.zeros((), dtype=dA.dtype)).contiguous()
