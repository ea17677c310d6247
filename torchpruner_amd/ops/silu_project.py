"""SiLU-on-load 1x1 project GEMM of a Fused-MBConv block (dense 3x3 expand, BN, SiLU, 1x1 project, BN) and
its data gradient. The hidden tensor is kept as the pre-activation ``z`` (N, C), N = B * hw rows (NHWC
flattened); the consumer activates it as it reads it:

    forward  out = (silu(z) @ wt) * scale + shift (+ res)          wt (C, Co), res / out (N, Co)
             apoz (B, C) += per-image counts of silu(z) > 0
    dgrad    gy = g @ wtT,  dz = gy * silu'(z)                     g (N, Co), wtT (Co, C)
             tay (R, B, C) += per-image sums of -(gy * silu(z)) (tay_mode 0) or |gy| (1)

GPU float32 operands run the gfx950 kernels of ``csrc/kernels/silu_project.hip`` (fp32 MFMA; the activated
tensor and ``gy`` never reach memory; ``Co <= 128`` in the forward); other operands run the PyTorch bodies
below in their own dtype, which in float64 are the oracle of the kernel tests. The slab has one slot per row
tile an image can meet; the bodies put the whole sum into slot 0.
"""
from __future__ import annotations

import torch

from ._native import require, use_native

__all__ = ["silu_project_fwd", "silu_project_dgrad", "silu_project_tay_slots"]

SILU_PROJECT_MAX_CO = 128  # the forward kernel's output width (four 32-column accumulators per wave)


def _silu_both(z: torch.Tensor):
    s = torch.sigmoid(z)
    return z * s, s * (1.0 + z * (1.0 - s))


def silu_project_tay_slots(hw: int, C: int) -> int:
    """Slots R of :func:`silu_project_dgrad`'s (R, B, C) slab for images of ``hw`` rows: the 64-row tiles an
    image can meet (it starts at a multiple of g = gcd(hw, 64) inside its first tile); 0 for a rejected shape."""
    if hw < 1 or C < 4 or C % 4:
        return 0
    return (hw - min(hw & -hw, 64) + 63) // 64 + 1


def _check(N, C, Co, what):
    if N < 1 or C % 4 or Co % 4 or C < 4 or Co < 4:
        raise ValueError(f"{what}: needs rows and C, Co multiples of 4, got N {N}, C {C}, Co {Co}")


def silu_project_fwd(z: torch.Tensor, wt: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, res=None,
                     apoz=None) -> torch.Tensor:
    """(N, Co) output; ``apoz``: a (B, C) tensor, B dividing N, that receives ``+=`` the counts."""
    if z.dim() != 2 or wt.dim() != 2 or wt.shape[0] != z.shape[1] or scale.shape != (wt.shape[1],) or \
            shift.shape != scale.shape or (res is not None and tuple(res.shape) != (z.shape[0], wt.shape[1])) or \
            (apoz is not None and (apoz.dim() != 2 or apoz.shape[1] != z.shape[1] or z.shape[0] % apoz.shape[0])):
        raise ValueError("silu_project_fwd: expected z (N, C), wt (C, Co), scale / shift (Co,), res (N, Co), apoz (B, C)")
    _check(z.shape[0], z.shape[1], wt.shape[1], "silu_project_fwd")
    if use_native(z) and z.dtype == torch.float32:
        return require().silu_project_fwd(z, wt, scale, shift, res, apoz)
    a = _silu_both(z)[0]
    out = (a @ wt.to(z.dtype)) * scale.to(z.dtype) + shift.to(z.dtype)
    if res is not None:
        out = out + res.to(z.dtype)
    if apoz is not None:
        apoz += (a > 0).view(apoz.shape[0], -1, z.shape[1]).sum(1).to(apoz.dtype)
    return out


def silu_project_dgrad(g: torch.Tensor, z: torch.Tensor, wtT: torch.Tensor, tay=None, tay_mode: int = 0) -> torch.Tensor:
    """(N, C) gradient of the pre-activation; ``tay``: a zeroed (``silu_project_tay_slots(N // B, C)``, B, C)
    slab that receives the score partials (sum its slots, or hand it to ``ops.score_fold_``)."""
    if z.dim() != 2 or g.dim() != 2 or wtT.dim() != 2 or g.shape[0] != z.shape[0] or \
            tuple(wtT.shape) != (g.shape[1], z.shape[1]):
        raise ValueError("silu_project_dgrad: expected g (N, Co), z (N, C), wtT (Co, C)")
    N, C = z.shape
    _check(N, C, g.shape[1], "silu_project_dgrad")
    if tay is not None:
        if tay_mode not in (0, 1):
            raise ValueError("tay_mode is 0 (Taylor) or 1 (Sensitivity)")
        if tay.dim() != 3 or tay.shape[2] != C or N % tay.shape[1] or \
                tay.shape[0] != silu_project_tay_slots(N // tay.shape[1], C):
            raise ValueError(f"tay must be a (silu_project_tay_slots, B, {C}) slab, got {tuple(tay.shape)}")
    if use_native(z) and z.dtype == torch.float32:
        return require().silu_project_dgrad(g, z, wtT, tay, int(tay_mode))
    a, d = _silu_both(z)
    gy = g.to(z.dtype) @ wtT.to(z.dtype)
    if tay is not None:
        term = gy.abs() if tay_mode == 1 else -(gy * a)
        tay[0] += term.view(tay.shape[1], -1, C).sum(1).to(tay.dtype)
    return gy * d
