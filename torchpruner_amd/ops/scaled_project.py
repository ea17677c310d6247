"""Channel-scaled 1x1 project GEMM: the ``cnt`` stacked outputs of a linear 1x1 conv whose input copies
are ONE activation ``a`` under per-(copy, image, channel) scales,

    out[j, n, :] = (a[n, :] * sc[j, n // hw, :]) @ wt + bias[j, n // hw, :] (+ res[n, :])

with ``a`` (N, C), ``sc`` (cnt, B, C), ``wt`` (C, Co), ``bias`` (cnt, B, Co), ``res`` (N, Co) or None and
N = B * hw. It is what the prefix copies of a gated inverted-residual block reduce to
(``MobileNetV3Engine.prefix_logits``): a masked channel has scale 0 and its constant contribution sits in
the bias, an unmasked one is scaled by the copy's gate. GPU float32 operands run the gfx950 kernel of
``csrc/kernels/scaled_project.hip`` (fp32 MFMA; ``a`` is staged once for four copies, the scaled copies
never exist); other operands run the PyTorch body below in their own dtype, which in float64 is the
oracle of the kernel test.
"""
from __future__ import annotations

import torch

from ._native import require, use_native

__all__ = ["scaled_project"]


def scaled_project(a: torch.Tensor, sc: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, res=None,
                   hw: int = 1) -> torch.Tensor:
    """(cnt, N, Co) outputs; ``C % 4 == 0`` and ``Co % 4 == 0``."""
    hw = int(hw)
    if a.dim() != 2 or sc.dim() != 3 or wt.dim() != 2 or bias.dim() != 3:
        raise ValueError("scaled_project: expected a (N, C), sc (cnt, B, C), wt (C, Co), bias (cnt, B, Co)")
    (N, C), (cnt, B, _), Co = a.shape, sc.shape, wt.shape[1]
    if hw < 1 or B * hw != N or cnt < 1 or N < 1 or sc.shape[2] != C or wt.shape[0] != C or \
            tuple(bias.shape) != (cnt, B, Co) or (res is not None and tuple(res.shape) != (N, Co)):
        raise ValueError(f"scaled_project: shapes do not chain (a {tuple(a.shape)}, sc {tuple(sc.shape)}, wt "
                         f"{tuple(wt.shape)}, bias {tuple(bias.shape)}, hw {hw})")
    if C % 4 or Co % 4:
        raise ValueError(f"scaled_project: C {C} and Co {Co} must be multiples of 4")
    if use_native(a) and a.dtype == torch.float32:
        return require().scaled_project(a.contiguous(), sc.float().contiguous(), wt.float().contiguous(),
                                        bias.float().contiguous(), None if res is None else res.float().contiguous(),
                                        hw)
    scaled = a.reshape(1, B, hw, C) * sc.to(a.dtype).reshape(cnt, B, 1, C)
    out = scaled @ wt.to(a.dtype) + bias.to(a.dtype).reshape(cnt, B, 1, Co)
    if res is not None:
        out = out + res.to(a.dtype).reshape(1, B, hw, Co)
    return out.reshape(cnt, N, Co)
