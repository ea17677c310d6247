"""SiLU prefix-scan 1x1 project GEMM: the ``cnt`` stacked outputs of a Fused-MBConv block (dense 3x3 expand,
BN, SiLU, 1x1 project, BN) whose expand SiLU is masked by the prefixes p0 .. p0 + cnt - 1 of a permutation,

    out[j, n, :] = sum_c [rank[c] >= p0 + j] * silu(z[n, c]) * wt[c, :] + shift (+ res[n, :])

with the stored pre-activation ``z`` (N, C), ``wt`` (C, Co) (BN scale folded in), ``shift`` (Co,), ``res``
(N, Co) or None, ``perm`` int32 (n,) over the real channels and ``rank`` int32 (C,) its rank vector over the
padded width (padding ranks after every real channel). It is what ``EfficientNetEngine.prefix_logits`` needs
at a fused block: copy j + 1 is copy j minus the one channel ``perm[p0 + j]``. GPU float32 operands run the
gfx950 kernel of ``csrc/kernels/silu_prefix_project.hip`` (a masked fp32-MFMA GEMM whose accumulators stay in
registers for the cnt - 1 rank-1 steps; neither silu(z) nor a base tensor reaches memory; ``Co <= 128``);
other operands run the PyTorch body below in their own dtype, which in float64 is the oracle of the kernel
test. The body reads ``rank`` only; the kernel walks ``perm``, which must be the permutation ``rank`` ranks.
"""
from __future__ import annotations

import torch

from ._native import require, use_native

__all__ = ["silu_prefix_project"]


def silu_prefix_project(z: torch.Tensor, wt: torch.Tensor, shift: torch.Tensor, res, perm: torch.Tensor,
                        rank: torch.Tensor, p0: int, cnt: int) -> torch.Tensor:
    """(cnt, N, Co) outputs; ``C % 4 == 0``, ``Co % 4 == 0`` and ``p0 + cnt - 1 <= n``."""
    p0, cnt = int(p0), int(cnt)
    if z.dim() != 2 or wt.dim() != 2 or wt.shape[0] != z.shape[1] or shift.shape != (wt.shape[1],) or \
            (res is not None and tuple(res.shape) != (z.shape[0], wt.shape[1])) or perm.dim() != 1 or \
            tuple(rank.shape) != (z.shape[1],):
        raise ValueError("silu_prefix_project: expected z (N, C), wt (C, Co), shift (Co,), res (N, Co), perm (n,), "
                         "rank (C,)")
    (N, C), Co, n = z.shape, wt.shape[1], perm.numel()
    if N < 1 or C % 4 or Co % 4 or C < 4 or Co < 4 or n > C or cnt < 1 or p0 < 0 or p0 + cnt - 1 > n:
        raise ValueError(f"silu_prefix_project: bad arguments (N {N}, C {C}, Co {Co}, n {n}, p0 {p0}, cnt {cnt})")
    if use_native(z) and z.dtype == torch.float32:
        return require().silu_prefix_project(z.contiguous(), wt.float().contiguous(), shift.float().contiguous(),
                                             None if res is None else res.float().contiguous(),
                                             perm.to(torch.int32).contiguous(), rank.to(torch.int32).contiguous(),
                                             p0, cnt)
    lim = torch.arange(p0, p0 + cnt, device=z.device, dtype=rank.dtype).view(cnt, 1, 1)
    a = torch.where(rank.view(1, 1, C) >= lim, z * torch.sigmoid(z), torch.zeros((), dtype=z.dtype, device=z.device))
    out = a @ wt.to(z.dtype) + shift.to(z.dtype)
    return out if res is None else out + res.to(z.dtype)
