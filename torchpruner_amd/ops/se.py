"""Squeeze-and-excitation gates on NHWC activations, in the pieces the training path runs:

    forward   p  = se_pool(x)                        (B, C)   mean over H, W of x (B, H, W, C)
              h, s = se_gate_fwd(p, w1, b1, w2, b2)  h = relu(p w1^T + b1) (B, Cs), s = gate(h w2^T + b2) (B, C)
              out = se_scale(x, s)                   x * s[b, c]
    backward  ds = se_bwd_reduce(g, x)               (B, C)   sum over H, W of g * x
              dz2, dz1, dp = se_gate_bwd(ds, s, h, w1, w2)
                                                     dz2 = ds * gate'(s), dz1 = (dz2 w2) * [h > 0], dp = dz1 w1
              dx = se_bwd_dx(g, s, dp)               g * s[b, c] + dp[b, c] / (H W)
              db = se_wgrad(a, m, dw, want_bias)     dw[r, k] = sum_b a[b, r] m[b, k], db[r] = sum_b a[b, r]
                                                     (dW2: a = dz2, m = h; dW1: a = dz1, m = p)

``gate`` is 0 (Hardsigmoid: clamp(z + 3, 0, 6) / 6, derivative 1/6 where 0 < s < 1) or 1 (Sigmoid,
derivative s (1 - s)): both derivatives are read from the stored s, the ReLU's from the stored h.
The weights are taken in the parameters' own layout: ``(Cs, C)`` of an ``nn.Linear`` or
``(Cs, C, 1, 1)`` of a 1x1 ``nn.Conv2d``. GPU tensors run the gfx950 kernels of
``csrc/kernels/squeeze_excite.hip`` (fp32; every sum in a fixed order); CPU tensors (and
``TORCHPRUNER_BACKEND=torch``) run the PyTorch bodies below in the tensors' own dtype, which in
float64 are the oracle of the kernel tests.
"""
from __future__ import annotations

import torch

from ._native import require, use_native

__all__ = ["SE_GATES", "se_pool", "se_gate_fwd", "se_scale", "se_bwd_reduce", "se_gate_bwd", "se_bwd_dx", "se_wgrad"]

SE_GATES = {"hardsigmoid": 0, "sigmoid": 1}
SE_MAX_FC = 12288  # C + Cs of the gate kernels (their rows live in the LDS)


def _check_act(t: torch.Tensor, name: str) -> None:
    if t.dim() != 4 or t.numel() == 0:
        raise ValueError(f"{name} must be a non-empty (B, H, W, C) tensor, got {tuple(t.shape)}")


def _check_rows(t: torch.Tensor, B: int, n: int, name: str) -> None:
    if tuple(t.shape) != (B, n):
        raise ValueError(f"{name} must be ({B}, {n}), got {tuple(t.shape)}")


def _check_gate(gate: int) -> int:
    if gate not in (0, 1):
        raise ValueError(f"gate code {gate}: 0 (Hardsigmoid) or 1 (Sigmoid)")
    return int(gate)


def _fc(w: torch.Tensor, n_out: int, n_in: int, name: str) -> torch.Tensor:
    """The (out, in) matrix of an fc weight given as (out, in) or (out, in, 1, 1)."""
    if not ((w.dim() == 2 or (w.dim() == 4 and tuple(w.shape[2:]) == (1, 1))) and tuple(w.shape[:2]) == (n_out, n_in)):
        raise ValueError(f"{name} must be ({n_out}, {n_in}) or ({n_out}, {n_in}, 1, 1), got {tuple(w.shape)}")
    return w.reshape(n_out, n_in)


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


def se_pool(x: torch.Tensor) -> torch.Tensor:
    """x (B, H, W, C) -> its mean over H and W, (B, C)."""
    _check_act(x, "x")
    if use_native(x):
        return require().se_pool(_c(x))
    return x.mean((1, 2))


def se_gate_fwd(p: torch.Tensor, w1: torch.Tensor, b1, w2: torch.Tensor, b2, gate: int = 0):
    """p (B, C) -> (h (B, Cs), s (B, C))."""
    gate = _check_gate(gate)
    if p.dim() != 2 or p.numel() == 0 or w1.dim() < 2:
        raise ValueError("p must be a non-empty (B, C) tensor and w1 a (Cs, C[, 1, 1]) weight")
    (B, C), Cs = p.shape, w1.shape[0]
    m1, m2 = _fc(w1, Cs, C, "w1"), _fc(w2, C, Cs, "w2")
    for b, n, name in ((b1, Cs, "b1"), (b2, C, "b2")):
        if b is not None and tuple(b.shape) != (n,):
            raise ValueError(f"{name} must be ({n},), got {tuple(b.shape)}")
    if C + Cs > SE_MAX_FC:
        raise ValueError(f"gate widths C + Cs = {C + Cs} exceed {SE_MAX_FC}")
    if use_native(p):
        return tuple(require().se_gate_fwd(_c(p), _c(w1), _c(b1), _c(w2), _c(b2), gate))
    z1 = p @ m1.t().to(p.dtype)
    if b1 is not None:
        z1 = z1 + b1.to(p.dtype)
    h = torch.clamp(z1, min=0.0)  # NaN passes through, as nan_relu
    z2 = h @ m2.t().to(p.dtype)
    if b2 is not None:
        z2 = z2 + b2.to(p.dtype)
    s = torch.clamp(z2 + 3.0, 0.0, 6.0) / 6.0 if gate == 0 else torch.sigmoid(z2)
    return h, s


def se_scale(x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """x (B, H, W, C) * s (B, C)."""
    _check_act(x, "x")
    _check_rows(s, x.shape[0], x.shape[3], "s")
    if use_native(x):
        return require().se_scale(_c(x), _c(s))
    return x * s[:, None, None, :].to(x.dtype)


def se_bwd_reduce(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """sum over H, W of g * x, (B, C)."""
    _check_act(g, "g")
    if g.shape != x.shape:
        raise ValueError(f"g {tuple(g.shape)} and x {tuple(x.shape)} must have one shape")
    if use_native(g):
        return require().se_bwd_reduce(_c(g), _c(x))
    return (g * x).sum((1, 2))


def se_gate_bwd(ds: torch.Tensor, s: torch.Tensor, h: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, gate: int = 0):
    """ds, s (B, C), h (B, Cs) -> (dz2 (B, C), dz1 (B, Cs), dp (B, C))."""
    gate = _check_gate(gate)
    if ds.dim() != 2 or ds.numel() == 0 or h.dim() != 2:
        raise ValueError("ds must be a non-empty (B, C) tensor and h (B, Cs)")
    (B, C), Cs = ds.shape, h.shape[1]
    _check_rows(s, B, C, "s")
    _check_rows(h, B, Cs, "h")
    m1, m2 = _fc(w1, Cs, C, "w1"), _fc(w2, C, Cs, "w2")
    if C + Cs > SE_MAX_FC:
        raise ValueError(f"gate widths C + Cs = {C + Cs} exceed {SE_MAX_FC}")
    if use_native(ds):
        return tuple(require().se_gate_bwd(_c(ds), _c(s), _c(h), _c(w1), _c(w2), gate))
    if gate == 0:
        d = ((s > 0) & (s < 1)).to(ds.dtype) / 6.0
    else:
        d = s * (1.0 - s)
    dz2 = ds * d
    dz1 = (dz2 @ m2.to(ds.dtype)) * (h > 0).to(ds.dtype)
    return dz2, dz1, dz1 @ m1.to(ds.dtype)


def se_bwd_dx(g: torch.Tensor, s: torch.Tensor, dp: torch.Tensor) -> torch.Tensor:
    """g (B, H, W, C) * s (B, C) + dp (B, C) / (H W)."""
    _check_act(g, "g")
    B, H, W, C = g.shape
    _check_rows(s, B, C, "s")
    _check_rows(dp, B, C, "dp")
    if use_native(g):
        return require().se_bwd_dx(_c(g), _c(s), _c(dp))
    return g * s[:, None, None, :].to(g.dtype) + (dp.to(g.dtype) / (H * W))[:, None, None, :]


def se_wgrad(a: torch.Tensor, m: torch.Tensor, dw: torch.Tensor, want_bias: bool = False):
    """dw[r, k] = sum_b a[b, r] * m[b, k], written into ``dw`` ((R, K) or (R, K, 1, 1), any positive
    strides: the parameter's); returns db[r] = sum_b a[b, r] when asked for, else None."""
    if a.dim() != 2 or a.numel() == 0 or m.dim() != 2 or m.shape[0] != a.shape[0]:
        raise ValueError("a / m must be non-empty (B, R) / (B, K) rows")
    _fc(dw, a.shape[1], m.shape[1], "dw")
    if use_native(a):
        return require().se_wgrad(_c(a), _c(m), dw, bool(want_bias))
    dw.copy_((a.t() @ m.to(a.dtype)).reshape(dw.shape))
    return a.sum(0) if want_bias else None
