"""Gates with a SiLU inner activation (ops.se_gate_act_fwd / se_gate_act_bwd, act = 1) against the ops' PyTorch
bodies in float64. Cases: both gates, the float4 and the per-element path, Cs = 1, a row longer than one
lane group. Tolerance per quantity: 16 x the largest float32 error of the PyTorch body on the CPU over the
cases (summation orders, a few ulp between expf implementations), floor 1e-6 * max|reference|; a wrong
derivative gives errors of order 1. Measured on an MI355X: profiles/numerics/se_silu.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_se_gpu import make_inputs
from torchpruner_amd import ops

CASES = [(1, 1, 1, 4, 1, 1), (3, 3, 5, 13, 8, 1), (1, 7, 7, 960, 240, 1), (3, 14, 14, 100, 24, 0)]
NAMES = ("h", "z1", "s", "dz2", "dz1", "dp")


def _chain(case, dtype, dev="cpu", act=1):
    B, H, W, C, Cs, gate = case
    t = {k: v.to(dtype).to(dev) for k, v in make_inputs(B, H, W, C, Cs, 3).items()}
    p, ds = ops.se_pool(t["x"]), ops.se_bwd_reduce(t["g"], t["x"])
    h, z1, s = ops.se_gate_act_fwd(p, t["w1"], t["b1"], t["w2"], t["b2"], gate, act)
    return dict(zip(NAMES, (h, z1, s, *ops.se_gate_act_bwd(ds, s, h, z1, t["w1"], t["w2"], gate, act)))), t, (p, ds)


@functools.lru_cache(maxsize=None)
def reference(case):
    return _chain(case, torch.float64)[0]


@functools.lru_cache(maxsize=None)
def bounds():
    """name -> (largest float32 CPU error of the PyTorch body over the cases, largest |reference|)."""
    err = lambda c, n: float((_chain(c, torch.float32)[0][n].double() - reference(c)[n]).abs().max())
    return {n: (max(err(c, n) for c in CASES), max(float(reference(c)[n].abs().max()) for c in CASES)) for n in NAMES}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_torch_bodies_match_autograd(case):
    """(CPU) the float64 bodies against autograd through x * gate(fc2(silu(fc1(pool(x)))))."""
    B, H, W, C, Cs, gate = case
    t = {k: v.double() for k, v in make_inputs(B, H, W, C, Cs, 3).items()}
    x = t["x"].clone().requires_grad_(True)
    z1 = F.linear(x.mean((1, 2)), t["w1"].reshape(Cs, C), t["b1"])
    z2 = F.linear(F.silu(z1), t["w2"].reshape(C, Cs), t["b2"])
    # (Hardsigmoid written out: ATen's backward multiplies by a float32 1 / 6 even in float64)
    s = torch.clamp(z2 + 3.0, 0.0, 6.0) / 6.0 if gate == 0 else torch.sigmoid(z2)
    dz1, dz2, dx = torch.autograd.grad(((x * s[:, None, None, :]) * t["g"]).sum(), (z1, z2, x))
    ref = reference(case)
    for name, want in (("z1", z1), ("h", F.silu(z1)), ("s", s), ("dz2", dz2), ("dz1", dz1)):
        torch.testing.assert_close(ref[name], want.detach(), rtol=1e-11, atol=1e-11, msg=name)
    torch.testing.assert_close(ops.se_bwd_dx(t["g"], ref["s"], ref["dp"]), dx, rtol=1e-11, atol=1e-11)  # dp


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_silu_gate_matches_fp64(cuda, case):
    got, ref = _chain(case, torch.float32, cuda)[0], reference(case)
    for name in NAMES:
        err32, big = bounds()[name]
        bound = max(16 * err32, 1e-6 * big)
        err = float((got[name].double().cpu() - ref[name]).abs().max())
        print(f"se_silu {case} {name}: fp32 body error {err32:.3g} bound {bound:.3g} kernel error {err:.3g}")
        assert torch.isfinite(got[name]).all() and err <= bound, (name, err, bound)
    assert all(torch.equal(v, got[n]) for n, v in _chain(case, torch.float32, cuda)[0].items())  # deterministic


@pytest.mark.gpu
def test_relu_entry_points_are_unchanged(cuda):
    """act = 0 of the new entry point is se_gate_fwd / se_gate_bwd bit for bit (z1 is empty)."""
    case = CASES[1]
    got, t, (p, ds) = _chain(case, torch.float32, cuda, act=0)
    h, s = ops.se_gate_fwd(p, t["w1"], t["b1"], t["w2"], t["b2"], case[5])
    want = dict(zip(("h", "s", "dz2", "dz1", "dp"), (h, s, *ops.se_gate_bwd(ds, s, h, t["w1"], t["w2"], case[5]))))
    assert got["z1"].numel() == 0 and all(torch.equal(got[k], v) for k, v in want.items())
