"""The squeeze-and-excitation kernels (csrc/kernels/squeeze_excite.hip) against float64 PyTorch
with derived per-element bounds, their run-to-run determinism, a MobileNetV3 training step and
Taylor attribution with the gates on the native kernels, and the TORCHPRUNER_NATIVE_SE=0 switch.

Kernel bounds. With u = 2^-24 every float32 operation adds at most u times the magnitude of its
result, so a sum is within (chain length) x u x sum|terms| of the exact value, the chain length
being the most roundings on any path from a term to the result. The bounds take the longest chain
any order of the sum can have, the number of terms n (a serial fused-multiply-add loop: one
rounding per term; the kernels' orders, registers then lanes then slots, are shorter: per-thread
terms + fold steps + the conversion, at most n for every shape here, down to one rounding for a
one-term sum), a bias counting as a term. They compose through the chain pool -> fc1 -> ReLU -> fc2
-> gate -> multiply and back: the error a stage inherits is the previous stage's bound pushed
through |W| (the stages are linear away from the kinks), plus its own n u sum|terms|. Single
operations add u each: the Hardsigmoid 2 u (|z| + 3) / 6 (its add and its divide), the Sigmoid
6 u (expf to 1 ulp = 2 u on e, the add, the divide, all on values of at most 1, derivative at most
1/4), a product u, dx = g s + dp (1 / HW) u on the sum for the fused multiply-add and 2 u more on
the dp term (the float32 1 / HW and its product). No element is excluded: the seeds are chosen so that, in float64, every fc1
pre-activation is farther than 1e-3 from 0 and every gate pre-activation farther than 1e-3 from
+-3 (test_reference_stays_clear_of_the_kinks checks that on the CPU), orders above the float32
rounding of these O(1) sums (a few 1e-7; the worst-case bounds above grow with the row length and
are far looser), so both implementations take the same branch everywhere; the GPU test asserts
that too (the same ReLU mask, the same saturated gate values).

Largest observed error / bound per quantity on an MI355X: profiles/numerics/se_kernels.txt.

Whole-model bounds are those of the existing native training tests
(test_mobilenet_gpu._compare_step: loss to 1e-4 relative, every gradient tensor to 2e-3 of its
largest entry + 1e-6), here against the same model in float64 on the library path. As there, the
BN affine parameters put every activation's input between its kinks (ReLU 0; Hardswish -3 and 3):
scale in (0.2, 0.3), shift 1.5, five standard deviations or more from each.
"""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24

# (B, H, W, C, Cs, gate code, seed): both gates, the float4 (C % 4 == 0) and the per-element path,
# one to many blocks per image, pixels split over blocks ((56, 56) at C = 16; (7, 7) at B = 1)
CASES = [
    (1, 1, 1, 4, 1, 0, 14),
    (3, 1, 1, 13, 8, 0, 0),
    (3, 3, 5, 6, 8, 0, 1),
    (3, 3, 5, 13, 1, 1, 0),
    (1, 3, 5, 100, 240, 0, 1),
    (1, 7, 7, 16, 8, 0, 1),
    (3, 7, 7, 72, 24, 0, 0),
    (1, 7, 7, 960, 240, 1, 0),
    (1, 14, 14, 100, 24, 1, 0),
    (3, 14, 14, 960, 240, 0, 18),
    (1, 56, 56, 16, 8, 0, 1),
    (3, 56, 56, 16, 8, 1, 0),
]
IDS = ["-".join(str(v) for v in c[:6]) for c in CASES]


def make_inputs(B, H, W, C, Cs, seed):
    """float32 CPU tensors, O(1): x with a per-(image, channel) offset (so the pooled value matters
    at every map size), fc weights scaled for O(1) inner pre-activations and gate pre-activations
    that spread over (-3, 3) and both saturated sides."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + Cs)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(B, H, W, C) + r(B, 1, 1, C)
    return dict(x=x, w1=(r(Cs, C) / C ** 0.5).reshape(Cs, C, 1, 1), b1=r(Cs),
                w2=(r(C, Cs) * (3.0 / Cs ** 0.5)).reshape(C, Cs, 1, 1), b2=r(C), g=r(B, H, W, C))


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64 values of every kernel output (the references of ops/se.py) and their bounds."""
    B, H, W, C, Cs, gate, seed = case
    t = {k: v.double() for k, v in make_inputs(B, H, W, C, Cs, seed).items()}
    x, g, b1, b2 = t["x"], t["g"], t["b1"], t["b2"]
    w1, w2 = t["w1"].reshape(Cs, C), t["w2"].reshape(C, Cs)
    HW = H * W
    val, bnd = {}, {}
    val["p"] = ops.se_pool(x)
    val["h"], val["s"] = ops.se_gate_fwd(val["p"], w1, b1, w2, b2, gate)
    val["out"] = ops.se_scale(x, val["s"])
    val["ds"] = ops.se_bwd_reduce(g, x)
    val["dz2"], val["dz1"], val["dp"] = ops.se_gate_bwd(val["ds"], val["s"], val["h"], w1, w2, gate)
    val["dx"] = ops.se_bwd_dx(g, val["s"], val["dp"])
    val["dw1"], val["dw2"] = torch.empty(Cs, C, dtype=torch.float64), torch.empty(C, Cs, dtype=torch.float64)
    val["db1"] = ops.se_wgrad(val["dz1"], val["p"], val["dw1"], True)
    val["db2"] = ops.se_wgrad(val["dz2"], val["h"], val["dw2"], True)
    z1 = val["p"] @ w1.t() + b1
    z2 = val["h"] @ w2.t() + b2
    p, h, s, ds, dz2, dz1, dp = (val[k] for k in ("p", "h", "s", "ds", "dz2", "dz1", "dp"))
    a1, a2 = w1.abs(), w2.abs()

    bnd["p"] = HW * U * x.abs().sum((1, 2)) / HW
    b_z1 = bnd["p"] @ a1.t() + (C + 1) * U * (p.abs() @ a1.t() + b1.abs())
    bnd["h"] = b_z1  # (the same branch of the ReLU on both sides)
    b_z2 = bnd["h"] @ a2.t() + (Cs + 1) * U * (h.abs() @ a2.t() + b2.abs())
    bnd["s"] = b_z2 / 6 + 2 * U * (z2.abs() + 3) / 6 if gate == 0 else b_z2 / 4 + 6 * U
    sb = s[:, None, None, :]
    bnd["out"] = x.abs() * bnd["s"][:, None, None, :] + U * (x * sb).abs()
    bnd["ds"] = HW * U * (g * x).abs().sum((1, 2))
    if gate == 0:
        d = ((s > 0) & (s < 1)).double() / 6
        b_d = U * d  # the float32 constant 1/6
    else:
        d = s * (1 - s)
        b_d = bnd["s"] + 2 * U * d
    bnd["dz2"] = d * bnd["ds"] + ds.abs() * b_d + bnd["ds"] * b_d + U * dz2.abs()
    live = (h > 0).double()
    bnd["dz1"] = (bnd["dz2"] @ a2 + C * U * (dz2.abs() @ a2)) * live
    bnd["dp"] = bnd["dz1"] @ a1 + Cs * U * (dz1.abs() @ a1)
    bnd["dx"] = (g.abs() * bnd["s"][:, None, None, :] + (bnd["dp"] / HW)[:, None, None, :]
                 + U * (g * sb).abs() + 3 * U * (dp.abs() / HW)[:, None, None, :])

    def outer(a, ba, m, bm):  # sum_b a[b, r] m[b, k]
        return ba.t() @ m.abs() + a.abs().t() @ bm + ba.t() @ bm + B * U * (a.abs().t() @ m.abs())

    bnd["dw1"], bnd["db1"] = outer(dz1, bnd["dz1"], p, bnd["p"]), bnd["dz1"].sum(0) + B * U * dz1.abs().sum(0)
    bnd["dw2"], bnd["db2"] = outer(dz2, bnd["dz2"], h, bnd["h"]), bnd["dz2"].sum(0) + B * U * dz2.abs().sum(0)
    return val, bnd, z1, z2


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_stays_clear_of_the_kinks(case):
    """(CPU) The chosen seeds: in float64 no fc1 pre-activation within 1e-3 of 0, no gate
    pre-activation within 1e-3 of +-3; both ReLU branches occur (one at least for Cs = 1) and, for
    the hard gate, all three regions: s exactly 0, exactly 1 and strictly in between."""
    val, bnd, z1, z2 = reference(case)
    gate, Cs = case[5], case[4]
    assert z1.abs().min() > 1e-3
    assert (z2.abs() - 3).abs().min() > 1e-3
    assert (val["h"] > 0).any() and (Cs == 1 or (val["h"] == 0).any())
    if gate == 0:
        s = val["s"]
        assert (s == 0).any() and (s == 1).any() and ((s > 0) & (s < 1)).any()
    for k, b in bnd.items():  # every quantity has a finite bound of its own shape
        assert b.shape == val[k].shape and torch.isfinite(b).all() and (b >= 0).all(), k


def _run_kernels(case, dev):
    B, H, W, C, Cs, gate, seed = case
    t = {k: v.to(dev) for k, v in make_inputs(B, H, W, C, Cs, seed).items()}
    out = {}
    out["p"] = ops.se_pool(t["x"])
    out["h"], out["s"] = ops.se_gate_fwd(out["p"], t["w1"], t["b1"], t["w2"], t["b2"], gate)
    out["out"] = ops.se_scale(t["x"], out["s"])
    out["ds"] = ops.se_bwd_reduce(t["g"], t["x"])
    out["dz2"], out["dz1"], out["dp"] = ops.se_gate_bwd(out["ds"], out["s"], out["h"], t["w1"], t["w2"], gate)
    out["dx"] = ops.se_bwd_dx(t["g"], out["s"], out["dp"])
    out["dw1"], out["dw2"] = torch.empty_like(t["w1"]), torch.empty_like(t["w2"])
    out["db1"] = ops.se_wgrad(out["dz1"], out["p"], out["dw1"], True)
    out["db2"] = ops.se_wgrad(out["dz2"], out["h"], out["dw2"], True)
    return out


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_match_fp64_within_derived_bounds(cuda, case):
    val, bnd, _, _ = reference(case)
    got = _run_kernels(case, cuda)
    again = _run_kernels(case, cuda)
    ratios = {}
    for k, want in val.items():
        a = got[k].double().cpu().reshape(want.shape)
        assert torch.isfinite(a).all(), k
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
        err = (a - want).abs()
        ratios[k] = float((err / bnd[k].clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
    print("se_kernels " + "-".join(str(v) for v in case[:6]) + " " + " ".join(f"{k}={r:.2g}" for k, r in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)
    assert torch.equal(got["h"].cpu() > 0, val["h"] > 0)  # the same branch of every ReLU
    if case[5] == 0:  # the saturated gate values are exact
        s = got["s"].cpu()
        assert torch.equal(s == 0, val["s"] == 0) and torch.equal(s == 1, val["s"] == 1)


@gpu
def test_nan_inputs_run_through(cuda):
    """The pruner's probe sends NaN channels through a switched gate: no fault, NaN out."""
    B, H, W, C, Cs = 2, 7, 7, 13, 8
    t = {k: v.to(cuda) for k, v in make_inputs(B, H, W, C, Cs, 0).items()}
    t["x"][:, :, :, 5] = float("nan")
    p = ops.se_pool(t["x"])
    h, s = ops.se_gate_fwd(p, t["w1"], t["b1"], t["w2"], t["b2"], 0)
    out = ops.se_scale(t["x"], s)
    torch.cuda.synchronize()
    assert torch.isnan(p[:, 5]).all() and not torch.isnan(p[:, :5]).any()
    assert torch.isnan(h).all() and torch.isnan(s).all() and torch.isnan(out).all()


# ------------------------------------------------------------------ whole model
def _v3(prune):
    """mobilenet_v3_small(10, small_input=True) on the CPU, dropout off (the native Philox dropout
    draws other masks than ATen's); ``prune``: every graph entry cut by 30 % + 1 random units."""
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    from torchpruner_amd.models import mobilenet_v3_small
    torch.manual_seed(0)
    model = mobilenet_v3_small(10, small_input=True)
    if prune:
        rng = np.random.RandomState(0)
        pruner = Pruner(model, (3, 32, 32), "cpu")
        for module, cascade in get_mobilenet_pruning_graph(model):
            n = module.weight.shape[0]
            pruner.prune_model(module, rng.choice(n, int(n * 0.3) + 1, replace=False), cascade)
    gen = torch.Generator().manual_seed(5)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        elif isinstance(m, torch.nn.BatchNorm2d):  # between the kinks of ReLU and Hardswish (module docstring)
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) * 0.1 + 0.2)
                m.bias.fill_(1.5)
        elif isinstance(m, torch.nn.Conv2d) and m.bias is not None:  # the gates' fcs: no symmetric start
            with torch.no_grad():
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.5)
    return model


def _gates(model):
    from torchpruner_amd import is_channel_gate
    return [m for m in model.modules() if is_channel_gate(m)]


def _batch(n=4):
    gen = torch.Generator().manual_seed(5)
    return torch.randn(n, 3, 32, 32, generator=gen), torch.randint(0, 10, (n,), generator=gen)


def _step(model, x, y, native):
    from torchpruner_amd.engine.train import native_convs
    model.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    with native_convs(model, enable=native):
        loss = F.cross_entropy(model(x), y)
        loss.backward()
    return float(loss.detach()), [x.grad.detach().double().cpu()] + [p.grad.detach().double().cpu()
                                                                      for p in model.parameters()]


def _compare_step(base, dev, hook_gate=None):
    """One training step on the native kernels against the same model in float64 on the library
    path (CPU). Returns the SE_COUNTS deltas."""
    from torchpruner_amd.engine.train import SE_COUNTS
    x, y = _batch()
    model = copy.deepcopy(base).to(dev).to(memory_format=torch.channels_last).train()
    handle = None
    if hook_gate is not None:
        handle = _gates(model)[hook_gate].fc1.register_forward_hook(lambda m, i, o: None)
    before = dict(SE_COUNTS)
    l_nat, g_nat = _step(model, x.to(dev).contiguous(memory_format=torch.channels_last), y.to(dev), True)
    delta = {k: SE_COUNTS[k] - before[k] for k in before}
    if handle is not None:
        handle.remove()
    l_ref, g_ref = _step(copy.deepcopy(base).double().train(), x.double(), y, False)
    print(f"loss native {l_nat:.7f} float64 {l_ref:.7f}")
    assert abs(l_nat - l_ref) < 1e-4 * max(1.0, abs(l_ref))
    names = ["input"] + [n for n, _ in model.named_parameters()]
    worst = 0.0
    for name, a, b in zip(names, g_nat, g_ref):
        err, lim = (a - b).abs().max().item(), 2e-3 * b.abs().max().item() + 1e-6
        worst = max(worst, err / lim)
        assert torch.isfinite(a).all() and a.shape == b.shape, name
        assert err <= lim, (name, err, lim)
    print(f"worst gradient error / bound: {worst:.3f}")
    return delta


@pytest.fixture(scope="module")
def v3_dense():
    return _v3(False)


@pytest.fixture(scope="module")
def v3_pruned():
    return _v3(True)


@gpu
def test_v3_training_step_matches_fp64(cuda, v3_dense):
    n = len(_gates(v3_dense))
    assert n == 9
    assert _compare_step(v3_dense, cuda) == {"fwd": n, "bwd": n}


@gpu
def test_pruned_v3_training_step_matches_fp64(cuda, v3_pruned):
    gates = _gates(v3_pruned)
    assert any(g.fc1.weight.shape[1] % 4 for g in gates)  # widths off the float4 path
    assert _compare_step(v3_pruned, cuda) == {"fwd": len(gates), "bwd": len(gates)}


@gpu
def test_hooked_inner_module_falls_back(cuda, v3_dense):
    """A forward hook on one gate's fc1: that gate runs its own forward (the fused one would not
    call fc1), the others stay native, the step is still right."""
    n = len(_gates(v3_dense))
    assert _compare_step(v3_dense, cuda, hook_gate=3) == {"fwd": n - 1, "bwd": n - 1}


@gpu
def test_gate_hook_still_fires_and_eval_mode_is_native(cuda, v3_dense):
    from torchpruner_amd.engine.train import SE_COUNTS, native_convs
    model = copy.deepcopy(v3_dense).to(cuda).eval()
    x = _batch()[0].to(cuda)
    seen = []
    h = _gates(model)[0].register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    with torch.no_grad():
        want = model(x)
        before = SE_COUNTS["fwd"]
        with native_convs(model, fuse=False):
            got = model(x)
    h.remove()
    assert SE_COUNTS["fwd"] - before == 9 and len(seen) == 2 and seen[0] == seen[1]
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)


@gpu
def test_taylor_on_generic_path(cuda, v3_dense):
    """Taylor scores of every graph entry on the generic path (gates on the native kernels) against
    the same metric with TORCHPRUNER_BACKEND=torch in float64 on the CPU, within the bound of
    test_mobilenet_gpu.test_pruned_mobilenet_taylor_on_generic_path (1e-4 of the largest score)."""
    from torchpruner_amd import TaylorAttributionMetric, get_mobilenet_pruning_graph
    from torchpruner_amd.data import DeviceLoader
    from torchpruner_amd.engine.train import SE_COUNTS
    x, y = _batch(16)
    base = copy.deepcopy(v3_dense)
    with torch.no_grad():  # eval-mode statistics = this batch's, so the BN outputs stay between the kinks
        for m in base.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.momentum = 1.0
        base.train()(x)
    base.eval()
    model = copy.deepcopy(base).to(cuda)
    mods = [m for m, _ in get_mobilenet_pruning_graph(model)]
    before = SE_COUNTS["fwd"]
    metric = TaylorAttributionMetric(model, DeviceLoader(x.to(cuda), y.to(cuda), 8), F.cross_entropy, cuda)
    got = metric.run_many(mods, find_best_evaluation_module=True)
    assert metric.last_path["path"] == "generic", metric.last_path
    assert SE_COUNTS["fwd"] - before >= 2 * 9
    m64 = copy.deepcopy(base).double()
    mods64 = [m for m, _ in get_mobilenet_pruning_graph(m64)]
    os.environ["TORCHPRUNER_BACKEND"] = "torch"
    try:
        ref = TaylorAttributionMetric(m64, DeviceLoader(x.double(), y, 8), F.cross_entropy, "cpu").run_many(
            mods64, find_best_evaluation_module=True)
    finally:
        del os.environ["TORCHPRUNER_BACKEND"]
    assert len(got) == len(ref) == 10
    for mod, a, e in zip(mods, got, ref):
        assert a.shape == e.shape == (mod.out_channels,)
        err = np.abs(a - e).max() / (np.abs(e).max() + 1e-30)
        print(f"{mod.out_channels} channels: rel. error {err:.3e}")
        assert err < 1e-4


def _ab_child():
    """(child process, TORCHPRUNER_NATIVE_SE=0) the step still matches and no gate kernel ran."""
    from torchpruner_amd.engine import train
    ops.require()
    assert not train._NATIVE_SE
    assert _compare_step(_v3(False), torch.device("cuda")) == {"fwd": 0, "bwd": 0}
    assert train.SE_COUNTS == {"fwd": 0, "bwd": 0}
    print("se switch off ok")


@gpu
def test_native_se_switch_off_keeps_library_path(cuda):
    env = dict(os.environ, TORCHPRUNER_NATIVE_SE="0")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            "import test_se_gpu as t; t._ab_child()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "se switch off ok" in r.stdout
