"""Shapley values on the MobileNet engine: the prefix-scan project kernel against its fp64 body, the
stacked prefix logits of every evaluation module against the module forward with a masking hook, and
the metric end to end against the fp64 hook path.

Measured on an MI355X (profiles/numerics/mobilenet_shapley_engine.txt): kernel error at most 0.31 of
its derived bound; stacked logits within 1.1e-6; Shapley values within 1.6e-4 of the reference's
maximum (bound 2e-2)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ kernel
def _kernel_case(N, C, Co, zero_fill, cuda):
    g = torch.Generator().manual_seed(N * 1000 + C + Co)
    n = C - 7
    a = torch.rand(N, C, generator=g) * 6
    fill = torch.zeros(C) if zero_fill else torch.rand(C, generator=g) * 6
    hit = torch.rand(N, C, generator=g) < 0.1
    a = torch.where(hit, fill.view(1, C).expand(N, C), a)  # some entries exactly at their fill: a zero delta
    wt = torch.randn(C, Co, generator=g)
    base = torch.randn(N, Co, generator=g) * 3
    perm = torch.randperm(n, generator=g).to(torch.int32)
    return [t.to(cuda) for t in (base, a, fill, wt, perm)], n


@pytest.mark.parametrize("zero_fill", [True, False], ids=["fill0", "fill"])
@pytest.mark.parametrize("Co", [32, 96])
@pytest.mark.parametrize("N,C", [(50, 64), (147, 160), (50, 160), (147, 64)])
def test_prefix_project_kernel_matches_fp64(cuda, N, C, Co, zero_fill):
    """|out[j] - ref| <= 3 j 2^-23 (|base| + sum_{i<j} |d_i wt_i|) elementwise: one rounding each for
    the difference, the product and the accumulate per step (derived, not measured); cnt = 1 returns
    base itself; two launches agree bit for bit."""
    from torchpruner_amd import ops
    (base, a, fill, wt, perm), n = _kernel_case(N, C, Co, zero_fill, cuda)
    b64, a64, f64, w64 = (t.double().cpu() for t in (base, a, fill, wt))
    worst = 0.0
    for cnt in (1, 2, 7, 33):
        for p0 in (0, 1, n - cnt + 1):
            out = ops.prefix_project(base, a, fill, wt, perm, p0, cnt)
            assert out.shape == (cnt, N, Co) and out.dtype == torch.float32 and out.is_cuda
            assert torch.equal(out[0], base)
            assert torch.equal(out, ops.prefix_project(base, a, fill, wt, perm, p0, cnt))
            ref = ops.prefix_project(b64, a64, f64, w64, perm.cpu(), p0, cnt)
            mag = b64.abs().clone()
            cols = perm.cpu().long()[p0:p0 + cnt - 1]
            got = out.double().cpu()
            for j in range(1, cnt):
                c = cols[j - 1]
                mag += ((a64[:, c] - f64[c]).unsqueeze(1) * w64[c].unsqueeze(0)).abs()
                bound = 3 * j * 2.0 ** -23 * mag
                err = (got[j] - ref[j]).abs()
                assert (err <= bound).all(), (cnt, p0, j, float((err / bound.clamp_min(1e-300)).max()))
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"prefix_project N={N} C={C} Co={Co}: worst error / bound = {worst:.3f}")


def test_prefix_project_spans_blocks_and_lds_tiles(cuda):
    """More steps than one LDS tile holds, a width whose float4 count does not divide a block's
    (Co = 36) and one that exceeds it (Co = 1040), one float4 per pixel row (Co = 4), and both sides of
    the launcher's switch from 64-float4 blocks (below 512 * 256 float4s per copy) to 256-float4 ones,
    the latter also with Co = 36 and with three LDS tiles of steps (Co = 4: 256 pixel rows per block,
    16 steps per tile): against the fp64 body."""
    from torchpruner_amd import ops
    for N, C, Co, cnt in ((37, 320, 36, 300), (5, 40, 1040, 9), (600, 32, 4, 20), (8191, 32, 64, 4),
                          (8192, 32, 64, 4), (14600, 40, 36, 5), (131100, 64, 4, 40)):
        g = torch.Generator().manual_seed(Co)
        a, fill, wt = torch.rand(N, C, generator=g), torch.rand(C, generator=g), torch.randn(C, Co, generator=g)
        base, perm = torch.randn(N, Co, generator=g), torch.randperm(C, generator=g).to(torch.int32)
        out = ops.prefix_project(base.to(cuda), a.to(cuda), fill.to(cuda), wt.to(cuda), perm.to(cuda), 3, cnt)
        ref = ops.prefix_project(base.double(), a.double(), fill.double(), wt.double(), perm, 3, cnt)
        mag = base.double().abs() + ((a.double() - fill.double()).abs()[:, perm.long()[3:3 + cnt - 1]]
                                     @ wt.double().abs()[perm.long()[3:3 + cnt - 1]])
        assert ((out.double().cpu() - ref).abs() <= 3 * cnt * 2.0 ** -23 * mag).all()


def test_prefix_project_binding_rejects(cuda):
    from torchpruner_amd import ops
    T = ops.require()
    (base, a, fill, wt, perm), n = _kernel_case(50, 64, 32, False, cuda)
    for args in ((base, a, fill, wt, perm, 0, 0), (base, a, fill, wt, perm, -1, 2), (base, a, fill, wt, perm, n, 2),
                 (base, a, fill, wt, perm.long(), 0, 2), (base, a[:49], fill, wt, perm, 0, 2),
                 (base, a, fill[:63], wt, perm, 0, 2), (base, a, fill, wt[:, :28].contiguous(), perm, 0, 2),
                 (base[:, :30].contiguous(), a, fill, wt[:, :30].contiguous(), perm, 0, 2),
                 (base.cpu(), a, fill, wt, perm, 0, 2)):
        with pytest.raises(RuntimeError):
            T.prefix_project(*args)


# ------------------------------------------------------------------ engine
_SETUP = {}


@pytest.fixture
def setup(cuda):
    """The pruned live-BN MobileNetV2 of test_mobilenet_engine_gpu.py, its engine, a float64 CPU copy
    and 6 images, built once for the module."""
    if not _SETUP:
        from test_mobilenet_engine_gpu import _live_bn_model
        from test_mobilenet_gpu import _pruned_mobilenet
        from torchpruner_amd.engine import maybe_mobilenet_engine
        model, x, y = _live_bn_model(_pruned_mobilenet())
        m64 = copy.deepcopy(model).double()
        model = model.to(cuda)
        eng = maybe_mobilenet_engine(model, [], cuda)
        assert eng is not None
        _SETUP.update(model=model, m64=m64, x=x[:6].to(cuda), y=y[:6].to(cuda), eng=eng, ref={})
    return _SETUP


def _hooked_logits(s, idx, rank, p0, cnt):
    """float64 CPU logits (cnt * B, classes) of the module forward with evaluation module ``idx``'s
    output channels of rank < p0 + j zeroed in copy j."""
    from torchpruner_amd.engine.mobilenet_engine import MobileNetEngine, build_mobilenet_plan
    m64 = s["m64"]
    mod = MobileNetEngine(m64, build_mobilenet_plan(m64)[0]).eval_modules()[idx]
    x = s["x"].double().cpu()
    outs = []
    for j in range(cnt):
        keep = (rank >= p0 + j).view(1, -1, 1, 1)
        h = mod.register_forward_hook(lambda _m, _i, o, keep=keep: torch.where(keep, o, torch.zeros((), dtype=o.dtype)))
        try:
            with torch.no_grad():
                outs.append(m64(x))
        finally:
            h.remove()
    return torch.cat(outs, 0)


@pytest.mark.parametrize("delta", ["1", "0"], ids=["prefix_project", "masked_copies"])
def test_prefix_logits_match_the_hooked_module(setup, monkeypatch, delta):
    """All 33 evaluation modules (16 post-expand, 17 post-depthwise: the expand-less first block,
    shortcut, stride-2 and last blocks), one chunk of 5 prefixes from the middle of a seeded
    permutation: rtol = atol = 2e-3 against the float64 module forward with a masking hook, with the
    prefix-scan kernel and with TORCHPRUNER_PREFIX_DELTA=0 (masked copies through the project conv).

    Measured on an MI355X: worst |logit error| 9.5e-7 to 1.04e-6 over three runs, the same on either
    path (logits of magnitude ~1; the tuner's conv choices differ between runs)."""
    s = setup
    eng = s["eng"]
    monkeypatch.setenv("TORCHPRUNER_PREFIX_DELTA", delta)
    mods = eng.eval_modules()
    kinds = [eng.locate(m) for m in mods]
    assert len(mods) == 33 and sum(k == "expand" for _, k in kinds) == 16 and kinds[0] == (0, "dw")
    assert any(eng.plan.blocks[bi].shortcut for bi, _ in kinds) and any(
        eng.plan.blocks[bi].dw.conv.stride[0] == 2 for bi, _ in kinds)
    cnt, worst = 5, 0.0
    for idx, (m, (bi, kind)) in enumerate(zip(mods, kinds)):
        n = eng.real_width(m)
        perm = torch.from_numpy(np.random.RandomState(idx).permutation(n))
        rank = torch.empty(n, dtype=torch.long)
        rank[perm] = torch.arange(n)
        p0 = n // 2 - 2
        if (idx, p0) not in s["ref"]:
            s["ref"][(idx, p0)] = _hooked_logits(s, idx, rank, p0, cnt)
        ref = s["ref"][(idx, p0)]
        with torch.no_grad():
            h, y = eng.forward_to(s["x"], bi)
            cp = y.shape[3]
            rank_p = torch.cat([rank, torch.full((cp - n,), n + 1)]).to(torch.int32).to(y.device)
            got = eng.prefix_logits(bi, kind, h, y, perm.to(torch.int32).to(y.device), rank_p, p0, cnt)
        assert got.shape == ref.shape == (cnt * 6, 10)
        worst = max(worst, float((got.double().cpu() - ref).abs().max()))
        torch.testing.assert_close(got.double().cpu(), ref, rtol=2e-3, atol=2e-3, msg=lambda t: f"{idx} {kind}: {t}")
        # the chunk's copies differ from one another (four more masked channels move an early
        # block's logits by ~1e-5 only: what the end-to-end test excludes those blocks for)
        assert (ref[:6] - ref[-6:]).abs().max() > 1e-7
    print(f"prefix logits (TORCHPRUNER_PREFIX_DELTA={delta}): worst abs error {worst:.3e}")


# ------------------------------------------------------------------ metric
def _mse_one_hot(out, y, reduction="mean"):
    return F.mse_loss(out, F.one_hot(y, out.shape[1]).to(out.dtype), reduction=reduction)


def _shapley(model, module, x, y, device, backend, criterion=F.cross_entropy, reduction="none", **kw):
    from torchpruner_amd import ShapleyAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    os.environ["TORCHPRUNER_BACKEND"] = backend
    try:
        np.random.seed(7)
        metric = ShapleyAttributionMetric(model, DeviceLoader(x, y, 3), criterion, device, sv_samples=2,
                                          reduction=reduction, **kw)
        return metric.run(module, find_best_evaluation_module=True), metric
    finally:
        del os.environ["TORCHPRUNER_BACKEND"]


def _targets(model):
    """(name, conv whose evaluation module is scored): the last block's post-expand and
    post-depthwise ReLU6 and graph entry [2]'s post-expand ReLU6."""
    from torchpruner_amd import get_mobilenet_pruning_graph
    graph = get_mobilenet_pruning_graph(model)
    return [("last expand", graph[0][0]), ("last depthwise", graph[0][1][1]), ("graph[2] expand", graph[2][0])]


def _ref64(s, ti, criterion=F.cross_entropy):
    """Per-sample Shapley values of target ``ti`` on the float64 CPU hook path, computed once."""
    key = ("sv", ti, criterion.__name__)
    if key not in s["ref"]:
        module = _targets(s["m64"])[ti][1]
        s["ref"][key] = _shapley(s["m64"], module, s["x"].double().cpu(), s["y"].cpu(), "cpu", "torch", criterion)[0]
    return s["ref"][key]


def _rel_err(got, ref):
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


def test_shapley_matches_the_fp64_hook_path(setup, cuda):
    """sv_samples=2, reduction="none", 6 images in batches of 3, np.random.seed(7): max abs error /
    max |ref| < 2e-2 (the bound of test_resnet_engine_shapley_matches_fp64) against the float64 CPU
    hook path, on the three modules where the reference's own fp32 run stays far inside that bound
    (1.4e-5, 7.4e-6, 1.6e-4). The served path must be the engine's: on the generic-hook path this
    test fails.

    Measured on an MI355X: 1.1e-5 (last expand), 6.0e-6 (last depthwise), 1.6e-4 (graph[2] expand); the
    three float64 reference runs take ~30 s each on the CPU."""
    s = setup
    for ti, (name, module) in enumerate(_targets(s["model"])):
        got, metric = _shapley(s["model"], module, s["x"], s["y"], cuda, "hip", mobilenet_engine=True)
        assert metric.last_path["path"] == "mobilenet", metric.last_path
        ref = _ref64(s, ti)
        assert got.shape == ref.shape == (6, module.weight.shape[0])
        err = _rel_err(got, ref)
        print(f"shapley {name}: max abs error / max |ref| = {err:.3e} (max |ref| {np.abs(ref).max():.3e})")
        assert err < 2e-2, (name, err)


def test_shapley_is_opt_in(setup, cuda, monkeypatch):
    s = setup
    monkeypatch.delenv("TORCHPRUNER_MOBILENET_ENGINE", raising=False)
    module = _targets(s["model"])[1][1]
    _, metric = _shapley(s["model"], module, s["x"][:3], s["y"][:3], cuda, "hip", prefix_batch=64)
    assert metric.last_path["path"] == "generic-hook", metric.last_path


@pytest.mark.parametrize("variant", ["prefix_batch_1", "prefix_batch_5", "mse", "mean"])
def test_shapley_variants_stay_within_the_bound(setup, cuda, variant):
    """On the last block's post-depthwise ReLU6: chunk sizes 1 and 5 (the default is the test above),
    an MSE-to-one-hot criterion and reduction="mean", each < 2e-2 against the float64 hook path."""
    s = setup
    ti = 1
    module = _targets(s["model"])[ti][1]
    kw, crit, red = {}, F.cross_entropy, "none"
    if variant.startswith("prefix_batch"):
        kw["prefix_batch"] = int(variant.rsplit("_", 1)[1])
    elif variant == "mse":
        crit = _mse_one_hot
    else:
        red = "mean"
    got, metric = _shapley(s["model"], module, s["x"], s["y"], cuda, "hip", crit, red, mobilenet_engine=True, **kw)
    assert metric.last_path["path"] == "mobilenet", metric.last_path
    # reduction="mean" divides the same fp64 sums of loss differences by the sample count: its
    # reference is the per-sample float64 hook-path result averaged (no second 30 s CPU run)
    ref = _ref64(s, ti, crit).mean(0) if red == "mean" else _ref64(s, ti, crit)
    assert got.shape == ref.shape
    err = _rel_err(got, ref)
    print(f"shapley variant {variant}: max abs error / max |ref| = {err:.3e}")
    assert err < 2e-2, (variant, err)


def test_shapley_after_a_prune(setup, cuda):
    """After Pruner.prune_model on the last block the engine repacks and n follows the new width."""
    from torchpruner_amd import Pruner, get_mobilenet_pruning_graph
    s = setup
    model = copy.deepcopy(s["model"])
    module, cascade = get_mobilenet_pruning_graph(model)[0]
    n = module.weight.shape[0]
    drop = np.setdiff1d(np.arange(n), np.arange(0, n, 3))  # keep one channel in three: a short reference run
    Pruner(model, (3, 32, 32), cuda).prune_model(module, drop, cascade)
    m64 = copy.deepcopy(model).double().cpu()
    width = n - len(drop)
    assert module.weight.shape[0] == width
    got, metric = _shapley(model, cascade[1], s["x"], s["y"], cuda, "hip", mobilenet_engine=True)
    assert metric.last_path["path"] == "mobilenet", metric.last_path
    ref, _ = _shapley(m64, get_mobilenet_pruning_graph(m64)[0][1][1], s["x"].double().cpu(), s["y"].cpu(), "cpu",
                      "torch")
    assert got.shape == ref.shape == (6, width)
    err = _rel_err(got, ref)
    print(f"shapley after a prune: max abs error / max |ref| = {err:.3e}")
    assert err < 2e-2, err
