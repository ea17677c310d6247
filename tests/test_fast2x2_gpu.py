"""The nine-product kernels of the 2x2-map conv layers (csrc/kernels/conv2x2_fast.hip) against
fp64 PyTorch, and the VGG16 engine pinned to them against the fp64 oracle.

Bound: max |out - ref| / max |ref| < 2e-5, the bound tests/test_wino4_gpu.py uses (the coefficients
of the transforms are 0 and +-1: V sums at most 4 pixels, Y at most 4 products). Shapes: B = 1, 5 and
130 (130 crosses a 128-row tile and leaves a partial one), channel counts of one to three 32-wide K
slices with N below, at and off the tile width, one K pass and a 2-way split."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 2e-5
BATCHES = [1, 5, 130]
CHANNELS = [(32, 32), (96, 64), (64, 96)]  # (C, K)


def _relerr(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


@functools.lru_cache(maxsize=None)
def _case(B, C, K):
    """Operands and the fp64 references of one shape, computed once and shared (read-only)."""
    from torchpruner_amd.engine.fused_chain import fast2x2_weights
    g = torch.Generator().manual_seed(B * 10007 + C * 101 + K)
    x = torch.randn(B, 2, 2, C, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    scale = torch.randn(K, generator=g).abs() + 0.5
    shift = torch.randn(K, generator=g) * 0.1
    xd = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    conv = F.conv2d(xd, w.double(), padding=1)
    y = (conv * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).clamp_min(0)
    # data gradient of the same conv: gy at its output, act = the (ReLU'd) activation at its input
    gy = torch.randn(B, 2, 2, K, generator=g)
    act = torch.randn(B, 2, 2, C, generator=g).clamp_min(0)
    bn = torch.randn(C, generator=g).abs() + 0.5
    (gx,) = torch.autograd.grad(conv, xd, gy.permute(0, 3, 1, 2).double(), retain_graph=True)
    gx = gx.permute(0, 2, 3, 1).contiguous()  # (B, 2, 2, C) fp64
    # the pooled form of a gradient: one value per (image, channel) at a random pixel of the window
    gp = torch.randn(B, 1, 1, K, generator=g)
    am = torch.randint(0, 4, (B, 1, 1, K), generator=g, dtype=torch.uint8)
    gfull = torch.zeros(B, 4, K).scatter_(1, am.view(B, 1, K).long(), gp.view(B, 1, K)).view(B, 2, 2, K)
    (gxp,) = torch.autograd.grad(conv, xd, gfull.permute(0, 3, 1, 2).double())
    return {"x": x, "w": w, "scale": scale, "shift": shift, "u9": fast2x2_weights(w), "u9t": fast2x2_weights(w, True),
            "y": y.detach().permute(0, 2, 3, 1).contiguous(), "gy": gy, "act": act, "bn": bn, "gx": gx,
            "gp": gp, "am": am, "gxp": gxp.permute(0, 2, 3, 1).contiguous()}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("CK", CHANNELS)
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("pool", [False, True])
def test_forward(cuda, B, CK, splits, pool):
    from torchpruner_amd import ops
    T = ops.require()
    c = _case(B, *CK)
    args = [c[k].to(cuda) for k in ("x", "u9", "scale", "shift")]
    y, _ = T.conv2x2_fast_fwd(*args, True, False, 0, splits)
    err = _relerr(y, c["y"])
    print(f"fwd B={B} C,K={CK} splits={splits}: rel err {err:.2e}")
    assert y.shape == (B, 2, 2, CK[1]) and err < BOUND
    if pool:  # pooled value and argmax byte: exactly maxpool2_nhwc of the unpooled result
        p, am = T.conv2x2_fast_fwd(*args, True, True, 0, splits)
        pr, amr = T.maxpool2_nhwc(y)
        assert p.shape == (B, 1, 1, CK[1]) and am.dtype == torch.uint8
        assert torch.equal(p, pr) and torch.equal(am, amr)


@pytest.mark.parametrize("cfg", range(7))
def test_forward_every_tile_config(cuda, cfg):
    from torchpruner_amd import ops
    T = ops.require()
    c = _case(130, 96, 64)
    y, _ = T.conv2x2_fast_fwd(*[c[k].to(cuda) for k in ("x", "u9", "scale", "shift")], True, False, cfg, 2)
    err = _relerr(y, c["y"])
    print(f"fwd cfg {cfg}: rel err {err:.2e}")
    assert err < BOUND


def test_forward_without_affine_or_relu(cuda):
    from torchpruner_amd import ops
    T = ops.require()
    c = _case(5, 64, 96)
    y, _ = T.conv2x2_fast_fwd(c["x"].to(cuda), c["u9"].to(cuda), None, None, False, False, 0, 1)
    ref = F.conv2d(c["x"].permute(0, 3, 1, 2).double(), c["w"].double(), padding=1).permute(0, 2, 3, 1)
    assert _relerr(y, ref) < BOUND


def _dgrad_refs(c, gx, mode, bn):
    a = c["act"].double()
    out = torch.where(a > 0, gx * (c["bn"].double() if bn else 1.0), torch.zeros_like(gx))
    tay = gx.abs() if mode else -(gx * a)
    return out, tay.permute(1, 2, 0, 3).reshape(4, gx.shape[0], gx.shape[3])  # slot = pixel


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("CK", CHANNELS)
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("want_out,mode,bn", [(True, 0, True), (False, 0, True), (True, 1, False), (False, 1, False),
                                               (True, 0, False), (True, 1, True)])
def test_data_gradient(cuda, B, CK, splits, want_out, mode, bn):
    from torchpruner_amd import ops
    T = ops.require()
    C, K = CK
    c = _case(B, C, K)
    out_ref, tay_ref = _dgrad_refs(c, c["gx"], mode, bn)
    tay = torch.zeros(4, B, C, device=cuda)
    out = T.conv2x2_fast_dgrad(c["gy"].to(cuda), None, c["u9t"].to(cuda), c["act"].to(cuda),
                               c["bn"].to(cuda) if bn else None, tay, want_out, 0, splits, mode)
    et = _relerr(tay, tay_ref)
    print(f"dgrad B={B} C,K={CK} splits={splits} mode={mode}: partials rel err {et:.2e}")
    assert et < BOUND
    if want_out:
        eo = _relerr(out, out_ref)
        print(f"    output rel err {eo:.2e}")
        assert out.shape == (B, 2, 2, C) and eo < BOUND
        assert (out.cpu()[c["act"] <= 0] == 0).all()  # the ReLU mask, exactly
    else:
        assert out is None


@pytest.mark.parametrize("B,CK,splits", [(130, (96, 64), 2), (5, (64, 96), 1)])
def test_data_gradient_from_pooled_gradient(cuda, B, CK, splits):
    """The pooled gradient + argmax bytes give what the explicitly unpooled gradient gives, bit for
    bit (the input transform unpools), and match fp64."""
    from torchpruner_amd import ops
    T = ops.require()
    C, K = CK
    c = _case(B, C, K)
    gp, am, u, act, bn = (c[k].to(cuda) for k in ("gp", "am", "u9t", "act", "bn"))
    tay = torch.zeros(4, B, C, device=cuda)
    out = T.conv2x2_fast_dgrad(gp, am, u, act, bn, tay, True, 0, splits, 0)
    tay2 = torch.zeros(4, B, C, device=cuda)
    out2 = T.conv2x2_fast_dgrad(T.unpool2_nhwc(gp, am), None, u, act, bn, tay2, True, 0, splits, 0)
    assert torch.equal(out, out2) and torch.equal(tay, tay2)
    out_ref, tay_ref = _dgrad_refs(c, c["gxp"], 0, True)
    assert _relerr(out, out_ref) < BOUND and _relerr(tay, tay_ref) < BOUND


def test_taylor_partials_accumulate(cuda):
    """The slab is accumulated into, as the dense path's epilogue does."""
    from torchpruner_amd import ops
    T = ops.require()
    c = _case(5, 64, 96)
    args = (c["gy"].to(cuda), None, c["u9t"].to(cuda), c["act"].to(cuda), None)
    once = torch.zeros(4, 5, 64, device=cuda)
    T.conv2x2_fast_dgrad(*args, once, False, 0, 1, 0)
    base = torch.full((4, 5, 64), 3.0, device=cuda)
    T.conv2x2_fast_dgrad(*args, base, False, 0, 1, 0)
    assert torch.equal(base, once + 3.0)


def test_nan_reaches_the_outputs_the_dense_form_marks(cuda):
    """A NaN input element turns NaN exactly the outputs the dense-GEMM form turns NaN (every pixel
    and channel of that image: the pruner's cascade probe relies on the marks), pooled or not."""
    from torchpruner_amd import ops
    from torchpruner_amd.engine.fused_chain import FusedChainEngine
    T = ops.require()
    B, C, K = 5, 64, 96
    c = _case(B, C, K)
    x = c["x"].clone()
    x[3, 0, 1, 17] = float("nan")
    x = x.to(cuda)
    scale, shift = c["scale"].to(cuda), c["shift"].to(cuda)
    e = {"scale": scale, "shift": shift, "w": c["w"].permute(0, 2, 3, 1).reshape(K, -1).contiguous().to(cuda)}
    d = FusedChainEngine._dense(e)
    dense, _ = T.conv_fwd(x.reshape(B, 1, 1, -1), d["w"], d["scale4"], d["shift4"], True, False, 1, 0, 1)
    dense = dense.view(B, 2, 2, K)
    y, _ = T.conv2x2_fast_fwd(x, c["u9"].to(cuda), scale, shift, True, False, 0, 1)
    assert torch.equal(y.isnan(), dense.isnan()) and y[3].isnan().all() and not y[:3].isnan().any()
    p, am = T.conv2x2_fast_fwd(x, c["u9"].to(cuda), scale, shift, True, True, 0, 1)
    pd, amd = T.maxpool2_nhwc(dense)
    assert torch.equal(p.isnan(), pd.isnan()) and torch.equal(am[3], amd[3])
    # data gradient: a NaN gradient element marks every input-gradient element of that image
    gy = c["gy"].clone()
    gy[2, 1, 0, 5] = float("nan")
    act = c["act"].to(cuda)
    td = torch.zeros(4, B, C, device=cuda)
    od = T.conv_dgrad(gy.to(cuda).reshape(B, 1, 1, -1), None, d["wt"], act.reshape(B, 1, 1, -1), None, td, True, 1, 0,
                      1, C).view(B, 2, 2, C)
    tf = torch.zeros(4, B, C, device=cuda)
    of = T.conv2x2_fast_dgrad(gy.to(cuda), None, c["u9t"].to(cuda), act, None, tf, True, 0, 1, 0)
    assert torch.equal(of.isnan(), od.isnan()) and torch.equal(tf.isnan(), td.isnan()) and tf[:, 2].isnan().all()


def test_bit_identical_runs(cuda):
    from torchpruner_amd import ops
    T = ops.require()
    c = _case(130, 96, 64)
    fw = [c[k].to(cuda) for k in ("x", "u9", "scale", "shift")]
    bw = (c["gy"].to(cuda), None, c["u9t"].to(cuda), c["act"].to(cuda), c["bn"].to(cuda))
    runs = []
    for _ in range(2):
        p, am = T.conv2x2_fast_fwd(*fw, True, True, 0, 2)
        tay = torch.zeros(4, 130, 96, device=cuda)
        out = T.conv2x2_fast_dgrad(*bw, tay, True, 0, 2, 0)
        runs.append((p, am, out, tay))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_engine_pinned_to_fast2x2_matches_fp64_oracle(cuda):
    """CIFAR VGG16-BN, B = 8, every 2x2-map layer pinned to the nine-product family: the three
    layers really ran it, forward and backward (no silent fallback), and the 13 Taylor score
    vectors match the fp64 oracle at the tolerance of the package smoke run."""
    from torchpruner_amd import TaylorAttributionMetric
    from torchpruner_amd.data import DeviceLoader
    from torchpruner_amd.engine import maybe_engine
    from torchpruner_amd.engine.fused_chain import FAST2, TUNER, family_policy, kernel_name
    from torchpruner_amd.engine.oracle import engine_scores_fp64, flip_violations
    from torchpruner_amd.models import prunable_vgg16
    from torchpruner_amd.utils import find_best_module_for_attributions
    torch.manual_seed(0)
    model = prunable_vgg16().to(cuda).eval()
    convs = [m for m in model.features if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 13
    x = torch.randn(8, 3, 32, 32, device=cuda)
    y = torch.randint(0, 10, (8,), device=cuda)
    with TUNER.pinned(family_policy("fast2x2")):
        metric = TaylorAttributionMetric(model, DeviceLoader(x, y, 8), F.cross_entropy, cuda)
        scores = metric.run_many(convs, find_best_evaluation_module=True)
        assert metric.last_path["path"] == "fused", metric.last_path
        picks = dict(TUNER.cache)
    fwd = [v for k, v in picks.items() if k[0] == "fwd" and tuple(k[1][1:3]) == (2, 2)]
    bwd = [v for k, v in picks.items() if k[0] == "bwd" and tuple(k[2][1:3]) == (2, 2)]
    # conv 10 / 11 share a shape (one key), conv 12 pools; the three data gradients: pooled
    # gradient (conv 12), full-resolution gradient (conv 11), and conv 10's, whose output is unpooled next
    assert len(fwd) == 2 and len(bwd) == 3, picks
    for cfg, _ in fwd + bwd:
        assert FAST2 <= cfg < FAST2 + 7 and kernel_name(cfg).startswith("fast2x2"), picks
    eng, idx = maybe_engine(model, [find_best_module_for_attributions(model, m) for m in convs], F.cross_entropy,
                            cuda)
    with TUNER.pinned(family_policy("fast2x2")):
        tot = {}
        sc, flips = engine_scores_fp64(eng, x, y, totals=tot)
    assert not flip_violations(flips, tot), flip_violations(flips, tot)
    for k, b in enumerate(idx):
        ref = np.abs(sc[b].numpy()).mean(0)
        err = np.abs(scores[k] - ref).max() / np.abs(ref).max()
        print(f"conv {k}: fused Taylor vs fp64 oracle rel. error {err:.2e}")
        assert err < 1e-4, f"conv {k}: rel. error {err:.2e}"
