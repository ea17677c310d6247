"""The conv weight-gradient kernels (conv_wgrad.hip: the pixel-split MFMA GEMM and its split combine;
wino_wgrad.hip: the F(2x2,3x3) transforms around 16 batched GEMMs) directly against the references of
tests/test_wgrad_math.py:

a. the direct kernel on integer operands: the whole (Cout, Kpad) result, pad columns included, EQUAL to fp64;
b. the same cases on randn operands under a derived fp32 bound;
c. the split combine's summation order bit for bit against slabs made by separate one-split calls, through the one-lane
   in-order path, every lane count the launcher picks, the 4-way unrolled loop and the grid-stride second sweep;
d. TP_WGRAD_COMBINE_LANES=1 in a child process: the strict in-order sum;
e. ``out=`` in the contiguous, channels_last and strided (a view inside a larger buffer) layouts;
f. the Winograd weight gradient, exact on integers and bounded on randn;
g. the launchers' refusal of an empty batch.

No bound is fitted to what the kernels give: each is derived in its test's docstring. Every test prints its figures;
those of an MI355X run are in profiles/numerics/wgrad.txt."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from test_wgrad_math import (DIRECT_CASES, U24, WINO_CARRIED, WINO_CARRIED_REAL, WINO_CASES, case_id, combine_emul,
                             direct_int_reference, eff_splits, kpad_of, lanes, mag_dw64, operands, out_hw, param_of,
                             ref_dw64, wino_int_reference, wino_wgrad_emul)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = [0, 1, 2]


def _T():
    from torchpruner_amd import ops
    return ops.require()


def _pixels(case):
    B, H, W, Cin, Cout, ks, s, p = case
    Ho, Wo = out_hw(H, W, ks, s, p)
    return B * Ho * Wo


def _split_requests(P):
    """splits in {1, 2, 7, number of slices}."""
    return sorted({1, 2, 7, -(-P // 32)})


@functools.lru_cache(maxsize=None)
def _direct_randn_reference(case):
    x, g = operands(case, "randn")
    return x, g, ref_dw64(x, g, *case[5:]), mag_dw64(x, g, *case[5:])


def _ratio(err, bound):
    """Largest err / bound; an element whose bound is zero (a pad column, a tap that only ever meets padding) must be
    exactly zero."""
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "non-zero where the reference has no term at all"
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


# ------------------------------------------------------------------------------------------- a. direct, exact
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("case", DIRECT_CASES, ids=case_id)
def test_direct_exact_on_integers(cuda, case, cfg):
    """Integer operands in [-3, 3]: every product and partial sum is an integer below 2^24 (asserted in
    test_wgrad_math.py), so the fp32 MFMA chain and the split combine are exact in any order: the (Cout, Kpad) result,
    pad columns included, equals the fp64 reference for every split count."""
    T = _T()
    x, g, ref = direct_int_reference(case)
    B, H, W, Cin, Cout, ks, s, p = case
    xd, gd = x.to(cuda), g.to(cuda)
    reqs = _split_requests(_pixels(case))
    for splits in reqs:
        dw = T.conv_wgrad(gd, xd, ks, s, p, cfg, splits)
        assert dw.shape == (Cout, kpad_of(ks, Cin)) and dw.dtype == torch.float32
        got = dw.double().cpu()
        bad = int((got != ref).sum())
        assert bad == 0, f"splits={splits}: {bad} of {ref.numel()} elements differ, largest {float((got - ref).abs().max())}"
    print(f"wgrad direct exact case={case_id(case)} cfg={cfg} splits={reqs} mismatches=0")


# ------------------------------------------------------------------------------------------- b. direct, fp64 bound
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("case", DIRECT_CASES, ids=case_id)
def test_direct_fp64_bound_on_randn(cuda, case, cfg):
    """randn operands carry full 24-bit mantissas, so a reduced-precision MFMA (which integers cannot see) shows.
    Per element, with u = 2^-24, P pixels and S effective splits,  |dw - ref| <= (P + S + 4) * u * mag,
    mag = the same gradient on |x|, |g|:
    - a split's element is a sum of at most P_s products accumulated one after the other in fp32: each product is
      rounded at most once and takes part in at most P_s rounded additions, so its error is at most
      ((1 + u)^(P_s + 1) - 1) * mag_s  (any accumulation order; a fused multiply-add only removes roundings; padded
      pixels and taps add exact zeros);
    - the combine adds the S slabs with at most S rounded additions on any term's path (lane sums, then the lanes);
    - together (1 + u)^(P + 1 + S) - 1 <= (P + S + 1) * u * (1 + (P + S) * u) for (P + S) * u << 1; here P + S < 2^11, so
      the second-order factor is below 1 + 2^-13 and three more units of u cover it and the final fp64 comparison."""
    T = _T()
    x, g, ref, mag = _direct_randn_reference(case)
    B, H, W, Cin, Cout, ks, s, p = case
    xd, gd = x.to(cuda), g.to(cuda)
    P = _pixels(case)
    worst = 0.0
    for splits in _split_requests(P):
        S = eff_splits(P, splits)[0]
        got = T.conv_wgrad(gd, xd, ks, s, p, cfg, splits).double().cpu()
        r = _ratio((got - ref).abs(), (P + S + 4) * U24 * mag)
        worst = max(worst, r)
        print(f"wgrad direct bound case={case_id(case)} cfg={cfg} splits={splits} S={S} P={P} err/bound={r:.4f}")
        assert r <= 1.0
    print(f"wgrad direct bound case={case_id(case)} cfg={cfg} largest err/bound={worst:.4f}")


# ------------------------------------------------------------------------------------------- c. combine order
# (Cin, Cout, P, splits) of 1x1 stride-1 convs on (1, P, 1, C) operands
COMBINE_1X1 = [
    (512, 512, 197, 7),   # n = 262144: ONE lane, the in-order sum; one unrolled pass plus 3 remainder terms
    (4, 8, 1277, 40),     # 8 lanes of 5 slabs: one unrolled pass plus a remainder term each
    (512, 128, 185, 6),   # n = 65536: 4 lanes
    (1024, 96, 185, 6),   # n = 98304: 3 lanes
]
COMBINE_LANES = {(512, 512, 197, 7): 1, (4, 8, 1277, 40): 8, (512, 128, 185, 6): 4, (1024, 96, 185, 6): 3}


@functools.lru_cache(maxsize=None)
def _combine_operands(Cin, Cout, P):
    gen = torch.Generator().manual_seed(Cin + Cout + P)
    return torch.randn(1, P, 1, Cin, generator=gen), torch.randn(1, P, 1, Cout, generator=gen)


def _check_combine(T, gd, xd, ks, pad, cfg, splits, slabs, SL, tag):
    """The split call == combine_emul(slabs, SL) bit for bit; a second call and the out= (FIN) combine give the same
    bits."""
    Cin, Cout = xd.shape[3], gd.shape[3]
    want = combine_emul(slabs, SL)
    dw = T.conv_wgrad(gd, xd, ks, 1, pad, cfg, splits)
    assert torch.equal(dw, want), (f"{tag}: {int((dw != want).sum())} of {want.numel()} elements differ from the "
                                   f"{SL}-lane order, largest {float((dw - want).abs().max())}")
    assert torch.equal(T.conv_wgrad(gd, xd, ks, 1, pad, cfg, splits), dw), f"{tag}: two calls differ"
    out = torch.full((Cout, Cin, ks, ks), float("nan"), device=gd.device)
    T.conv_wgrad(gd, xd, ks, 1, pad, cfg, splits, out)
    assert torch.equal(out, param_of(dw, Cin, ks)), f"{tag}: the out= combine differs"
    return dw, want


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("Cin,Cout,P,splits", COMBINE_1X1, ids=lambda v: str(v))
def test_combine_order_1x1(cuda, Cin, Cout, P, splits, cfg):
    """Slab q of the split call is the one-split result on pixels [q * 32 * per, (q + 1) * 32 * per): the GEMM kernel
    walks a split's slices in order whatever blockIdx.y it has. The combine must add them in the documented order:
    the result equals combine_emul(slabs, lanes(n, S)) bit for bit (and, checked on the reference side, does not equal
    another lane count's order, so the comparison can tell them apart)."""
    T = _T()
    x, g = _combine_operands(Cin, Cout, P)
    xd, gd = x.to(cuda), g.to(cuda)
    S, per = eff_splits(P, splits)
    assert S == splits
    n = Cout * kpad_of(1, Cin)
    SL = lanes(n, S)
    assert SL == COMBINE_LANES[(Cin, Cout, P, splits)]
    step = 32 * per
    slabs = torch.stack([T.conv_wgrad(gd[:, a:a + step], xd[:, a:a + step], 1, 1, 0, cfg, 1) for a in range(0, P, step)])
    assert slabs.shape[0] == S
    dw, want = _check_combine(T, gd, xd, 1, 0, cfg, splits, slabs, SL, f"{Cin}->{Cout} P={P} S={S}")
    others = [o for o in (1, 2, 3, 4, 8) if o != SL and o <= S]
    told_apart = [o for o in others if not torch.equal(combine_emul(slabs, o), want)]
    assert told_apart == others, f"orders {set(others) - set(told_apart)} give the same bits: the case proves nothing"
    ref = ref_dw64(x, g, 1, 1, 0)
    r = _ratio((dw.double().cpu() - ref).abs(), (P + S + 4) * U24 * mag_dw64(x, g, 1, 1, 0))
    print(f"wgrad combine 1x1 {Cin}->{Cout} P={P} S={S} n={n} lanes={SL} cfg={cfg} bits=equal err/bound={r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("cfg", CFGS)
def test_combine_order_3x3_per_image(cuda, cfg):
    """B = 6 images of 8x8, 16 -> 16, 3x3: 12 slices in 6 splits, so every split is one image and its slab the
    one-split call on that image (n = 2560: 6 lanes of one slab, added in lane order)."""
    T = _T()
    case = (6, 8, 8, 16, 16, 3, 1, 1)
    x, g = operands(case, "randn")
    xd, gd = x.to(cuda), g.to(cuda)
    S, per = eff_splits(6 * 64, 6)
    assert (S, per) == (6, 2)
    n = 16 * kpad_of(3, 16)
    SL = lanes(n, S)
    assert SL == 6
    slabs = torch.stack([T.conv_wgrad(gd[b:b + 1], xd[b:b + 1], 3, 1, 1, cfg, 1) for b in range(6)])
    dw, want = _check_combine(T, gd, xd, 3, 1, cfg, 6, slabs, SL, "3x3 per image")
    # one slab per lane: lane order is slab order (0.f + v == v), another lane count's order is not
    assert torch.equal(combine_emul(slabs, 1), want) and not torch.equal(combine_emul(slabs, 3), want)
    r = _ratio((dw.double().cpu() - ref_dw64(x, g, 3, 1, 1)).abs(), (384 + S + 4) * U24 * mag_dw64(x, g, 3, 1, 1))
    print(f"wgrad combine 3x3 per-image S={S} n={n} lanes={SL} cfg={cfg} bits=equal err/bound={r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("cfg", CFGS)
def test_combine_grid_stride_sweep_exact(cuda, cfg):
    """512 -> 512 3x3 on one 8x8 image in 2 splits: n = 2359296 elements > 16384 blocks * 64, so the combine's blocks
    sweep their grid stride more than twice. Integer operands: EQUAL to fp64 over the whole matrix, so an element
    skipped or written twice by a sweep shows. Also through out=, and twice."""
    T = _T()
    case = (1, 8, 8, 512, 512, 3, 1, 1)
    x, g, ref = direct_int_reference(case)
    xd, gd = x.to(cuda), g.to(cuda)
    assert eff_splits(64, 2) == (2, 1) and 512 * kpad_of(3, 512) > 2 * 16384 * 64
    dw = T.conv_wgrad(gd, xd, 3, 1, 1, cfg, 2)
    bad = int((dw.double().cpu() != ref).sum())
    assert bad == 0, f"{bad} of {ref.numel()} elements differ"
    assert torch.equal(T.conv_wgrad(gd, xd, 3, 1, 1, cfg, 2), dw)
    out = torch.full((512, 512, 3, 3), float("nan"), device=cuda)
    T.conv_wgrad(gd, xd, 3, 1, 1, cfg, 2, out)
    assert torch.equal(out, param_of(dw, 512, 3))
    print(f"wgrad combine grid-stride n={ref.numel()} cfg={cfg} mismatches=0")


# ------------------------------------------------------------------------------------------- d. the env switch
_CHILD = """
import sys
import torch
from torchpruner_amd import ops
T = ops.require()
d = torch.load(sys.argv[1])
dw = T.conv_wgrad(d["g"].cuda(), d["x"].cuda(), 1, 1, 0, d["cfg"], d["splits"])
torch.cuda.synchronize()
torch.save(dw.cpu(), sys.argv[2])
"""


def test_combine_lanes_env_forces_in_order_sum(cuda, tmp_path):
    """TP_WGRAD_COMBINE_LANES=1 (read once per process, hence a fresh child): the 4 -> 8, 40-split case, which takes 8
    lanes by default, must come out as the strict in-order sum of its slabs, which differs in bits from the 8-lane
    order."""
    T = _T()
    Cin, Cout, P, splits, cfg = 4, 8, 1277, 40, 1
    x, g = _combine_operands(Cin, Cout, P)
    xd, gd = x.to(cuda), g.to(cuda)
    slabs = torch.stack([T.conv_wgrad(gd[:, a:a + 32], xd[:, a:a + 32], 1, 1, 0, cfg, 1) for a in range(0, P, 32)]).cpu()
    assert slabs.shape[0] == 40
    src, dst = tmp_path / "operands.pt", tmp_path / "dw.pt"
    torch.save({"x": x, "g": g, "cfg": cfg, "splits": splits}, src)
    env = dict(os.environ, TP_WGRAD_COMBINE_LANES="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(src), str(dst)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    child = torch.load(dst)
    seq, par = combine_emul(slabs, 1), combine_emul(slabs, 8)
    assert not torch.equal(seq, par)
    assert torch.equal(child, seq), f"{int((child != seq).sum())} elements differ from the in-order sum"
    assert not torch.equal(child, par)
    print(f"wgrad combine env TP_WGRAD_COMBINE_LANES=1 S=40 bits=in-order "
          f"differs_from_8_lanes_in={int((child != par).sum())} of {par.numel()}")


# ------------------------------------------------------------------------------------------- e. out= layouts
SENTINEL = -123456.75


def _out_layout(layout, co, ci, ks, dev):
    """(the tensor the op writes, the whole buffer behind it)."""
    if layout == "contiguous":
        buf = torch.full((co, ci, ks, ks), SENTINEL, device=dev)
        return buf, buf
    if layout == "channels_last":
        buf = torch.full((co, ci, ks, ks), SENTINEL, device=dev).contiguous(memory_format=torch.channels_last)
        return buf, buf
    if layout == "bucket":  # a parameter's slot of a flat gradient bucket, at an offset of 5 floats
        buf = torch.full((co * ci * ks * ks + 13,), SENTINEL, device=dev)
        return buf[5:5 + co * ci * ks * ks].view(co, ci, ks, ks), buf
    buf = torch.full((co + 2, ci + 3, ks + 2, ks + 1), SENTINEL, device=dev)  # strided on every dim
    return buf[1:1 + co, 2:2 + ci, 1:1 + ks, 1:1 + ks], buf


def _outside_untouched(view, buf):
    """Elements of ``buf`` outside ``view`` still hold the sentinel's bits."""
    bits = buf.clone().view(torch.int32)
    # mark the view's elements through the view's own geometry
    marker = torch.zeros_like(buf)
    marker.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(1.0)
    inside = marker != 0
    want = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    return int(inside.sum()) == view.numel() and bool((bits[~inside] == want).all())


@pytest.mark.parametrize("splits", [1, 5])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last", "bucket", "strided"])
@pytest.mark.parametrize("op", ["conv_wgrad", "wino_wgrad"])
def test_out_layouts(cuda, op, layout, splits):
    """out= of the real channels (44 of 64 out, 50 of 64 in) in four layouts, integer operands: the view holds the fp64
    reference exactly (for conv_wgrad also the GEMM-layout result of the same call), and every element of the buffer
    outside the view keeps its bits."""
    T = _T()
    case = (2, 10, 12, 64, 64, 3, 1, 1)
    co, ci = 44, 50
    x, g, ref = direct_int_reference(case)
    xd, gd = x.to(cuda), g.to(cuda)
    view, buf = _out_layout(layout, co, ci, 3, cuda)
    if op == "conv_wgrad":
        T.conv_wgrad(gd, xd, 3, 1, 1, 0, splits, view)
        assert torch.equal(view, param_of(T.conv_wgrad(gd, xd, 3, 1, 1, 0, splits), 64, 3)[:co, :ci])
    else:
        T.wino_wgrad(gd, xd, 0, splits, view)
    assert torch.equal(view.double().cpu(), param_of(ref, 64, 3)[:co, :ci])
    assert _outside_untouched(view, buf)
    print(f"wgrad out= op={op} layout={layout} splits={splits} exact=yes outside=untouched")


# ------------------------------------------------------------------------------------------- f. Winograd
def _wino_split_requests(T_tiles):
    """splits in {1, 4, number of slices}."""
    return sorted({1, 4, -(-T_tiles // 32)})


def _wino_out(case, dev):
    B, H, W, Cin, Cout = case
    if case == WINO_CARRIED:
        co, ci = WINO_CARRIED_REAL
        return torch.full((co, ci, 3, 3), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
    return torch.full((Cout, Cin, 3, 3), float("nan"), device=dev)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("case", WINO_CASES, ids=case_id)
def test_wino_exact_on_integers(cuda, case, cfg):
    """Integer operands in [-3, 3]: V, dM and dU are integers, the output transform halves twice; every intermediate
    is a multiple of 1/4 below 2^22 (asserted in test_wgrad_math.py), so the result equals the fp64 conv2d_weight. Two
    calls give equal bits."""
    T = _T()
    x, g, ref = wino_int_reference(case)
    B, H, W, Cin, Cout = case
    xd, gd = x.to(cuda), g.to(cuda)
    reqs = _wino_split_requests(B * (H // 2) * (W // 2))
    for splits in reqs:
        out, again = _wino_out(case, cuda), _wino_out(case, cuda)
        T.wino_wgrad(gd, xd, cfg, splits, out)
        T.wino_wgrad(gd, xd, cfg, splits, again)
        want = ref[:out.shape[0], :out.shape[1]]
        bad = int((out.double().cpu() != want).sum())
        assert bad == 0, f"splits={splits}: {bad} of {want.numel()} elements differ"
        assert torch.equal(out, again)
    print(f"wgrad wino exact case={case_id(case)} cfg={cfg} splits={reqs} mismatches=0")


@functools.lru_cache(maxsize=None)
def _wino_randn_reference(case):
    B, H, W, Cin, Cout = case
    x, g = operands((B, H, W, Cin, Cout, 3, 1, 1), "randn")
    return (x, g, param_of(ref_dw64(x, g, 3, 1, 1), Cin, 3).contiguous(),
            wino_wgrad_emul(x, g, torch.float64, absolute=True))


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("case", WINO_CASES, ids=case_id)
def test_wino_fp64_bound_on_randn(cuda, case, cfg):
    """|dW - ref| <= (T + S + 16) * 2^-24 * mag, T tiles, S effective splits, mag = wino_wgrad_emul(absolute=True): the
    three steps with every matrix and operand replaced by its absolute value, which bounds the absolute sum behind
    every intermediate. Roundings on the path of one term:
    - V = B^T d B: each entry adds or subtracts two values per pass (rows, then columns): 2 rounded additions;
    - dM = A dY A^T: likewise at most 2;
    - the GEMM over T tiles: the product and at most T additions, then at most S in the combine: T + 1 + S;
    - dW = G^T dU G: two passes of a 4-term sum (the factors 1/2 and 1 are exact): 3 additions each; a compiler that
      does not contract them rounds the four products as well, 8 in all;
    2 + 2 + (T + 1 + S) + 8 = T + S + 13; (1 + u)^(T + S + 13) - 1 <= (T + S + 16) * u for T + S < 2^11.
    Two calls give equal bits."""
    T = _T()
    x, g, ref, mag = _wino_randn_reference(case)
    B, H, W, Cin, Cout = case
    xd, gd = x.to(cuda), g.to(cuda)
    tiles = B * (H // 2) * (W // 2)
    worst = 0.0
    for splits in _wino_split_requests(tiles):
        S = eff_splits(tiles, splits)[0]
        out, again = _wino_out(case, cuda), _wino_out(case, cuda)
        T.wino_wgrad(gd, xd, cfg, splits, out)
        T.wino_wgrad(gd, xd, cfg, splits, again)
        assert torch.equal(out, again)
        co, ci = out.shape[:2]
        r = _ratio((out.double().cpu() - ref[:co, :ci]).abs(), (tiles + S + 16) * U24 * mag[:co, :ci])
        worst = max(worst, r)
        print(f"wgrad wino bound case={case_id(case)} cfg={cfg} splits={splits} S={S} T={tiles} err/bound={r:.4f}")
        assert r <= 1.0
    print(f"wgrad wino bound case={case_id(case)} cfg={cfg} largest err/bound={worst:.4f}")


# ------------------------------------------------------------------------------------------- g. empty batch
def test_empty_batch_is_refused(cuda):
    """An empty batch used to reach the launcher and divide by zero there (SIGFPE); both ops now raise."""
    T = _T()
    x, g = torch.zeros(0, 8, 8, 8, device=cuda), torch.zeros(0, 8, 8, 8, device=cuda)
    with pytest.raises(RuntimeError, match="empty"):
        T.conv_wgrad(g, x, 3, 1, 1, 0, 1)
    with pytest.raises(RuntimeError, match="empty"):
        T.conv_wgrad(g, x, 1, 1, 0, 1, 4)
    with pytest.raises(RuntimeError, match="empty"):
        T.wino_wgrad(g, x, 0, 1, torch.zeros(8, 8, 3, 3, device=cuda))
    xs = torch.zeros(2, 8, 8, 12, device=cuda)[..., 1:9]  # not contiguous: refused by the operand check
    with pytest.raises(RuntimeError):
        T.conv_wgrad(torch.zeros(2, 8, 8, 8, device=cuda), xs, 3, 1, 1, 0, 1)
    flat = torch.zeros(2 * 8 * 8 * 8 + 4, device=cuda)
    xo = flat[1:1 + 2 * 8 * 8 * 8].view(2, 8, 8, 8)       # contiguous, 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="aligned"):
        T.conv_wgrad(torch.zeros(2, 8, 8, 8, device=cuda), xo, 3, 1, 1, 0, 1)
    with pytest.raises(RuntimeError, match="aligned"):
        T.wino_wgrad(xo, torch.zeros(2, 8, 8, 8, device=cuda), 0, 1, torch.zeros(8, 8, 3, 3, device=cuda))
    with pytest.raises(RuntimeError):
        T.conv_wgrad(torch.zeros(2, 1, 1, 8, device=cuda), torch.zeros(2, 2, 2, 8, device=cuda), 3, 2, 0, 0, 1)
    print("wgrad refusals empty_batch=RuntimeError misaligned=RuntimeError kernel_larger_than_map=RuntimeError")
