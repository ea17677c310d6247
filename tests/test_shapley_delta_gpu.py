"""The two kernels of the Shapley prefix-delta evaluation, each against a reference written here:

- ``prefix_tri_operands`` (shapley.hip) is a gather and a select, so its reference is exact and the
  comparison is bit for bit;
- ``prefix_delta`` (the GEN 1x1 MFMA kernel with a row-broadcast residual, conv_mfma.hip) runs on every one
  of the seven tile configs the tuner may pick, against fp64 with an a-priori rounding bound;
- both together against fp64 masked copies of a Linear (the pairing of T's and Wsub's columns);
- the engine's ``prefix_delta_loss`` against its own masked-copy path and an fp64 CPU model, per prefix
  and sample instead of averaged into scores.

No bound here is tuned to what the kernels give: each is derived in the test's docstring. The measured
figures of an MI355X run are in profiles/numerics/shapley_delta.txt (every test prints its own line)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops

from test_mlp_engine_gpu import _fcnet
from test_ops_edges import _bits_np

U24 = 2.0 ** -24  # unit roundoff of fp32


def _act64(pre, relu, slope):
    """The epilogue's activation in fp64: none, ReLU (slope 0) or LeakyReLU."""
    return torch.where(pre > 0, pre, pre * slope) if relu else pre


# ---------------------------------------------------------------------------------- prefix_tri_operands
# (B, C, N, len(perm), p0, cnt, Kc)
TRI_CASES = [(1, 5, 3, 5, 0, 1, 32),            # cnt = 1: T and Wsub entirely zero
             (3, 40, 10, 37, 0, 32, 32),        # perm shorter than the padded width, cnt == Kc
             (3, 40, 10, 37, 30, 8, 32),        # the last prefix: reads perm[36]
             (4, 100, 12, 100, 17, 33, 64),     # cnt just past a 32-granule: zero columns 33..63
             (130, 300, 8, 300, 0, 256, 256)]   # 8.5 M elements: the grid-stride loop's second sweep


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,N,n,p0,cnt,Kc", TRI_CASES)
def test_prefix_tri_operands_bits(cuda, B, C, N, n, p0, cnt, Kc):
    """T[(j*B + b), i] = z[b, perm[p0+i]] if i < j else +0.0;  Wsub[n, i] = W[n, perm[p0+i]] if i < cnt-1
    else +0.0, as int32 bits (a NaN only has to be a NaN). z carries one NaN, one +inf and one -inf in
    gathered units: copy j has not removed unit perm[p0+i] for i >= j, and the entry there must be +0.0
    (a multiply by a 0 / 1 mask would give NaN)."""
    T = ops.require()
    g = torch.Generator().manual_seed(100 * B + C + N + p0 + cnt)
    z = torch.randn(B, C, generator=g)
    W = torch.randn(N, C, generator=g)
    perm = torch.randperm(C, generator=g)[:n].to(torch.int32)
    pn = perm.numpy().astype(np.int64)
    if cnt >= 2:  # gathered columns are i = 0 .. cnt-2; the NaN sits in the last one (row block cnt-1 only)
        spots = [(cnt - 2, float("nan")), (0, float("inf")), ((cnt - 1) // 2, float("-inf"))]
    else:         # nothing is gathered: the non-finite values must not appear anywhere
        spots = [(0, float("nan")), (1 % n, float("inf")), (2 % n, float("-inf"))]
    for s, (i, v) in enumerate(spots):
        z[s % B, pn[p0 + i if cnt >= 2 else i]] = v
    zn, Wn = z.numpy(), W.numpy()
    cols = pn[p0:p0 + cnt - 1]                       # the units copies 1 .. cnt-1 remove, in order
    gz = np.zeros((B, Kc), np.float32)
    gz[:, :cnt - 1] = zn[:, cols]
    lower = np.arange(Kc)[None, :] < np.arange(cnt)[:, None]                     # (cnt, Kc): i < j
    t_ref = np.where(lower[:, None, :], gz[None, :, :], np.float32(0.0)).astype(np.float32).reshape(cnt * B, Kc)
    w_ref = np.zeros((N, Kc), np.float32)
    w_ref[:, :cnt - 1] = Wn[:, cols]
    if cnt >= 2:  # the planted values are where the reference says, and masked to +0.0 above the diagonal
        assert np.isnan(t_ref[(cnt - 1) * B:, cnt - 2]).sum() == 1 and not np.isnan(t_ref[:(cnt - 1) * B]).any()
        assert np.isinf(t_ref).any()
    tri, wsub = T.prefix_tri_operands(z.to(cuda), W.to(cuda), perm.to(cuda), p0, cnt, Kc)
    assert tuple(tri.shape) == (cnt * B, Kc) and tuple(wsub.shape) == (N, Kc)
    assert _bits_np(tri, t_ref.reshape(-1)), "T differs from the gather / select reference"
    assert _bits_np(wsub, w_ref.reshape(-1)), "Wsub differs from the gather reference"


# ----------------------------------------------------------------------------------------- prefix_delta
# (B0, cnt, Kc, N); M = cnt * B0
DELTA_SHAPES = [(1, 1, 32, 4),       # one row, one quad of columns, one K slice
                (5, 32, 32, 12),     # M 160: the residual wraps inside every tile height, ragged M tail
                (7, 40, 64, 68),     # M 280: more than one 256-row tile, N crosses the 64-wide column tile
                (130, 3, 32, 132),   # M 390: the residual block is taller than a 128-row tile, N crosses 128
                (3, 96, 96, 200)]    # M 288: three K slices
ACTS = [(False, 0.0), (True, 0.0), (True, 0.01)]


@functools.lru_cache(maxsize=None)
def _delta_case(B0, cnt, Kc, N):
    """Dense operands of one shape and their fp64 pre-activation / magnitude sums (computed once, read-only)."""
    g = torch.Generator().manual_seed(1000 * B0 + 10 * cnt + Kc + N)
    M = cnt * B0
    Tm, Ws, y0 = torch.randn(M, Kc, generator=g), torch.randn(N, Kc, generator=g), torch.randn(B0, N, generator=g)
    pre = y0.double().repeat(cnt, 1) - Tm.double() @ Ws.double().T          # row r reads y0[r % B0]
    mag = y0.double().abs().repeat(cnt, 1) + Tm.double().abs() @ Ws.double().abs().T
    return Tm, Ws, y0, pre, mag


def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("B0,cnt,Kc,N", DELTA_SHAPES)
@pytest.mark.parametrize("relu,slope", ACTS)
@pytest.mark.parametrize("cfg", range(7))
def test_prefix_delta_every_tile_config(cuda, cfg, relu, slope, B0, cnt, Kc, N):
    """out[r] = act(y0[r % B0] - T @ Wsub^T) with DENSE random T and Wsub (triangular operands would hide an
    error in the K tail behind their zeros), against fp64.

    Bound per element, before the activation:  (Kc + 4) * 2^-24 * (|y0[r % B0]| + (|T| @ |Wsub|^T)[r]).
    The fp32 MFMA is a k-ordered fma chain with one rounding per k step (Kc roundings, each relative to a
    partial sum that the magnitude sum bounds); one rounding each for the -1 scale, the residual add and
    the LeakyReLU multiply, and the fourth unit covers the fp32 rounding of the slope itself (the
    reference multiplies by the fp64 0.01). The activation has slope <= 1, so |act(a) - act(b)| <= |a - b|
    and the bound carries through it. Nothing here is fitted to the kernel's output.

    Also: with T = 0 the accumulator contributes exactly zero (values equal act(y0[r % B0])); the same
    operands give the same bits twice (no atomics); one NaN in y0[b, n] reaches out[j*B0 + b, n] for every
    j and nothing else; one NaN in row r of T reaches row r of out and no other row."""
    T = ops.require()
    Tm, Ws, y0, pre, mag = _delta_case(B0, cnt, Kc, N)
    M = cnt * B0
    Td, Wd, yd = Tm.to(cuda), Ws.to(cuda), y0.to(cuda)
    neg1 = -torch.ones(N, device=cuda)
    out = T.prefix_delta(Td, Wd, neg1, yd, relu, slope, cfg)
    assert tuple(out.shape) == (M, N)
    err = (out.double().cpu() - _act64(pre, relu, slope)).abs()
    bound = (Kc + 4) * U24 * mag
    ratio = float((err / bound).max())
    print(f"shapley_delta b cfg={cfg} relu={int(relu)} slope={slope} B0={B0} cnt={cnt} Kc={Kc} N={N} "
          f"max_err_over_bound={ratio:.4f}")
    assert bool((err <= bound).all()), f"max err / bound = {ratio}"
    # the same bits from a second call
    assert _same_bits(T.prefix_delta(Td, Wd, neg1, yd, relu, slope, cfg), out)
    # T = 0: the fp32 activation of the broadcast residual, exactly (the sign of a zero is not pinned)
    y_rep = y0.repeat(cnt, 1)
    want0 = torch.where(y_rep > 0, y_rep, y_rep * torch.tensor(slope, dtype=torch.float32)) if relu else y_rep
    out0 = T.prefix_delta(torch.zeros_like(Td), Wd, neg1, yd, relu, slope, cfg).cpu()
    assert bool((out0 == want0).all())
    # one NaN in the residual: that (b, n) of every row block, nothing else
    b, n = B0 // 2, N - 1
    yn = y0.clone()
    yn[b, n] = float("nan")
    outn = T.prefix_delta(Td, Wd, neg1, yn.to(cuda), relu, slope, cfg).cpu()
    hit = torch.zeros(M, N, dtype=torch.bool)
    hit[b::B0, n] = True
    assert torch.equal(torch.isnan(outn), hit)
    assert _same_bits(outn[~hit], out.cpu()[~hit])
    # one NaN in the last row of T (last K column): that row of out, no other row
    r = M - 1
    Tn = Tm.clone()
    Tn[r, Kc - 1] = float("nan")
    outr = T.prefix_delta(Tn.to(cuda), Wd, neg1, yd, relu, slope, cfg).cpu()
    hit = torch.zeros(M, N, dtype=torch.bool)
    hit[r] = True
    assert torch.equal(torch.isnan(outr), hit)
    assert _same_bits(outr[~hit], out.cpu()[~hit])


# ------------------------------------------------------------------------------------------ composition
# (B, C, N, p0, cnt); the permutation covers all C units
COMPOSE_CASES = [(5, 40, 12, 0, 1), (5, 40, 12, 9, 32),
                 (5, 40, 12, 20, 21),       # the last copy has every unit removed
                 (20, 200, 68, 100, 40)]


@functools.lru_cache(maxsize=None)
def _compose_case(B, C, N, p0, cnt):
    g = torch.Generator().manual_seed(7 * B + C + N + 3 * p0 + cnt)
    z, W, bias = torch.randn(B, C, generator=g), torch.randn(N, C, generator=g), torch.randn(N, generator=g)
    perm = torch.randperm(C, generator=g).to(torch.int32)
    rank = torch.empty(C, dtype=torch.long)
    rank[perm.long()] = torch.arange(C)
    z64, W64 = z.double(), W.double()
    keep = (rank.view(1, C) >= (p0 + torch.arange(cnt)).view(cnt, 1)).double()            # (cnt, C)
    pre = torch.einsum("jc,bc,nc->jbn", keep, z64, W64) + bias.double()                   # masked copies
    y0 = pre[0].float()                                                                   # rounded on the host
    gone = keep[0].view(1, C) - keep                                                      # units p0 .. p0+j-1
    mag = torch.einsum("jc,bc,nc->jbn", gone, z64.abs(), W64.abs())                       # (|T| @ |Wsub|^T)[j, b]
    return z, W, perm, y0, pre.reshape(cnt * B, N), mag.reshape(cnt * B, N)


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,N,p0,cnt", COMPOSE_CASES)
@pytest.mark.parametrize("relu,slope", [(True, 0.01), (False, 0.0)])
@pytest.mark.parametrize("cfg", [0, 2, 5])
def test_prefix_delta_composition_vs_masked_copies(cuda, cfg, relu, slope, B, C, N, p0, cnt):
    """Both kernels together against fp64 masked copies of a Linear:
    ref_j = act((z * (rank >= p0 + j)) @ W^T + b), y0 = fp32(ref pre-activation of j = 0). This is the test
    that fails when T and Wsub disagree about the dropped column or the prefix offset.

    Bound: as in the tile-config test with the chain length cnt in place of Kc (columns cnt-1 .. Kc-1 of both
    operands are zero and add exactly nothing), plus 2^-24 * |y0| for the rounding of y0 to fp32:
    (cnt + 4) * 2^-24 * (|y0| + (|T| @ |Wsub|^T)[r]) + 2^-24 * |y0|, the magnitude sum taken over the units
    copy j removed beyond the base prefix.

    Finite inputs only: with a non-finite activation in an already-removed unit the delta form gives NaN
    (inf - inf) where a masked copy gives a finite value. That is a property of the method, not tested."""
    T = ops.require()
    z, W, perm, y0, pre, mag = _compose_case(B, C, N, p0, cnt)
    Kc = -(-cnt // 32) * 32
    tri, wsub = T.prefix_tri_operands(z.to(cuda), W.to(cuda), perm.to(cuda), p0, cnt, Kc)
    # the two operands agree on the dropped column: both are exactly zero from column cnt-1 on (an extra
    # column in only one of them would meet zeros in the other and leave the product unchanged)
    assert not bool(tri[:, cnt - 1:].any()) and not bool(wsub[:, cnt - 1:].any())
    out = T.prefix_delta(tri, wsub, -torch.ones(N, device=cuda), y0.to(cuda), relu, slope, cfg)
    assert tuple(out.shape) == (cnt * B, N)
    y_abs = y0.double().abs().repeat(cnt, 1)
    bound = (cnt + 4) * U24 * (y_abs + mag) + U24 * y_abs
    err = (out.double().cpu() - _act64(pre, relu, slope)).abs()
    ratio = float((err / bound).max())
    print(f"shapley_delta c cfg={cfg} relu={int(relu)} slope={slope} B={B} C={C} N={N} p0={p0} cnt={cnt} "
          f"max_err_over_bound={ratio:.4f}")
    assert bool((err <= bound).all()), f"max err / bound = {ratio}"


# ---------------------------------------------------------------------------------------- engine wiring
@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1])
def test_engine_prefix_delta_per_sample_losses(cuda, k):
    """``engine.prefix_delta_loss`` at the two delta-capable points of the pruned-width MLP (k = 0: hidden
    layer, N4 = 200 of 197; k = 1: last hidden layer feeding the 10-logit Linear, N4 = 12 sliced back to
    10), per prefix and sample: the (cnt, B) losses against the engine's masked-copy path
    (``loss_from`` on ``prefix_mask`` copies) and an fp64 CPU evaluation of the model with the same units
    zeroed. max|delta - fp64| <= 3 * max|copies - fp64| + 2e-6 per (p0, cnt) case: the yardstick is the
    masked-copy path against the reference, the figures are those of
    test_mlp_engine_gpu.py::test_shapley_prefix_delta_matches_masked_copies."""
    from torchpruner_amd import ShapleyAttributionMetric
    from torchpruner_amd.attributions.methods.shapley import _PermOf, _RankPadder
    from torchpruner_amd.engine import maybe_engine
    from torchpruner_amd.engine.fused_chain import TUNER
    model = _fcnet(odd=True).to(cuda)
    g = torch.Generator().manual_seed(21 + k)
    x = torch.randn(5, 784, generator=g)
    y = torch.randint(0, 10, (5,), generator=g)
    act = model.fc[2 + 2 * k]
    m64 = copy.deepcopy(model).double().cpu()
    gone = []  # units the hook zeroes
    m64.fc[2 + 2 * k].register_forward_hook(
        lambda mod, inp, out: out.index_fill(1, torch.as_tensor(gone, dtype=torch.long), 0.0))
    with TUNER.fixed(), torch.no_grad():
        eng, idx = maybe_engine(model, [act], F.cross_entropy, cuda)
        assert list(idx) == [k] and eng.prefix_delta_ok(k)
        zk, _ = eng.forward(x.to(cuda), stop_after=k)
        n = eng.real_width(k)
        assert n == (198, 197)[k] and zk.shape[0] == 5
        perm = np.random.RandomState(5 + k).permutation(n)
        rank_t = ShapleyAttributionMetric._rank_of(perm, cuda)
        perm_t, rank_p = _PermOf()(rank_t), _RankPadder(n)(rank_t, zk.shape[3])
        assert perm_t.dtype == torch.int32 and perm_t.cpu().tolist() == perm.tolist()
        yd = y.to(cuda)
        for p0, cnt in ((0, 1), (3, 33), (n - 4, 5)):  # the last copy of the last case has every unit removed
            delta = eng.prefix_delta_loss(k, zk, perm_t, rank_p, p0, cnt, yd, None)
            masked = ops.prefix_mask(zk.permute(0, 3, 1, 2), rank_p, p0, cnt)
            copies = eng.loss_from(k, masked.permute(0, 2, 3, 1), yd.repeat(cnt), None).view(cnt, 5)
            ref = []
            for j in range(cnt):
                gone[:] = perm[:p0 + j].tolist()
                ref.append(F.cross_entropy(m64(x.double()), y, reduction="none"))
            ref = torch.stack(ref)
            assert tuple(delta.shape) == tuple(copies.shape) == tuple(ref.shape) == (cnt, 5)
            e_d = float((delta.double().cpu() - ref).abs().max())
            e_c = float((copies.double().cpu() - ref).abs().max())
            print(f"shapley_delta d k={k} p0={p0} cnt={cnt} max_err_delta={e_d:.3e} max_err_copies={e_c:.3e}")
            assert e_d <= 3 * e_c + 2e-6, (k, p0, cnt, e_d, e_c)
