"""The LDS-staged SiLU depthwise kernels (csrc/kernels/dwconv_silu.hip) at the edges of their band
arithmetic, bit for bit.

Shapes (EDGES): a last column band narrower than the others (33 = 17 + 16, 65 = 22 + 22 + 21), a middle
column band with halo on both sides, several column bands under a stride-2 forward, even H at stride 2,
dgrad row bands that start on an odd row at stride 2 (rbh 3 and 5), a one-row last band
(21 = 5 + 5 + 5 + 5 + 1), pad 0 and pad k - 1, a row split between 1 and the finest (B = 300: 4 bands in
a slab of 5 slots), and three channel slices with a ragged last one. Each case lists the split it was
chosen for, (tw, ncb, bw, nsl, nrb, rbh, slots), of the forward's output map and of the dgrad's input
map; the GPU test asserts it through dwconv_silu_tile, so a retuned tile fails here, not silently.

Exact regime: z has integer magnitudes in [100, 131] with random signs, w integers in [-2, 2], scale in
{1, 2}, shift 16384, g integers in [-3, 3]. The kernels' sigmoid is 0 at -100 and 1 at +100 (the
numerics contract of the kernel file's header), so in_act = 4 gives a = max(z, 0) and the slope [z > 0];
|conv| <= 25 * 2 * 131 = 6550, so v = scale * conv + 16384 lies in [3284, 29484], y = v and silu'(v) = 1;
|dA| <= 25 * 2 * 3 * 2 = 300 and |dA * a| <= 39300. Every value is an integer below 2^24 and so is
every partial sum, in any order, while the sum of the magnitudes stays below 2^24 (asserted on the
CPU): fp32 computes all of it exactly and the comparison needs no tolerance. The reference is written
here in fp64 with the saturated activations substituted (clamp_min(0) and z > 0); the CPU test holds
the fp64 bodies of ops/dwconv_silu.py, the oracle of the smooth-regime test, to it within 1e-30: they
differ only by terms around 1e-38 from sigmoid(-100) != 0 in fp64.

The smooth regime (real SiLU arithmetic, fp64 bodies, tolerances) runs the same shapes in
test_dwconv_silu_gpu.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

# (B, H, W, C), the dgrad's split of the (H, W) map, [((k, s, pad), the forward's split of the (Ho, Wo) map)]
EDGES = [
    ((1, 8, 33, 8), (32, 2, 17, 1, 2, 4, 4),
     [((3, 1, 1), (32, 2, 17, 1, 2, 4, 4)), ((5, 1, 2), (32, 2, 17, 1, 2, 4, 4)),
      ((3, 2, 1), (32, 1, 17, 1, 1, 4, 1)), ((5, 2, 2), (32, 1, 17, 1, 1, 4, 1))]),
    ((1, 6, 66, 8), (32, 3, 22, 1, 2, 3, 6),
     [((3, 2, 1), (32, 2, 17, 1, 1, 3, 2)), ((5, 2, 2), (32, 2, 17, 1, 1, 3, 2)),
      ((3, 1, 1), (32, 3, 22, 1, 2, 3, 6))]),
    ((1, 4, 65, 8), (32, 3, 22, 1, 1, 4, 3),
     [((5, 1, 2), (32, 3, 22, 1, 1, 4, 3)), ((3, 1, 1), (32, 3, 22, 1, 1, 4, 3))]),
    ((1, 21, 3, 8), (8, 1, 3, 1, 5, 5, 5),
     [((3, 1, 1), (8, 1, 3, 1, 5, 5, 5)), ((5, 1, 2), (8, 1, 3, 1, 5, 5, 5)),
      ((3, 2, 1), (8, 1, 2, 1, 3, 4, 3)), ((5, 2, 2), (8, 1, 2, 1, 3, 4, 3))]),
    ((2, 12, 12, 8), (16, 1, 12, 1, 3, 4, 3),
     [((3, 2, 1), (8, 1, 6, 1, 2, 3, 2)), ((5, 2, 2), (8, 1, 6, 1, 2, 3, 2)), ((3, 2, 0), (8, 1, 5, 1, 1, 5, 1)),
      ((5, 1, 4), (16, 1, 16, 1, 4, 4, 4)), ((3, 1, 0), (16, 1, 10, 1, 3, 4, 3))]),
    ((1, 9, 14, 8), (16, 1, 14, 1, 2, 5, 2),
     [((3, 2, 1), (8, 1, 7, 1, 1, 5, 1)), ((5, 2, 2), (8, 1, 7, 1, 1, 5, 1)), ((5, 1, 2), (16, 1, 14, 1, 2, 5, 2))]),
    ((300, 19, 4, 8), (8, 1, 4, 1, 4, 5, 5),
     [((5, 1, 2), (8, 1, 4, 1, 4, 5, 5)), ((3, 2, 1), (8, 1, 2, 1, 3, 4, 3))]),
    ((2, 10, 16, 136), (16, 1, 16, 3, 3, 4, 3),
     [((3, 1, 1), (16, 1, 16, 3, 3, 4, 3)), ((5, 2, 2), (8, 1, 8, 2, 1, 5, 1))]),
]
CASES = [(shape, ksp, fsplit, dsplit) for shape, dsplit, lst in EDGES for ksp, fsplit in lst]
IDS = ["x".join(map(str, shape)) + "-k%ds%dp%d" % ksp for shape, ksp, _, _ in CASES]
EXACT = float(1 << 24)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _band_sums(m, split):
    """(B, rows, cols, C) -> the (slots, B, C) slab: slot rb * ncb + cb holds the sum over the pixels of
    row band rb and column band cb, every other slot 0"""
    _, ncb, bw, _, nrb, rbh, slots = split
    out = torch.zeros(slots, m.shape[0], m.shape[3], dtype=m.dtype)
    for rb in range(nrb):
        for cb in range(ncb):
            out[rb * ncb + cb] = m[:, rb * rbh:(rb + 1) * rbh, cb * bw:(cb + 1) * bw].sum((1, 2))
    return out


@functools.lru_cache(maxsize=None)
def _exact(shape, ksp, in_act):
    """fp32 inputs of the exact regime and their fp64 reference with the saturated activations; computed
    once per case and shared (read only) by the CPU and the GPU test"""
    (B, H, W, C), (k, s, pad) = shape, ksp
    gen = torch.Generator().manual_seed(1000 * H + 100 * W + 10 * k + s + 7 * pad + in_act)
    ri = lambda lo, hi, *size: torch.randint(lo, hi + 1, size, generator=gen).float()
    z = ri(100, 131, *shape) * (2 * ri(0, 1, *shape) - 1)
    w, scale, shift = ri(-2, 2, C, 1, k, k), ri(1, 2, C), torch.full((C,), 16384.0)
    w[C - 4:], scale[C - 4:], shift[C - 4:] = 0.0, 0.0, 0.0  # padded channels: finite garbage z
    z[..., C - 4:] = torch.randn(B, H, W, 4, generator=gen) * 1e3
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    g = ri(-3, 3, B, Ho, Wo, C)

    d = lambda t: t.double()
    a = d(z).clamp_min(0) if in_act else d(z)
    v = F.conv2d(_nchw(a), d(w), None, s, pad, 1, C).permute(0, 2, 3, 1) * d(scale) + d(shift)  # y = v: sigmoid(v) = 1
    gm = d(g) * d(scale)  # silu'(v) = 1
    dA = torch.nn.grad.conv2d_input((B, C, H, W), d(w), _nchw(gm).contiguous(), s, pad, 1, C).permute(0, 2, 3, 1)
    return {"z": z, "w": w, "scale": scale, "shift": shift, "g": g, "y": v.contiguous(),
            "apoz": (v > 0).sum((1, 2)).double(), "dz": (dA * (d(z) > 0) if in_act else dA).contiguous(),
            "term": (-(dA * a), dA.abs())}


@pytest.mark.parametrize("in_act", [0, 4])
@pytest.mark.parametrize("shape,ksp,fsplit,dsplit", CASES, ids=IDS)
def test_exact_reference(shape, ksp, fsplit, dsplit, in_act):
    """The fp64 bodies agree with the saturated reference within 1e-30, and every reference value, every
    per-slot sum and the magnitudes summed per slot stay below 2^24: fp32 holds all of them exactly."""
    from torchpruner_amd import ops
    (B, H, W, C), (k, s, pad), r = shape, ksp, _exact(shape, ksp, in_act)
    d = lambda t: t.double()
    near = lambda got, ref: got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-30
    Ho, Wo = r["y"].shape[1:3]
    for split, rows, cols in ((fsplit, Ho, Wo), (dsplit, H, W)):  # the bands cover the map, none is empty
        _, ncb, bw, _, nrb, rbh, slots = split
        assert (ncb - 1) * bw < cols <= ncb * bw and (nrb - 1) * rbh < rows <= nrb * rbh and nrb * ncb <= slots
    apoz, pre = torch.zeros(B, C, dtype=torch.float64), torch.empty_like(r["y"])
    pool = torch.zeros(ops.dwconv_silu_pool_slots(Ho, Wo, C), B, C, dtype=torch.float64)
    y = ops.dwconv_silu_fwd(d(r["z"]), d(r["w"]), d(r["scale"]), d(r["shift"]), s, pad, in_act, 4, apoz, pre, pool)
    assert near(y, r["y"]) and near(pre, r["y"]) and torch.equal(apoz, r["apoz"])
    assert near(pool.sum(0), r["y"].sum((1, 2))) and pool.shape[0] == fsplit[6]
    assert torch.equal(r["apoz"][:, :C - 4], torch.full((B, C - 4), float(Ho * Wo), dtype=torch.float64))
    for mode in (0, 1):
        tay = torch.zeros(ops.dwconv_silu_tay_slots(H, W, C), B, C, dtype=torch.float64)
        dz = ops.dwconv_silu_dgrad(d(r["g"]), r["y"], d(r["w"]), d(r["scale"]), d(r["z"]), H, W, s, pad, in_act, 4, tay,
                                   mode)
        assert near(dz, r["dz"]) and near(tay.sum(0), r["term"][mode].sum((1, 2))) and tay.shape[0] == dsplit[6]
    for m in (r["y"], r["dz"], *r["term"]):
        assert torch.equal(m, m.round()) and float(m.abs().max()) < EXACT
    assert float(_band_sums(r["y"].abs(), fsplit).max()) < EXACT
    assert max(float(_band_sums(t.abs(), dsplit).max()) for t in r["term"]) < EXACT
    pad_c = slice(C - 4, C)
    assert all(not m[..., pad_c].any() for m in (r["y"], r["dz"], *r["term"], r["apoz"]))


def _same(got, ref, what):
    """bit-for-bit (as values: -0 == 0) against the float32 cast of the fp64 reference"""
    got, ref = got.cpu(), ref.float()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {ref.numel()} differ, first at {i}: {float(got[i])} != {float(ref[i])}")


@pytest.mark.gpu
@pytest.mark.parametrize("in_act", [0, 4])
@pytest.mark.parametrize("shape,ksp,fsplit,dsplit", CASES, ids=IDS)
def test_dwconv_silu_exact(cuda, shape, ksp, fsplit, dsplit, in_act):
    from torchpruner_amd import ops
    T = ops.require()
    (B, H, W, C), (k, s, pad), r = shape, ksp, _exact(shape, ksp, in_act)
    Ho, Wo = r["y"].shape[1:3]
    # the split this case was chosen for is the one the launchers take: [tw, lq, ncb, bw, nsl, nrb, rbh, slots]
    for split, rows, cols in ((fsplit, Ho, Wo), (dsplit, H, W)):
        t = list(T.dwconv_silu_tile(B, rows, cols, C))
        assert len(t) == 8 and 2 ** t[1] * t[0] == 256 and tuple(t[:1] + t[2:]) == split, (t, split)
    assert T.dwconv_silu_pool_slots(Ho, Wo, C) == fsplit[6] and T.dwconv_silu_tay_slots(H, W, C) == dsplit[6]

    zc, wc, scc, shc, gc = (r[n].to(cuda) for n in ("z", "w", "scale", "shift", "g"))
    apoz, pre = torch.zeros(B, C, device=cuda), torch.full(r["y"].shape, float("nan"), device=cuda)
    pool = torch.zeros(fsplit[6], B, C, device=cuda)
    y = T.dwconv_silu_fwd(zc, wc, scc, shc, s, pad, in_act, 4, apoz, pre, pool)
    _same(y, r["y"], "y")
    _same(pre, r["y"], "pre")
    _same(apoz, r["apoz"], "apoz")
    _same(pool, _band_sums(r["y"], fsplit), "pool slots")  # each band in its own slot, zeros in all others
    assert not pool[fsplit[4] * fsplit[1]:].any(), "a slot past nrb * ncb was written"
    pad_c = slice(C - 4, C)
    assert not y[..., pad_c].any() and not pre[..., pad_c].any() and not apoz[:, pad_c].any()
    assert not pool[..., pad_c].any()

    vc = r["y"].float().to(cuda)  # the dgrad is checked on the reference's pre-activation, not the forward's
    for mode in (0, 1):
        tay = torch.zeros(dsplit[6], B, C, device=cuda)
        dz = T.dwconv_silu_dgrad(gc, vc, wc, scc, zc, H, W, s, pad, in_act, 4, tay, mode)
        _same(dz, r["dz"], f"dz (tay_mode {mode})")
        _same(tay, _band_sums(r["term"][mode], dsplit), f"tay slots (tay_mode {mode})")
        assert not tay[dsplit[4] * dsplit[1]:].any(), "a slot past nrb * ncb was written"
        assert not dz[..., pad_c].any() and not tay[..., pad_c].any()


@pytest.mark.gpu
def test_dwconv_silu_tile_binding(cuda):
    from torchpruner_amd import ops
    T = ops.require()
    assert list(T.dwconv_silu_tile(1, 112, 112, 32)) == [32, 3, 4, 28, 1, 28, 4, 112]
    assert list(T.dwconv_silu_tile(32, 112, 112, 32)) == [32, 3, 4, 28, 1, 8, 14, 112]
    for bad in [(0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 6), (1, 8, 8, 0), (1, 1 << 26, 1, 4),
                (1 << 24, 1, 1, 4), (1, 1 << 40, 1, 4), (1 << 31, 8, 8, 8)]:
        assert list(T.dwconv_silu_tile(*bad)) == [], bad
