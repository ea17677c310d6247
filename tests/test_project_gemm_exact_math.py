"""Operand generators, float64 references and case tables of tests/test_project_gemm_exact_gpu.py, and the CPU
half of its claims: wherever that file asks a project GEMM kernel (scaled_project.hip, silu_project.hip,
silu_prefix_project.hip) for EQUALITY with float64, the reference must survive float32
(``ref == ref.float().double()``) and the sum of absolute terms must stay below 2^24, so every partial sum is
an exactly representable number in any summation order. Both are asserted here, where the float64 bodies run,
for every parametrised case.

* ``scaled_project``: integer a, wt, bias, res and sc in {0, 0.5, 1, 2}: every product is a multiple of 0.5.
* the Sensitivity slab of ``silu_project_dgrad``: integer g and wtT give an integer gy; ``slab_ref`` sums |gy|
  per (64-row tile, image) into slot ``tile - first tile of the image``, the kernel's documented layout.
* one-hot weights (``silu_prefix_project``, ``silu_project_fwd``): an output element is a single SiLU term, so
  nothing is summed; those tests hold the value to the SiLU's own error and the structure to equality.
"""
import pytest
import torch

SILU_ULP = 6  # twice the kernels' worst SiLU error, 2.96 x 2^-24 x silu(|z|) (profiles/numerics/silu_project.txt)
TILE = 64     # rows per block of the silu_project kernels

# (B, HW, C, Co, cnt): two column tiles + a partial copy group at HW = 1; one K slice, one full column tile and
# one full copy group; N = 64 exactly with three column tiles; the shape that reaches the 64-row-tile branch
SCALED_SHAPES = [(3, 49, 40, 36, 6), (5, 1, 20, 68, 5), (1, 33, 16, 64, 4), (2, 32, 36, 132, 1),
                 (29, 196, 160, 160, 6)]
# (N, C, Co): C <= Co
PREFIX_SHAPES = [(70, 4, 4), (31, 36, 36), (64, 64, 64), (65, 96, 128), (1, 128, 128)]
# (B, HW): 64 | HW (the slot formula's other branch), 63 / 65 around it, many images per tile, straddling tiles
SLAB_GEOMS = [(2, 64), (2, 128), (1, 192), (3, 63), (3, 65), (70, 1), (2, 49), (3, 150)]
SLAB_C = [4, 64, 132]   # one partial column chunk of the dgrad, one exact, three
SLAB_CO = [4, 40]
FWD_GEOMS = [(2, 64), (3, 65), (70, 1)]
FWD_C = [4, 36, 64, 128]
_CACHE = {}


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def silu_z(g, shape):
    """+-uniform[2^-6, 12]: clear of denormal products and of the exponential's overflow."""
    mag = torch.rand(shape, generator=g) * (12 - 2.0 ** -6) + 2.0 ** -6
    return torch.where(torch.rand(shape, generator=g) < 0.5, -mag, mag)


def silu64(z):
    z = z.double()
    return z * torch.sigmoid(z)


def scaled_case(B, HW, C, Co, cnt):
    """Operands (float32, integer-valued up to sc's halves), the float64 body without res, and its magnitude."""
    key = ("scaled", B, HW, C, Co, cnt)
    if key not in _CACHE:
        from torchpruner_amd import ops
        g = torch.Generator().manual_seed(B * 1000 + HW + C + Co + cnt)
        N = B * HW
        a = _ints(g, (N, C), 4)
        sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cnt, B, C), generator=g)]
        sc = torch.where(torch.rand(cnt, B, C, generator=g) < 0.25, torch.zeros(()), sc)  # masked channels
        wt, bias, res = _ints(g, (C, Co), 4), _ints(g, (cnt, B, Co), 8), _ints(g, (N, Co), 8)
        ref = ops.scaled_project(a.double(), sc.double(), wt.double(), bias.double(), None, hw=HW)
        mag = ops.scaled_project(a.double().abs(), sc.double(), wt.double().abs(), bias.double().abs(),
                                 res.double().abs(), hw=HW)
        _CACHE[key] = (a, sc, wt, bias, res, ref, mag)
    return _CACHE[key]


def prefix_case(N, C, Co):
    """One-hot weights over n real channels and C - n padding channels (ranked after them, never masked)."""
    g = torch.Generator().manual_seed(N * 10000 + C * 200 + Co)
    n = C - (1 if C == 4 else 3)
    perm = torch.randperm(n, generator=g)
    rank = torch.full((C,), n + 1)
    rank[perm] = torch.arange(n)
    wt = torch.zeros(C, Co)
    wt[torch.arange(C), torch.arange(C)] = 1.0
    return {"z": silu_z(g, (N, C)), "wt": wt, "shift": torch.zeros(Co), "perm": perm.int(), "rank": rank.int(), "n": n}


def prefix_ranges(n):
    return [(0, n + 1), (3, min(34, n - 2)), (n, 1)]


def slab_case(B, HW, C, Co):
    key = ("slab", B, HW, C, Co)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(B * 1000 + HW * 7 + C + Co)
        N = B * HW
        gr, wtT = _ints(g, (N, Co), 8), _ints(g, (Co, C), 3)
        z = torch.randn(N, C, generator=g) * 3
        _CACHE[key] = (gr, wtT, z, (gr.double() @ wtT.double()).abs())
    return _CACHE[key]


def slab_ref(term, B, HW, R):
    """(R, B, C) float64: ``term`` (N, C) summed over the rows of image b inside 64-row tile t, in slot
    t - (b HW) // 64."""
    out = torch.zeros(R, B, term.shape[1], dtype=torch.float64)
    for b in range(B):
        first = (b * HW) // TILE
        for t in range(first, ((b + 1) * HW - 1) // TILE + 1):
            lo, hi = max(b * HW, t * TILE), min((b + 1) * HW, (t + 1) * TILE)
            assert 0 <= t - first < R
            out[t - first, b] = term[lo:hi].sum(0)
    return out


def fwd_case(B, HW, C):
    g = torch.Generator().manual_seed(B * 1000 + HW * 7 + C)
    return silu_z(g, (B * HW, C))


def representable(ref, mag):
    return bool(torch.equal(ref, ref.float().double())) and float(mag.max()) < 2.0 ** 24


@pytest.mark.parametrize("B,HW,C,Co,cnt", SCALED_SHAPES)
def test_scaled_reference_survives_float32(B, HW, C, Co, cnt):
    a, sc, wt, bias, res, ref, mag = scaled_case(B, HW, C, Co, cnt)
    assert a.abs().max() <= 4 and wt.abs().max() <= 4 and bias.abs().max() <= 8 and res.abs().max() <= 8
    assert set(sc.unique().tolist()) <= {0.0, 0.5, 1.0, 2.0} and 0.15 < float((sc == 0).float().mean()) < 0.35
    assert torch.equal(ref * 2, (ref * 2).round())  # multiples of 0.5
    assert representable(ref, mag)
    with_res = ref + res.double().view(1, B * HW, Co)
    assert representable(with_res, mag)


@pytest.mark.parametrize("Co", SLAB_CO)
@pytest.mark.parametrize("C", SLAB_C)
@pytest.mark.parametrize("B,HW", SLAB_GEOMS)
def test_slab_reference_survives_float32_and_covers_every_row(B, HW, C, Co):
    from torchpruner_amd import ops
    gr, wtT, z, term = slab_case(B, HW, C, Co)
    R = ops.silu_project_tay_slots(HW, C)
    ref = slab_ref(term, B, HW, R)
    assert torch.equal(term, term.round()) and representable(term, gr.double().abs() @ wtT.double().abs())
    assert representable(ref, ref) and torch.equal(ref.sum(0), term.view(B, HW, C).sum(1))
    # the body puts the whole sum into slot 0: the same total
    body = torch.zeros(R, B, C, dtype=torch.float64)
    ops.silu_project_dgrad(gr.double(), z.double(), wtT.double(), body, 1)
    assert torch.equal(body.sum(0), ref.sum(0))
    # every slot of the formula is used by some image of a long enough batch: R is tight
    used = {(t - (b * HW) // TILE) for b in range(64) for t in range((b * HW) // TILE, ((b + 1) * HW - 1) // TILE + 1)}
    assert used == set(range(R))


@pytest.mark.parametrize("N,C,Co", PREFIX_SHAPES)
def test_one_hot_prefix_cases_are_single_terms(N, C, Co):
    from torchpruner_amd import ops
    t = prefix_case(N, C, Co)
    n = t["n"]
    assert 2.0 ** -6 <= float(t["z"].abs().min()) and float(t["z"].abs().max()) <= 12 and C <= Co
    assert sorted(t["rank"][t["perm"].long()].tolist()) == list(range(n)) and int((t["rank"] > n).sum()) == C - n
    s = silu64(t["z"])
    for p0, cnt in prefix_ranges(n):
        assert cnt >= 1 and p0 + cnt - 1 <= n
        ref = ops.silu_prefix_project(t["z"].double(), t["wt"].double(), t["shift"].double(), None, t["perm"],
                                      t["rank"], p0, cnt)
        keep = t["rank"].view(1, 1, C) >= torch.arange(p0, p0 + cnt).view(cnt, 1, 1)
        assert torch.equal(ref[:, :, :C], torch.where(keep, s, torch.zeros((), dtype=torch.float64)))
        assert not ref[:, :, C:].any()
        if p0 + cnt - 1 == n:  # every real channel masked: the last copy is the padding channels alone
            assert not ref[-1][:, :C][:, t["rank"] < n].any() and ref[-1][:, :C][:, t["rank"] > n].all()
