"""``ops.silu_prefix_project`` (csrc/kernels/silu_prefix_project.hip) against its float64 body, and the
binding's rejections. Bound per element: (C + cnt + 10) 2^-24 times the sum of absolute terms of copy 0 (the
body on absolute operands: every partial sum of every copy is below it). C + 1: the C products of the GEMM,
each rounded and added; cnt: one fused multiply-subtract per step; 2: shift and res; 6: twice the kernel's
SiLU error (2.96 x 2^-24 silu(|z|), profiles/numerics/silu_project.txt: the same formula), once in the GEMM
and once in a step; rounded up to 10. Figures: profiles/numerics/silu_prefix_project.txt."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C_ULP = 10
N = 2 * 5 * 7  # two 64-row tiles, the second one partial


def _case(C, Co, seed=0, N=N):
    """n real channels and 1 (C = 4) or 3 padding channels that rank after them."""
    g = torch.Generator().manual_seed(seed * 10000 + C * 200 + Co + (0 if N == 70 else N * 1000000))
    n = C - (1 if C == 4 else 3)
    perm = torch.randperm(n, generator=g)
    rank = torch.full((C,), n + 1)
    rank[perm] = torch.arange(n)
    return {"z": torch.randn(N, C, generator=g) * 3, "wt": torch.randn(C, Co, generator=g),
            "shift": torch.randn(Co, generator=g), "res": torch.randn(N, Co, generator=g) * 3,
            "perm": perm.int(), "rank": rank.int()}


def _check(cuda, t, p0, cnt, with_res, label):
    from torchpruner_amd import ops
    N, C = t["z"].shape
    cnt = min(cnt, t["perm"].numel() + 1 - p0)  # the prefixes a permutation of n channels has from p0 on

    def run(f, g, cnt=cnt):
        return ops.silu_prefix_project(g(f(t["z"])), g(f(t["wt"])), g(f(t["shift"])), g(f(t["res"])) if with_res else None,
                                       f(t["perm"]), f(t["rank"]), p0, cnt)
    got, again = run(lambda v: v.to(cuda), lambda v: v), run(lambda v: v.to(cuda), lambda v: v)
    ref = run(lambda v: v.double() if v.is_floating_point() else v, lambda v: v)
    mag = run(lambda v: v.double() if v.is_floating_point() else v, torch.abs, 1)
    assert got.shape == ref.shape == (cnt, N, t["wt"].shape[1])
    assert torch.equal(got, again) and torch.isfinite(got).all()
    r = float(((got.double().cpu() - ref).abs() / ((C + cnt + C_ULP) * 2.0 ** -24 * mag)).max())
    print(f"silu_prefix_project {label} p0={p0} cnt={cnt} res={int(with_res)}: worst error / bound = {r:.4f}")
    assert r <= 1.0


# C: one partial K slice, one full + one partial, three full. Co: one, one, four accumulators. cnt: the masked
# GEMM alone, one step, 34 steps (past the 32 of one LDS step tile; clamped to the prefixes a narrow C has).
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("cnt", [1, 2, 35])
@pytest.mark.parametrize("p0", [0, 3])
@pytest.mark.parametrize("Co", [4, 24, 128])
@pytest.mark.parametrize("C", [4, 36, 96])
def test_matches_the_fp64_body(cuda, C, Co, p0, cnt, with_res):
    _check(cuda, _case(C, Co), p0, cnt, with_res, f"C={C} Co={Co}")


# Tile edges. Co: the dispatcher's boundaries (32 | 36: one | two accumulators, 64 | 68: two | four; 36 and 64 run
# the two-accumulator instantiation) and a partly filled four-accumulator tile (100). N: one row, fewer than 32 (the
# second wave owns no valid row), exact multiples of 64, one past. cnt - 1 steps that fill one or two 32-step LDS
# delta tiles exactly (32, 64), overflow them by one (33, 65), and the full scan p0 = 0, cnt = n + 1, whose last copy
# is shift + res plus the padding channels. (p0, cnt) = (n, 1): every real channel masked in the GEMM itself.
EDGES = [(36, Co, N, 3, 35) for Co in (32, 36, 64, 68, 100)]
EDGES += [(36, 40, rows, 3, 35) for rows in (1, 31, 64, 65, 128)]
EDGES += [(96, 40, N, 0, cnt) for cnt in (33, 34, 65, 66, 94)]
EDGES += [(C, 24, N, C - (1 if C == 4 else 3), 1) for C in (4, 36, 96)]


@pytest.mark.parametrize("C,Co,rows,p0,cnt", EDGES)
def test_tile_edges_match_the_fp64_body(cuda, C, Co, rows, p0, cnt):
    t = _case(C, Co, N=rows)
    n = t["perm"].numel()
    assert p0 + cnt - 1 <= n or (p0, cnt) == (3, 35)  # only the 35 is clamped (to n - 2 copies from p0 = 3)
    _check(cuda, t, p0, cnt, True, f"edges N={rows} C={C} Co={Co}")


def test_extreme_pre_activations_stay_finite_and_inside_the_bound(cuda):
    """z at +-100 and +-88 (the exponential overflows / underflows) and 0."""
    t = _case(36, 24)
    vals = torch.tensor([100.0, -100.0, 0.0, 88.0, -88.0, 1.28, -1.28])
    t["z"] = vals[torch.arange(N * 36) % len(vals)].view(N, 36).contiguous()
    _check(cuda, t, 3, 9, True, "extreme")


@pytest.mark.parametrize("name", ["host_operand", "C_not_multiple_of_4", "Co_over_the_limit", "cnt_below_1",
                                  "negative_p0", "range_past_perm", "short_rank", "misaligned_z", "long_perm"])
def test_binding_rejects(cuda, name):
    from torchpruner_amd import ops
    t = {k: v.to(cuda) for k, v in _case(36, 24).items()}
    p0, cnt = 3, 5
    if name == "host_operand":
        t["wt"] = t["wt"].cpu()
    elif name == "C_not_multiple_of_4":
        t["z"], t["wt"], t["rank"] = t["z"][:, :34].contiguous(), t["wt"][:34].contiguous(), t["rank"][:34].contiguous()
    elif name == "Co_over_the_limit":
        t["wt"], t["shift"], t["res"] = (torch.rand(s, device=cuda) for s in ((36, 132), (132,), (N, 132)))
    elif name == "cnt_below_1":
        cnt = 0
    elif name == "negative_p0":
        p0 = -1
    elif name == "range_past_perm":
        p0, cnt = 30, 5  # p0 + cnt - 1 = 34 > n = 33
    elif name == "short_rank":
        t["rank"] = t["rank"][:32].contiguous()
    elif name == "misaligned_z":
        t["z"] = torch.zeros(N * 36 + 1, device=cuda)[1:].view(N, 36)
    elif name == "long_perm":
        t["perm"] = torch.arange(40, device=cuda, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.require().silu_prefix_project(t["z"], t["wt"], t["shift"], t["res"], t["perm"], t["rank"], p0, cnt)
