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


def _case(C, Co, seed=0):
    """n real channels and 1 (C = 4) or 3 padding channels that rank after them."""
    g = torch.Generator().manual_seed(seed * 10000 + C * 200 + Co)
    n = C - (1 if C == 4 else 3)
    perm = torch.randperm(n, generator=g)
    rank = torch.full((C,), n + 1)
    rank[perm] = torch.arange(n)
    return {"z": torch.randn(N, C, generator=g) * 3, "wt": torch.randn(C, Co, generator=g),
            "shift": torch.randn(Co, generator=g), "res": torch.randn(N, Co, generator=g) * 3,
            "perm": perm.int(), "rank": rank.int()}


def _check(cuda, t, p0, cnt, with_res, label):
    from torchpruner_amd import ops
    C = t["z"].shape[1]
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
