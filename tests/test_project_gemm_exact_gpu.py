"""Exact and selector tests of the project GEMM kernels (csrc/kernels/scaled_project.hip, silu_project.hip,
silu_prefix_project.hip). The tolerance tests of these kernels compare random operands under a
(K + c) 2^-24 sum-of-|terms| bound, which can absorb a row, channel, column, copy or slot that is off by one;
here such an error cannot hide:

* ``scaled_project`` on integer operands (sc in {0, 0.5, 1, 2}) must EQUAL float64: every product and partial
  sum is a multiple of 0.5 below 2^24, whatever the order.
* ``silu_prefix_project`` and ``silu_project_fwd`` with one-hot weights: an output element is ONE SiLU term.
  Masked elements, columns past C and the copy-to-copy structure are held to equality; the value itself to the
  kernels' SiLU error alone, |out - z sigmoid(z)| <= 6 x 2^-24 x silu(|z|) with the float64 SiLU: 6 is twice
  the worst 2.96 measured for this formula (profiles/numerics/silu_project.txt, that file's unit).
  The masked element of a later copy is exactly 0 because the step subtracts ``xp_silu(z) * 1`` from an
  accumulator that holds the same ``xp_silu(z)``: one function on one input on both paths.
* the Sensitivity slab of ``silu_project_dgrad`` on integer g and wtT: every slot must EQUAL the tile-aware
  float64 reference ``slab_ref`` (slot = tile - first tile of the image), unused slots stay 0, and the slabs
  next to ``tay`` and ``apoz`` inside a larger buffer keep their sentinel.

The operands, references and case tables are in tests/test_project_gemm_exact_math.py, which asserts on the CPU
that every reference asked for equality survives float32. Figures: profiles/numerics/*_project.txt."""
import pytest
import torch

from test_project_gemm_exact_math import (FWD_C, FWD_GEOMS, PREFIX_SHAPES, SCALED_SHAPES, SILU_ULP, SLAB_C, SLAB_CO,
                                          SLAB_GEOMS, fwd_case, prefix_case, prefix_ranges, representable, scaled_case,
                                          silu64, slab_case, slab_ref)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _silu_ratio(got, z):
    """worst |got - silu64(z)| / (2^-24 silu(|z|)) over the elements given."""
    return float(((got.double() - silu64(z)).abs() / (2.0 ** -24 * silu64(z.abs()))).max())


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("B,HW,C,Co,cnt", SCALED_SHAPES)
def test_scaled_project_equals_fp64_on_integer_operands(cuda, B, HW, C, Co, cnt, with_res):
    from torchpruner_amd import ops
    a, sc, wt, bias, res, ref, mag = scaled_case(B, HW, C, Co, cnt)
    if with_res:
        ref = ref + res.double().view(1, B * HW, Co)
    assert representable(ref, mag)
    out = ops.scaled_project(a.to(cuda), sc.to(cuda), wt.to(cuda), bias.to(cuda), res.to(cuda) if with_res else None,
                             hw=HW)
    assert out.shape == (cnt, B * HW, Co) and out.dtype == torch.float32
    assert torch.equal(out.double().cpu(), ref)


@pytest.mark.parametrize("N,C,Co", PREFIX_SHAPES)
def test_silu_prefix_project_one_hot(cuda, N, C, Co):
    """(a) masked elements are exactly 0, (b) the others within the SiLU bound, (c) copy j + 1 equals copy j
    bit for bit outside column perm[p0 + j], (d) columns past C are exactly 0."""
    from torchpruner_amd import ops
    t = prefix_case(N, C, Co)
    n, z, rank, perm = t["n"], t["z"], t["rank"], t["perm"]
    d = {k: v.to(cuda) for k, v in t.items() if k != "n"}
    for p0, cnt in prefix_ranges(n):
        out = ops.silu_prefix_project(d["z"], d["wt"], d["shift"], None, d["perm"], d["rank"], p0, cnt).cpu()
        assert out.shape == (cnt, N, Co)
        keep = (rank.view(1, 1, C) >= torch.arange(p0, p0 + cnt).view(cnt, 1, 1)).expand(cnt, N, C)
        real = out[:, :, :C]
        assert not real[~keep].any(), "(a) a masked element is not exactly 0"
        zz = z.view(1, N, C).expand(cnt, N, C)
        r = _silu_ratio(real[keep], zz[keep])
        print(f"silu_prefix_project one-hot N={N} C={C} Co={Co} p0={p0} cnt={cnt}: worst SiLU error = {r:.3f} x 2^-24 silu(|z|)")
        assert r <= SILU_ULP, "(b)"
        bits = out.view(torch.int32)
        for j in range(cnt - 1):
            same = torch.ones(Co, dtype=torch.bool)
            same[int(perm[p0 + j])] = False
            assert torch.equal(bits[j + 1][:, same], bits[j][:, same]), f"(c) copy {j + 1}"
        assert not out[:, :, C:].any(), "(d) a column past C is not exactly 0"


@pytest.mark.parametrize("Co", SLAB_CO)
@pytest.mark.parametrize("C", SLAB_C)
@pytest.mark.parametrize("B,HW", SLAB_GEOMS)
def test_sensitivity_slab_and_apoz_equal_fp64_per_slot(cuda, B, HW, C, Co):
    from torchpruner_amd import ops
    gr, wtT, z, term = slab_case(B, HW, C, Co)
    R = ops.silu_project_tay_slots(HW, C)
    ref = slab_ref(term, B, HW, R)
    assert representable(ref, ref)
    big = torch.full((R + 2, B, C), SENTINEL, device=cuda)
    big[1:R + 1] = 0
    dz = ops.silu_project_dgrad(gr.to(cuda), z.to(cuda), wtT.to(cuda), big[1:R + 1], 1)
    assert dz.shape == (B * HW, C) and torch.isfinite(dz).all()
    big = big.cpu()
    assert torch.equal(big[1:R + 1].double(), ref)  # every slot, the unused ones (0 in the reference) included
    assert (big[0] == SENTINEL).all() and (big[R + 1] == SENTINEL).all()
    # APoZ of a forward call on the same z, inside guards of its own
    cnt = torch.full((B + 2, C), SENTINEL, device=cuda)
    cnt[1:B + 1] = 0
    out = ops.silu_project_fwd(z.to(cuda), wtT.t().contiguous().to(cuda), torch.ones(Co, device=cuda),
                               torch.zeros(Co, device=cuda), None, cnt[1:B + 1])
    assert torch.isfinite(out).all()
    cnt = cnt.cpu()
    assert torch.equal(cnt[1:B + 1], (z > 0).view(B, HW, C).sum(1).float())
    assert (cnt[0] == SENTINEL).all() and (cnt[B + 1] == SENTINEL).all()


@pytest.mark.parametrize("C", FWD_C)
@pytest.mark.parametrize("B,HW", FWD_GEOMS)
def test_silu_project_fwd_one_hot(cuda, B, HW, C):
    from torchpruner_amd import ops
    z = fwd_case(B, HW, C)
    apoz = torch.zeros(B, C, device=cuda)
    out = ops.silu_project_fwd(z.to(cuda), torch.eye(C, device=cuda), torch.ones(C, device=cuda),
                               torch.zeros(C, device=cuda), None, apoz).cpu()
    assert out.shape == (B * HW, C)
    r = _silu_ratio(out, z)
    print(f"silu_project_fwd one-hot B={B} HW={HW} C={C}: worst SiLU error = {r:.3f} x 2^-24 silu(|z|)")
    assert r <= SILU_ULP
    assert torch.equal(apoz.cpu(), (z > 0).view(B, HW, C).sum(1).float())
