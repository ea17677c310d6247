"""``ops.silu_project_fwd`` / ``ops.silu_project_dgrad`` (csrc/kernels/silu_project.hip) against their float64
bodies, and the bindings' rejections. Bound: the body on absolute operands gives the magnitude, times
(K + c) 2^-24 with K the reduction length (C forward, Co for gy, + the rows of an image for the slab) and
c = 33: twice the worst error of the kernel's SiLU and slope measured on an MI355X over z in [-100, 100]
against float64, in units of 2^-24 of silu(|z|) / slope(|z|) (16.4 for the slope at z = 16.6, where
1 - sigmoid cancels; 3.0 for the SiLU). Figures: profiles/numerics/silu_project.txt."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

C_ULP = 33
# HW: 1 and 9 (many images per 64-row tile), 49 (tiles that straddle two images), 150 (an image over four tiles).
# C: one partial K slice, two, four (two column chunks of the dgrad). Co: one, two, four (72, 128) accumulators.
SHAPES = list(itertools.product([(1, 1), (5, 9), (2, 49), (3, 150)], [4, 36, 100], [4, 24, 40]))
SHAPES += [((3, 150), 100, 72), ((70, 1), 36, 128)]
# Tile edges. Co at the forward dispatcher's boundaries (32 | 36, 64 | 68) and a partly filled four-accumulator
# tile (100); C of exactly two and four K slices / one and two dgrad column chunks, and one column past them (132);
# HW a multiple of 64 (the slot formula's other branch, no image shares a tile), 63 and 65 around it, 32 (two images
# fill a tile exactly).
SHAPES += [((2, 49), 36, Co) for Co in (32, 64, 68, 100)] + [((2, 49), C, 24) for C in (64, 128, 132)]
SHAPES += [(shape, 36, 24) for shape in ((2, 64), (2, 128), (3, 63), (3, 65), (2, 32))]
_CASES = {}


def _case(B, HW, C, Co):
    if (B, HW, C, Co) not in _CASES:
        g = torch.Generator().manual_seed(B * 1000 + HW * 7 + C + Co)
        N = B * HW
        _CASES[B, HW, C, Co] = {"z": torch.randn(N, C, generator=g) * 3, "wt": torch.randn(C, Co, generator=g),
                                "scale": torch.rand(Co, generator=g) + 0.5, "shift": torch.randn(Co, generator=g),
                                "res": torch.randn(N, Co, generator=g) * 3, "g": torch.randn(N, Co, generator=g)}
    return _CASES[B, HW, C, Co]


def _ratio(got, ref, mag, K):
    bound = (K + C_ULP) * 2.0 ** -24 * mag
    return float(((got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max())


def _check_fwd(cuda, t, B, with_extras, label):
    from torchpruner_amd import ops
    C = t["z"].shape[1]
    d = {k: v.to(cuda) for k, v in t.items()}
    d64 = {k: v.double() for k, v in t.items()}

    def run(o, f=lambda v: v):
        ap = torch.zeros(B, C, device=o["z"].device, dtype=o["z"].dtype) if with_extras else None
        return ops.silu_project_fwd(f(o["z"]), f(o["wt"]), f(o["scale"]), f(o["shift"]),
                                    f(o["res"]) if with_extras else None, ap), ap
    (out, ap), (out2, ap2), (ref, rap), (mag, _) = run(d), run(d), run(d64), run(d64, torch.abs)
    assert torch.equal(out, out2) and torch.isfinite(out).all()
    if with_extras:
        assert torch.equal(ap, ap2) and torch.equal(ap.double().cpu(), rap)
    r = _ratio(out, ref, mag, C)
    print(f"silu_project_fwd {label} extras={int(with_extras)}: worst error / bound = {r:.4f}")
    assert r <= 1.0


def _check_dgrad(cuda, t, B, HW, mode, label):
    from torchpruner_amd import ops
    C, Co = t["z"].shape[1], t["g"].shape[1]
    wtT = (t["wt"] * t["scale"]).t().contiguous()
    R = ops.silu_project_tay_slots(HW, C)

    def run(g, z, w, dev, dt):
        tay = torch.zeros(R, B, C, device=dev, dtype=dt) if mode is not None else None
        return ops.silu_project_dgrad(g, z, w, tay, mode or 0), tay
    dev = (t["g"].to(cuda), t["z"].to(cuda), wtT.to(cuda), cuda, torch.float32)
    (dz, tay), (dz2, tay2) = run(*dev), run(*dev)
    assert torch.equal(dz, dz2) and torch.isfinite(dz).all()
    ref, rtay = run(t["g"].double(), t["z"].double(), wtT.double(), "cpu", torch.float64)
    mag, mtay = run(t["g"].double().abs(), t["z"].double().abs(), wtT.double().abs(), "cpu", torch.float64)
    r = _ratio(dz, ref, mag, Co)
    rt = 0.0
    if mode is not None:
        assert torch.equal(tay, tay2)
        rt = _ratio(tay.sum(0), rtay.sum(0), mtay.sum(0).abs(), Co + HW)
    print(f"silu_project_dgrad {label} tay_mode={mode}: worst error / bound = dz {r:.4f} tay {rt:.4f}")
    assert r <= 1.0 and rt <= 1.0


@pytest.mark.parametrize("with_extras", [False, True], ids=["plain", "res_apoz"])
@pytest.mark.parametrize("shape,C,Co", SHAPES)
def test_forward_matches_the_fp64_body(cuda, shape, C, Co, with_extras):
    B, HW = shape
    _check_fwd(cuda, _case(B, HW, C, Co), B, with_extras, f"B={B} HW={HW} C={C} Co={Co}")


@pytest.mark.parametrize("mode", [None, 0, 1], ids=["notay", "taylor", "sensitivity"])
@pytest.mark.parametrize("shape,C,Co", SHAPES)
def test_dgrad_matches_the_fp64_body(cuda, shape, C, Co, mode):
    B, HW = shape
    _check_dgrad(cuda, _case(B, HW, C, Co), B, HW, mode, f"B={B} HW={HW} C={C} Co={Co}")


def test_extreme_pre_activations_stay_finite_and_inside_the_bound(cuda):
    """z at +-100 and +-88 (the exponential overflows / underflows), 0, and around +-1.28 (the slope's zero)."""
    B, HW, C, Co = 2, 49, 36, 24
    t = dict(_case(B, HW, C, Co))
    vals = torch.tensor([100.0, -100.0, 0.0, 1.28, -1.28, 1.2785, -1.2785, 88.0, -88.0])
    t["z"] = vals[torch.arange(B * HW * C) % len(vals)].view(B * HW, C).contiguous()
    _check_fwd(cuda, t, B, True, "extreme")
    for mode in (0, 1):
        _check_dgrad(cuda, t, B, HW, mode, "extreme")


def _reject(name, cuda):
    t = {k: v.to(cuda) for k, v in _case(5, 9, 36, 24).items()}
    z, wt, sc, sh, res, g = (t[k] for k in ("z", "wt", "scale", "shift", "res", "g"))
    wtT = wt.t().contiguous()
    tay, mode = torch.zeros(2, 5, 36, device=cuda), 0
    if name == "host_operand":
        wt, wtT = wt.cpu(), wtT.cpu()
    elif name == "C_not_multiple_of_4":
        z, wt, wtT, tay = z[:, :34].contiguous(), wt[:34].contiguous(), wtT[:, :34].contiguous(), None
    elif name == "shapes_do_not_chain":
        wt, wtT = wt[:32].contiguous(), wtT[:, :32].contiguous()
    elif name == "apoz_tay_rows_do_not_divide":
        tay = torch.zeros(2, 4, 36, device=cuda)
    elif name == "bad_tay_mode":
        mode = 2
    elif name == "Co_over_the_limit":
        wt, sc, sh, res = (torch.rand(s, device=cuda) for s in ((36, 132), (132,), (132,), (45, 132)))
    apoz = torch.zeros(tay.shape[1], z.shape[1], device=cuda) if tay is not None else None
    return (z, wt, sc, sh, res, apoz), (g, z, wtT, tay, mode)


@pytest.mark.parametrize("name,ops_hit", [("host_operand", "fd"), ("C_not_multiple_of_4", "fd"),
                                          ("shapes_do_not_chain", "fd"), ("apoz_tay_rows_do_not_divide", "fd"),
                                          ("bad_tay_mode", "d"), ("Co_over_the_limit", "f")])
def test_bindings_reject(cuda, name, ops_hit):
    from torchpruner_amd import ops
    fwd, dgrad = _reject(name, cuda)
    if "f" in ops_hit:
        with pytest.raises(RuntimeError):
            ops.require().silu_project_fwd(*fwd)
    if "d" in ops_hit:
        with pytest.raises(RuntimeError):
            ops.require().silu_project_dgrad(*dgrad)
