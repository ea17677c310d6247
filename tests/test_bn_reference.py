"""(CPU) The fp64 reference and the a-priori bounds of tests/bn_reference.py, checked without the kernels:

- the reference against fp64 autograd through F.batch_norm (P > 1), every activation, with and without a
  residual, with padding channels, and the bit-packing helpers;
- every bound function on a NumPy emulation of the algorithm that batchnorm.hip documents: per-lane fp32 sums
  over the rows r0 + rl, r0 + rl + 16, ... of a row group, fp64 folds, the fp64 finalize with its fp32 stores,
  and the fp32 apply passes with one rounding per operation (no fma: the largest number of roundings a build
  can have). A correct implementation of that algorithm stays inside every bound at every shape and input
  family of tests/test_bn_train_direct_gpu.py, so the bounds cannot fail a correct kernel; the code under test
  has no part in this."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_reference as R

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------- reference vs autograd
def e64(mag, P):
    """Two fp64 evaluations of one formula from the same fp64 inputs (the reference and autograd; no kernel is
    involved): each is a sum of at most P + 16 terms and a dozen further operations, so within (P + 64) 2^-53 of
    the magnitude ``mag`` of the terms added; both together, and the statistics (sums of P terms, relative
    (P + 64) 2^-53, on which every output depends once more) make it 4 (P + 64) 2^-53 mag."""
    return 4 * (P + 64) * R.U53 * mag


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("P,C,cr", [(2, 4, 0), (37, 13, 0), (37, 16, 13), (200, 72, 67)])
def test_reference_matches_autograd(P, C, cr, act, res):
    crr = cr or C
    gen = torch.Generator().manual_seed(P * 1000 + C * 10 + act)
    x = torch.randn(P, C, generator=gen, dtype=torch.float64) * 2 + 0.5
    x[:, crr:] = 0
    gamma = (torch.rand(crr, generator=gen, dtype=torch.float64) * 1.5 + 1.5).requires_grad_(True)
    beta = (torch.rand(crr, generator=gen, dtype=torch.float64) * 4 + 1).requires_grad_(True)
    rs = torch.randn(P, C, generator=gen, dtype=torch.float64) if res else None
    if res:
        rs[:, crr:] = 0
    g = torch.randn(P, C, generator=gen, dtype=torch.float64)
    xr = x[:, :crr].clone().requires_grad_(True)
    rr = rs[:, :crr].clone().requires_grad_(True) if res else None
    rm, rv = torch.zeros(crr, dtype=torch.float64), torch.ones(crr, dtype=torch.float64)
    v = F.batch_norm(xr, rm, rv, gamma, beta, True, 0.1, R.EPS)
    if res:
        v = v + rr
    y = R.act_fn(v, act)
    y.backward(g[:, :crr])

    mean, var, invstd = R.stats(x)
    fw = R.fwd_from_stats(x, mean, invstd, gamma.detach(), beta.detach(), rs, act, cr)
    ymag = (x * fw["a"]).abs() + fw["bmag"] + (rs.abs() if res else 0)
    R.check((fw["y"][:, :crr] - y.detach()).abs(), e64(ymag[:, :crr], P), "y")
    assert not bool(fw["y"][:, crr:].any())
    nrm, nrv, _ = R.running(torch.zeros(C), torch.ones(C), mean, var, P, 0.1)
    m32 = float(torch.tensor(0.1, dtype=torch.float32))
    R.check((nrm[:crr] - rm / 0.1 * m32).abs(), e64(1 + mean[:crr].abs(), P), "running_mean")
    R.check((nrv[:crr] - ((1 - m32) + (rv - 0.9) / 0.1 * m32)).abs(), e64(1 + var[:crr], P), "running_var")
    keep = None
    if act:
        keep = R.act_bit(fw["y"], act)
        assert P == 2 or 0.1 < float(keep[:, :crr].double().mean()) < 0.95
    bw = R.bwd_from_stats(g, x, mean, invstd, gamma.detach(), keep, cr)
    dxmag = (bw["gm"] * bw["a"]).abs() + bw["k1"].abs() + (bw["k2"] * x).abs()
    R.check((bw["dx"][:, :crr] - xr.grad).abs(), e64(dxmag[:, :crr], P), "dx")
    R.check((bw["dgamma"] - gamma.grad).abs(), e64(bw["abs1"][:crr], P), "dgamma")
    R.check((bw["dbeta"] - beta.grad).abs(), e64(bw["abs0"][:crr], P), "dbeta")
    assert not bool(bw["dx"][:, crr:].any()) and bw["dgamma"].shape == (crr,)
    if res:
        assert torch.equal(bw["gm"][:, :crr], rr.grad)


def test_reference_p1():
    """P = 1: var = 0, invstd = 1/sqrt(eps), y = beta, and the running variance takes the biased variance."""
    x = torch.tensor([[3.0, -2.0, 0.0, 5.5]])
    mean, var, invstd = R.stats(x)
    assert torch.equal(mean, x[0].double()) and not bool(var.any())
    assert torch.equal(invstd, torch.full((4,), 1.0 / R.EPS ** 0.5, dtype=torch.float64))
    beta = torch.tensor([1.0, 2.0, 3.0, 4.0])
    assert torch.equal(R.fwd_from_stats(x, mean, invstd, None, beta)["y"][0], beta.double())
    _, nrv, vstat = R.running(torch.zeros(4), torch.ones(4), mean, var, 1, 1.0)
    assert not bool(vstat.any()) and not bool(nrv.any())


@pytest.mark.parametrize("P,C", [(1, 4), (3, 8), (5, 13), (7, 70), (2, 1)])
def test_bits_round_trip(P, C):
    gen = torch.Generator().manual_seed(P * 100 + C)
    b = torch.rand(P, C, generator=gen) < 0.5
    by = R.pack_bits(b)
    assert by.dtype == torch.uint8 and by.numel() == (P * C + 3) // 4
    bits, rest = R.unpack_bits(by, P * C)
    assert torch.equal(bits.view(P, C), b) and not bool(rest.any())
    for e, bit in enumerate(b.reshape(-1).tolist()):  # the layout itself: element e is bit e % 4 of byte e // 4
        assert ((int(by[e // 4]) >> (e % 4)) & 1) == int(bit)
    by2 = by.clone()
    by2[-1] |= 0x80  # a stray high bit is reported, not dropped
    assert bool(R.unpack_bits(by2, P * C)[1].any())


def test_groups_formula():
    """The geometry the cases are chosen for."""
    assert [R.bn_groups(p, 64) for p in (1, 60, 127, 130, 200, 4481)] == [1, 1, 1, 2, 3, 70]
    assert -(-4481 // 70) == 65 and 69 * 65 > 4481  # the last group starts past P: empty
    assert R.bn_groups(2112, 2052) == 31 and 2112 // 64 == 33  # capped by the 33 column blocks
    assert R.rows_per_thread(4481, 64) == 5 and R.rows_per_thread(1, 4) == 1 and R.rows_per_thread(60, 4) == 4
    assert len(R.GEOMETRY) <= 40
    for p in {p for p, _ in R.GEOMETRY if p != 2112}:
        assert sum(1 for q, _ in R.GEOMETRY if q == p) >= 2
    for c in {c for _, c in R.GEOMETRY if c != 2052}:
        assert sum(1 for _, d in R.GEOMETRY if d == c) >= 2


# -------------------------------------------------------------------------- the documented algorithm
def emu_sums(terms, P, C):
    """fp64 column sums of fp32 terms (P, C) in the kernels' order: 16 row lanes per row group, lane rl adds rows
    r0 + rl, r0 + rl + 16, ... < min(P, r0 + rows_per_group) sequentially in fp32; lanes and groups fold in fp64."""
    groups = R.bn_groups(P, C)
    rpg = -(-P // groups)
    r0 = np.arange(groups)[:, None] * rpg
    r1 = np.minimum(P, r0 + rpg)
    acc = np.zeros((groups, R.BN_RL, C), f32)
    for k in range(-(-rpg // R.BN_RL)):
        rows = r0 + np.arange(R.BN_RL)[None, :] + R.BN_RL * k
        valid = rows < r1
        vals = np.where(valid[..., None], terms[np.where(valid, rows, 0)], f32(0))
        acc = (acc + vals).astype(f32)
    return acc.astype(f64).sum((0, 1))


def emu_fwd(x, gamma, beta, res, act, cr, rm, rv, mom):
    P, C = x.shape
    s, q = emu_sums(x, P, C), emu_sums((x * x).astype(f32), P, C)
    m = s / P
    var = np.maximum(q / P - m * m, 0.0)
    is32, m32 = (1.0 / np.sqrt(var + f64(f32(R.EPS)))).astype(f32), m.astype(f32)
    live = np.arange(C) < cr
    ga = np.where(live, gamma, f32(0)).astype(f32)
    a = (ga * is32).astype(f32)
    b = (np.where(live, beta, f32(0)).astype(f32) - ((m32 * ga).astype(f32) * is32).astype(f32)).astype(f32)
    y = ((x * a).astype(f32) + b).astype(f32)
    if res is not None:
        y = (y + res).astype(f32)
    if act:
        y = np.maximum(y, f32(0))
        if act == 2:
            y = np.minimum(y, f32(6))
    mo = f32(mom)
    vst = (var * P / (P - 1) if P > 1 else var).astype(f32)
    nrm = (((f32(1) - mo) * rm).astype(f32) + (mo * m32).astype(f32)).astype(f32)
    nrv = (((f32(1) - mo) * rv).astype(f32) + (mo * vst).astype(f32)).astype(f32)
    return m32, is32, y, nrm, nrv


def emu_bwd(g, x, mean, invstd, gamma, keep, cr):
    P, C = x.shape
    d = np.where(keep, g, f32(0)).astype(f32)
    t1 = ((d * (x - mean).astype(f32)).astype(f32) * invstd).astype(f32)
    sg, sgx = emu_sums(d, P, C), emu_sums(t1, P, C)
    live = np.arange(C) < cr
    is64 = invstd.astype(f64)
    ac = np.where(live, gamma, 0).astype(f64) * is64
    k2 = -ac * is64 * sgx / P
    k1 = -ac * sg / P - k2 * mean.astype(f64)
    a32, k1, k2 = ac.astype(f32), k1.astype(f32), k2.astype(f32)
    dx = (((d * a32).astype(f32) + k1).astype(f32) + (k2 * x).astype(f32)).astype(f32)
    return sgx.astype(f32)[:cr], sg.astype(f32)[:cr], dx


def family(name, P, C, gen):
    if name == "std":
        return torch.randn(P, C, generator=gen) * 3 + 1
    if name == "const":  # channel 0 all zeros, channel 1 all 7.0
        x = torch.randn(P, C, generator=gen) * 3 + 1
        x[:, 0], x[:, 1] = 0.0, 7.0
        return x
    return torch.randn(P, C, generator=gen) + float(name)


OPTION_CASES = [(p, c, cr) for p in (60, 200) for c, cr in ((16, 0), (16, 13), (67, 0), (72, 0), (72, 67))]
EMU_CASES = ([("std", p, c, 0, 1, False) for p, c in R.GEOMETRY] +
             [("std", p, c, cr, act, res) for p, c, cr in OPTION_CASES for act, res in ((0, True), (2, True), (1, False))] +
             [(r, p, 8, 0, 0, False) for r in ("0.3333333333333333", "10", "100") for p in (200, 3136)] +
             [("const", 200, 8, 0, 0, False), ("const", 200, 13, 0, 1, False)] +
             [("std", 2100, c, 0, 1, False) for c in (8, 67)] + [("std", 4481, 13, 0, 0, False)])


@pytest.mark.parametrize("fam,P,C,cr,act,res", EMU_CASES,
                         ids=[f"{f}-{p}x{c}-cr{cr}-act{a}{'-res' if r else ''}" for f, p, c, cr, a, r in EMU_CASES])
def test_documented_algorithm_is_inside_every_bound(fam, P, C, cr, act, res):
    crr = cr or C
    gen = torch.Generator().manual_seed(P * 131 + C * 7 + act)
    x = family(fam, P, C, gen)
    x[:, crr:] = 0
    gamma, beta = torch.rand(crr, generator=gen) * 1.5 + 0.5, torch.randn(crr, generator=gen) * 2
    rs = torch.randn(P, C, generator=gen) if res else None
    if res:
        rs[:, crr:] = 0
    g = torch.randn(P, C, generator=gen)
    g[:, crr:] = 1.0
    rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    pad = lambda t: np.concatenate([t.numpy(), np.zeros(C - crr, f32)])
    mom = 0.1
    m32, is32, y, nrm, nrv = emu_fwd(x.numpy(), pad(gamma), pad(beta), rs.numpy() if res else None, act, crr,
                                     rm0.numpy(), rv0.numpy(), mom)
    m32, is32, y = torch.from_numpy(m32), torch.from_numpy(is32), torch.from_numpy(y)
    Rr = R.rows_per_thread(P, C)
    what = f"{fam} {P}x{C}"
    # (a) statistics
    mean, var, em, ev = R.check_stats(x, m32, is32, Rr, what=what)
    rrm, rrv, vstat = R.running(rm0, rv0, mean, var, P, mom)
    scale = P / (P - 1) if P > 1 else 1.0
    R.check((torch.from_numpy(nrm).double() - rrm).abs(), R.e_running(em, mom, rm0, rrm), what + " running_mean")
    R.check((torch.from_numpy(nrv).double() - rrv).abs(),
            R.e_running(ev * scale + R.U * vstat.abs(), mom, rv0, rrv), what + " running_var")
    # (b) from the emulation's own fp32 mean / invstd
    fw = R.fwd_from_stats(x, m32, is32, gamma, beta, rs, act, cr)
    R.check((y.double() - fw["y"]).abs(), R.e_y(x, fw, rs), what + " y")
    keep = R.act_bit(y, act) if act else torch.ones(P, C, dtype=torch.bool)
    dgamma, dbeta, dx = emu_bwd(g.numpy(), x.numpy(), m32.numpy(), is32.numpy(), pad(gamma), keep.numpy(), crr)
    bw = R.bwd_from_stats(g, x, m32, is32, gamma, keep, cr)
    e0, e1 = R.e_sum(bw["abs0"], Rr), R.e_sum(bw["abs1"], Rr)
    R.check((torch.from_numpy(dbeta).double() - bw["dbeta"]).abs(), e0[:crr], what + " dbeta")
    R.check((torch.from_numpy(dgamma).double() - bw["dgamma"]).abs(), e1[:crr], what + " dgamma")
    R.check((torch.from_numpy(dx).double() - bw["dx"]).abs(), R.e_dx(x, bw, P, e0, e1), what + " dx")
    assert not bool(dx[:, crr:].any()) and not bool(y[:, crr:].any())
    assert torch.isfinite(torch.from_numpy(dx)).all()


def test_a_dropped_row_leaves_the_bounds():
    """The bounds see what the old tolerances (1e-4) could not: the statistics of 4481 rows with the last row
    dropped, or the first one counted twice, are outside the mean bound."""
    P, C = 4481, 64
    x = torch.randn(P, C, generator=torch.Generator().manual_seed(5)) * 3 + 1
    mean, var, _ = R.stats(x)
    em = R.e_mean(x, mean, R.rows_per_thread(P, C))
    dropped = x[:-1].double().sum(0) / P
    twice = (x.double().sum(0) + x[0].double()) / P
    assert float(((dropped - mean).abs() / em).median()) > 1 and float(((twice - mean).abs() / em).median()) > 1
    assert float((dropped - mean).abs().max()) < 1e-2  # ... while 1e-4 of a standard deviation (3) hides most of them


def test_hswish_inputs_stay_clear_of_the_kinks():
    """From the fp64 reference alone: at most 0.5 % of the pre-activations of the unit tails' case lie within twice
    the band of a kink (the kernel's statistics move v by far less than the band), and all three branches are busy."""
    x, gamma, beta, _ = R.tail_inputs(*R.TAIL_SHAPE)
    mean, _, invstd = R.stats(x)
    v = R.fwd_from_stats(x, mean, invstd, gamma, beta)["v"]
    near = ((v + 3).abs() <= 2 * R.KINK_BAND) | ((v - 3).abs() <= 2 * R.KINK_BAND)
    print(f"within 2e-5 of a kink: {int(near.sum())} of {near.numel()}")
    assert float(near.double().mean()) <= 0.005
    assert float((v < -3).double().mean()) > 0.05 and float((v > 3).double().mean()) > 0.05
