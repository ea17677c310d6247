"""A hand-written fp64 reference of the training BatchNorm launchers of csrc/kernels/batchnorm.hip
(tp_bn_fwd_train, tp_bn_bwd_train and their ``_pre`` forms) and the a-priori error bounds their direct
tests assert (tests/test_bn_train_direct_gpu.py on the kernels, tests/test_bn_reference.py on a NumPy
emulation of the documented algorithm). A plain module: no fixtures, no F.batch_norm (which refuses
P = 1 and hides the intermediates). Everything works on (P, C) tensors of any device and returns fp64.

The checks are split in two:
 (a) statistics: the kernel's fp32 ``mean`` / ``invstd`` (and running statistics) against fp64 from x;
 (b) everything else (y, the mask, dx, dgamma, dbeta, dres) against fp64 evaluated FROM THE KERNEL'S
     OWN fp32 mean / invstd, which the backward launchers take as inputs anyway. The bounds of (b) are
     then a few roundings of the terms actually added, and the conditioning of the statistics (sums of
     x and x^2 in fp32) cannot hide an error of the apply passes.

No bound is fitted to what the kernels give. u = 2^-24 is the unit roundoff of fp32; every fp32
operation returns its exact result times (1 + d), |d| <= u (a contracted fma rounds once instead of
twice: fewer roundings than counted, never more). The fp64 folds (16 row lanes, then the row groups,
then 64 fold lanes: under 1200 additions) contribute 1200 * 2^-53 < u / 2^18 relative to the sum of
magnitudes and are covered by the slack named at each bound.

R is the number of rows one thread adds into its fp32 partial before the fp64 folds: a block walks
rows_per_group = ceil(P / groups) rows with 16 row lanes, so R = ceil(rows_per_group / 16)."""
import torch

U = 2.0 ** -24
U53 = 2.0 ** -53
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the launchers take eps as a float
BN_RL = 16  # row lanes of a statistics block

# (P, C) of the row / column geometry tests. P: 1 (var = 0, the P > 1 guard of the unbiased variance);
# 60, 63, 64, 65 (one group, around the 64-row unrolled step); 127 (one group, unrolled + tail); 130 (two
# groups of 65); 200 (three groups, ragged last); 4481 (70 groups of 65 rows, the last one empty).
# C: 4, 64, 68 float4 rows (68: a second column block of one quad); 13, 67, 70 per-element rows (a partial
# quad, in the second block for 67 and 70); (2112, 2052): 33 column blocks cap the groups at 31.
GEOMETRY = ([(1, c) for c in (4, 13, 68, 67)] + [(60, 64), (60, 70), (63, 4), (63, 67), (64, 68), (64, 13),
            (65, 64), (65, 70), (127, 68), (127, 67)] + [(130, c) for c in (4, 13, 64, 70)] +
            [(p, c) for p in (200, 4481) for c in (4, 64, 68, 13, 67, 70)] + [(2112, 2052)])


# The unit tails (Hardswish, SiLU) run the empty-group shape only; pre-activations within KINK_BAND of a kink of
# the Hardswish (-3, +3) are excluded from its comparisons.
TAIL_SHAPE = (4481, 13)
KINK_BAND = 1e-5


def tail_inputs(P, C):
    """x, gamma, beta, g of the unit tails' case (fp32, CPU): about a sixth of the pre-activations beyond either kink."""
    gen = torch.Generator().manual_seed(29)
    x = torch.randn(P, C, generator=gen) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=gen) * 1.5 + 1.5, torch.rand(C, generator=gen) * 6 - 3
    return x, gamma, beta, torch.randn(P, C, generator=gen)


def bn_groups(P, C, T=None):
    """Row groups of the statistics pass: ``T.bn_groups`` if the extension binds it, else the two-line
    formula of tp::bn_groups (min(1024 / column blocks, P / 64), at least 1)."""
    if T is not None and hasattr(T, "bn_groups"):
        return int(T.bn_groups(P, C))
    col_blocks = (C + 63) // 64
    return min(max(1, min(1024, 1024 // max(1, col_blocks))), max(1, P // 64))


def rows_per_thread(P, C, T=None):
    """R: the fp32 terms one thread adds."""
    rpg = -(-P // bn_groups(P, C, T))
    return -(-rpg // BN_RL)


# ------------------------------------------------------------------------------------------ reference
def stats(x, eps=EPS):
    """(mean, biased var, invstd) over the rows of x (P, C), fp64."""
    x = x.double()
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def running(old_mean, old_var, mean, var, P, momentum):
    """The running statistics after one step, as bn_fwd_finalize: (1 - m) * old + m * stat with the unbiased
    variance for P > 1 and the biased one for P = 1; ``momentum`` as the float the launcher receives."""
    m = float(torch.tensor(momentum, dtype=torch.float32))
    vstat = var * P / (P - 1) if P > 1 else var
    return (1.0 - m) * old_mean.double() + m * mean, (1.0 - m) * old_var.double() + m * vstat, vstat


def act_fn(v, act):
    """0 none, 1 ReLU, 2 ReLU6"""
    return v if act == 0 else v.clamp_min(0) if act == 1 else v.clamp(0, 6)


def act_bit(y, act):
    """bn_act_bit: "the gradient passes", read off the activation's output (strict on both sides)."""
    return (y > 0) if act == 1 else (y > 0) & (y < 6)


def _full(v, C, cr, fill, dev):
    out = torch.full((C,), fill, dtype=torch.float64, device=dev)
    if v is not None:
        out[:cr] = v.double()
    return out


def fwd_from_stats(x, mean, invstd, gamma, beta, res=None, act=0, cr=0):
    """y = act(x * a + b (+ res)) in fp64 from given statistics: a = gamma * invstd, b = beta - mean * a,
    a = b = 0 at channels c >= cr (padding). Returns a, b, bmag = |beta| + |mean * a| (the magnitude of the
    terms of b), v (before the activation, res included) and y."""
    P, C = x.shape
    cr = cr or C
    live = (torch.arange(C, device=x.device) < cr).double()
    a = _full(gamma, C, cr, 1.0, x.device) * invstd.double() * live
    be = _full(beta, C, cr, 0.0, x.device) * live
    ma = mean.double() * a
    b = be - ma
    v = x.double() * a + b
    if res is not None:
        v = v + res.double()
    return {"a": a, "b": b, "bmag": be.abs() + ma.abs(), "v": v, "y": act_fn(v, act)}


def bwd_from_stats(g, x, mean, invstd, gamma, keep=None, cr=0, gm=None):
    """The backward in fp64 from given mean / invstd and a given keep mask (bool (P, C), None: all):
    gm = g * keep, dbeta = sum gm, dgamma = sum gm * xhat, dx = a * gm + k1 + k2 * x with
    k2 = -a * invstd * dgamma / P, k1 = -a * dbeta / P - k2 * mean (= a * (gm - dbeta/P - xhat * dgamma/P)).
    Channels c >= cr: a = k1 = k2 = 0, and dgamma / dbeta have cr entries. ``gm`` (fp64, instead of g and
    keep): the gradient reaching the BN when the activation's derivative is not a mask (the unit tails)."""
    P, C = x.shape
    cr = cr or C
    live = (torch.arange(C, device=x.device) < cr).double()
    gm = (g.double() if gm is None else gm) * live
    if keep is not None:
        gm = gm * keep.double()
    mu, is64 = mean.double(), invstd.double()
    xhat = (x.double() - mu) * is64
    t0, t1 = gm, gm * xhat
    sg, sgx = t0.sum(0), t1.sum(0)
    a = _full(gamma, C, cr, 1.0, x.device) * is64 * live
    k2 = -a * is64 * sgx / P
    k1 = -a * sg / P - k2 * mu
    return {"gm": gm, "xhat": xhat, "dbeta": sg[:cr], "dgamma": sgx[:cr], "abs0": t0.abs().sum(0),
            "abs1": t1.abs().sum(0), "a": a, "k1": k1, "k2": k2, "dx": a * gm + k1 + k2 * x.double()}


def pack_bits(b):
    """bool (P, C) -> uint8[ceil(P*C/4)]: byte i, bit q = flat element 4i + q (low nibble only)."""
    flat = b.reshape(-1).to(torch.uint8)
    if flat.numel() % 4:
        flat = torch.cat([flat, flat.new_zeros(4 - flat.numel() % 4)])
    w = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=b.device)
    return (flat.view(-1, 4) * w).sum(1).to(torch.uint8)


def unpack_bits(by, n=None):
    """uint8 bytes -> bool: all 8 bits of every byte in element order 4i + q for q < 4, then the high nibble
    separately. Returns (bits of the first ``n`` elements, everything else as one bool tensor that must be all
    False: the tail bits of the last byte and every high nibble)."""
    b = by.to(torch.int32)
    low = ((b[:, None] >> torch.arange(4, device=by.device, dtype=torch.int32)) & 1).bool().reshape(-1)
    n = low.numel() if n is None else n
    return low[:n], torch.cat([low[n:], (b >> 4) != 0])


# -------------------------------------------------------------------------------------------- bounds
def e_mean(x, mean, R):
    """|mean_kernel - mean| <= (R + 2) u mean|x| + u |mean|.
    A thread adds R fp32 terms: R - 1 roundings, each relative to a partial sum that the thread's sum of |x|
    bounds, so all threads together are off by (R - 1) u sum|x|; dividing by P: (R - 1) u mean|x|. The
    remaining 3 u mean|x| hold the fp64 folds and the division (< u / 2^18) and the second-order terms
    ((1 + u)^R - 1 - R u < u for R < 4096). The store (float)m rounds once: u |mean|."""
    return (R + 2) * U * x.double().abs().mean(0) + U * mean.abs()


def e_var(x, mean, R):
    """|var_kernel - var| <= (R + 2) u mean(x^2) + 2 |mean| E_mean + E_mean^2.
    var_kernel = q/P - m*m in fp64 from the folded sums. q: every term x*x rounds once (not at all when
    contracted into an fma) and a thread adds R of them: R u sum(x^2), with 2 u for folds and second order
    as in e_mean. m is off by at most E_mean (which counts the store that m does not even have: looser, as
    the form is), so m*m by 2 |mean| E_mean + E_mean^2. The clamp at 0 only moves var_kernel towards var >= 0."""
    em = e_mean(x, mean, R)
    return (R + 2) * U * (x.double() ** 2).mean(0) + 2 * mean.abs() * em + em ** 2


def invstd_interval(var, ev, eps=EPS):
    """invstd_kernel = (float)(1 / sqrt(var_kernel + eps)) with var_kernel in [max(var - E_var, 0), var + E_var]:
    inside [1/sqrt(var + E_var + eps), 1/sqrt(max(var - E_var, 0) + eps)], widened by 2u relative (u: the
    fp32 store; u: the fp64 sqrt and division, 2^-52, and the products by 1 -+ 2u below)."""
    lo = 1.0 / torch.sqrt(var + ev + eps) * (1 - 2 * U)
    hi = 1.0 / torch.sqrt((var - ev).clamp_min(0) + eps) * (1 + 2 * U)
    return lo, hi


def e_running(e_stat, momentum, old, new):
    """|run_kernel - run| <= momentum E + 3u (|old| + |new|), run = (1 - m) * old + m * stat in fp32:
    E is the error of the fp32 stat the kernel blends in (its store rounding included); 1.f - m, its product
    with old, and m * stat round once each: 2u (1 - m)|old| + u m |stat|, and the sum u |new|. Since
    m |stat| <= |new| + (1 - m)|old| that is at most 3u |old| + 2u |new|."""
    return float(momentum) * e_stat + 3 * U * (old.double().abs() + new.abs())


def e_y(x, ref, res=None):
    """|v_kernel - v| <= 4u (|x a| + |b|) + u |res| + u |v|, before the clamp (the activations are
    1-Lipschitz and monotone, so the bound holds after it), with v, a, b of fwd_from_stats at the kernel's
    own mean / invstd and |b| taken as |beta| + |mean a|, the magnitude of the two terms that b adds (b itself
    may cancel, and its rounding errors are relative to these terms).
    a_kernel = fl(gamma * invstd): u |a|; x * a_kernel rounds once more: 2u |x a|. b_kernel = beta -
    fl(fl(mean * gamma) * invstd): 2u |mean a| + u |b| <= 3u (|beta| + |mean a|). The sum x*a + b rounds once,
    u (|x a| + |b|) before the residual; the residual add rounds once, u |v|. Total 3u |x a| + 4u |b| + u |v|;
    the fourth u |x a| and u |res| hold the second-order terms. Exactly 0 where a = b = 0 and res = 0."""
    xa = (x.double() * ref["a"]).abs()
    e = 4 * U * (xa + ref["bmag"]) + U * ref["v"].abs()
    return e if res is None else e + U * res.double().abs()


def e_sum(abs_terms, R, e_terms=None):
    """|dbeta_kernel - dbeta|, |dgamma_kernel - dgamma| <= (R + 3) u sum|term| per channel, terms gm and
    gm * xhat (xhat from the fp32 mean / invstd that both sides read). One term gm * (x - mean) * invstd
    rounds three times (3u |term|; gm itself is exact: g or 0), a thread's R - 1 additions give (R - 1) u
    sum|term|, the fp32 store u |sum| <= u sum|term|: R + 3, folds and second order inside the rounding up
    of R - 1 to R. ``e_terms``: a per-channel sum of errors that the terms themselves carry (the unit tails'
    gm = g * act'(v) is computed, not read)."""
    e = (R + 3) * U * abs_terms
    return e if e_terms is None else e + (1 + (R + 3) * U) * e_terms


def e_dx(x, ref, P, e_sg, e_sgx, e_gm=None):
    """|dx_kernel - dx| <= 6u (|gm a| + |k1| + |k2 x|) + |a| (E_sg + |xhat| E_sgx) / P.
    Second part: dx = a (gm - sg/P - xhat sgx/P), and the kernel's sums are off by E_sg, E_sgx. First part, the
    evaluation dx = fl(fl(gm * a) + k1) + fl(k2 * x) with a, k1, k2 each rounded once to fp32 from fp64:
    2u |gm a| + u |k1| + 2u |k2 x| for coefficients and products, u (|gm a| + |k1|) and u (|gm a| + |k1| +
    |k2 x|) for the two additions: 4u |gm a| + 3u |k1| + 3u |k2 x|, rounded up to 6u for the second order.
    ``e_gm``: the error of a computed gm (unit tails), entering as |a| e_gm."""
    a, k1, k2 = ref["a"], ref["k1"], ref["k2"]
    e = 6 * U * ((ref["gm"] * a).abs() + k1.abs() + (k2 * x.double()).abs())
    e = e + a.abs() * (e_sg + ref["xhat"].abs() * e_sgx) / P
    return e if e_gm is None else e + (1 + 6 * U) * a.abs() * e_gm


def e_fold(pre, G):
    """Sums of G fp64 tile statistics: the kernel's fold (4 lanes, then up to 256 groups, then 64 fold lanes)
    and the reference's own fp64 sum each stay within (G + 2) 2^-53 of the sum of magnitudes."""
    return 2 * (G + 2) * U53 * pre.abs().sum(0)


def check(err, bound, what=""):
    """Asserts err <= bound everywhere (0 <= 0 included, NaN fails); returns the largest err / bound."""
    worst = float(torch.where(bound > 0, err / bound, torch.zeros_like(err)).max()) if err.numel() else 0.0
    ok = err <= bound
    assert bool(ok.all()), f"{what}: max err / bound = {worst:.3f}, {int((~ok).sum())} of {ok.numel()} entries over"
    return worst


def check_stats(x, mean_k, invstd_k, R, cr=0, what=""):
    """Check (a): the kernel's fp32 mean / invstd against fp64 from x. Returns (mean, var, E_mean, E_var)."""
    mean, var, _ = stats(x)
    em, ev = e_mean(x, mean, R), e_var(x, mean, R)
    check((mean_k.double() - mean).abs(), em, what + " mean")
    lo, hi = invstd_interval(var, ev)
    isk = invstd_k.double()
    bad = ~((isk >= lo) & (isk <= hi))
    assert not bool(bad.any()), (f"{what} invstd outside its interval at channels {bad.nonzero().flatten().tolist()[:8]}: "
                                 f"{isk[bad][:4].tolist()} vs [{lo[bad][:4].tolist()}, {hi[bad][:4].tolist()}]")
    return mean, var, em, ev
