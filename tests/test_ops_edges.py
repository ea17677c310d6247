"""The elementwise ops (channel_reduce, prefix_mask, cross_entropy, dropout, gather_multi, score_fold_,
the Shapley scatters, column_accumulate, channel_fill_ / nan_channels, the training pools) at the shapes
where they can go wrong: every kernel variant the launchers choose between (float4 / scalar, chunked,
misaligned operands, tails), one-element and odd sizes, NaN / inf inputs.

Every check is a function of the device: on the CPU it runs the PyTorch fallback of
``torchpruner_amd.ops``, on the GPU (marked ``gpu``) the HIP kernel. The reference is never the op
itself: a few lines of fp64 PyTorch / NumPy here. Tolerances are a-priori rounding bounds of the
number formats (stated at each check), not tuned figures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from torchpruner_amd import ops

U24, U53 = 2.0 ** -24, 2.0 ** -53  # unit roundoffs of fp32 / fp64


@pytest.fixture(params=[pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)])
def dev(request):
    if request.param == "cuda":
        return request.getfixturevalue("cuda")
    return torch.device("cpu")


def _on(t, dev, cl=False, offset=False):
    """``t`` on ``dev`` (channels_last when ``cl``); ``offset``: the same values in a view whose storage
    starts one float into its allocation, so the data pointer is 4-byte aligned only."""
    t = t.to(dev)
    if cl:
        t = t.contiguous(memory_format=torch.channels_last)
    if offset:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        v = buf.as_strided(t.shape, t.stride(), 1)
        v.copy_(t)
        assert v.data_ptr() == buf.data_ptr() + t.element_size() and v.stride() == t.stride()
        t = v
    return t


def _same_bits(a, b):
    """Bit-for-bit equality of two float32 tensors (NaN payloads and the sign of zero included)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------ channel_reduce
# (shape, channels_last): the kernel each one lands on is named in the issue's list
REDUCE_CASES = [((1, 5, 3, 3), False), ((2, 7, 49), False), ((3, 10), False), ((2, 33, 7, 7), False),
                ((2, 33, 7, 7), True),    # scalar NHWC
                ((2, 64, 5, 5), True),    # float4 NHWC, one chunk
                ((1, 32, 40, 40), True),  # float4 NHWC, 64 chunks + nhwc_finish
                ((2, 8, 36, 36), True),   # scalar NHWC, S > 1024: 2 chunks + nhwc_finish
                ((2, 6, 4, 4), False),    # float4 rows, 4 lanes per row
                ((2, 3, 16, 17), False)]  # scalar rows, 64 lanes per row


def _reduce_ref(a, g, mode):
    """fp64 reference and sum_s |term_s| per (b, c)."""
    a, g = a.double().flatten(2) if a.dim() > 2 else a.double().unsqueeze(2), \
        g.double().flatten(2) if g.dim() > 2 else g.double().unsqueeze(2)
    if mode in ("taylor", "taylor_signed"):
        term = -(g * a)
    elif mode == "sensitivity":
        term = g.abs()
    elif mode == "apoz":
        term = (a > 0).double()
    else:
        term = g
    ref = term.sum(2)
    return (ref.abs() if mode == "taylor" else ref), term.abs().sum(2), term.shape[2]


def _check_reduce(dev, shape, cl, special):
    gen = torch.Generator().manual_seed(sum(shape) + 7 * cl)
    a, g = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    if special:  # one NaN and one +inf in the activation, in different (sample, channel) rows
        a.view(-1)[a.numel() // 3] = float("nan")
        a[-1, -1].view(-1)[-1] = float("inf")
    for offset in (False, True):
        ad, gd = _on(a, dev, cl, offset), _on(g, dev, cl, offset)
        for mode in ops.REDUCE_MODES:
            calls = [(ad, gd)]
            if mode == "apoz":
                calls.append((ad, None))      # activation-only
            if mode in ("sensitivity", "sum_grad"):
                calls.append((None, gd))      # gradient-only
            ref, mag, S = _reduce_ref(a, g, mode)
            for act, grad in calls:
                out = ops.channel_reduce(act, grad, mode).cpu()
                what = f"{mode} {shape} cl={cl} offset={offset} act={act is not None} grad={grad is not None}"
                assert out.shape == ref.shape and out.dtype == torch.float32, what
                if mode == "apoz":  # a count: exact (NaN > 0 is false, +inf > 0 is true)
                    assert torch.equal(out, ref.float()), what
                    continue
                # an fp32 sum of S rounded products, in any order: |out - ref| <= (S + 2) u sum|term|
                fin = torch.isfinite(ref)
                assert torch.equal(torch.isnan(out), torch.isnan(ref)), what
                assert torch.equal(out[~fin & ~torch.isnan(ref)].double(), ref[~fin & ~torch.isnan(ref)]), what
                err, bound = (out.double() - ref).abs()[fin], ((S + 2) * U24 * mag)[fin]
                assert bool((err <= bound).all()), f"{what}: max err/bound {(err / bound.clamp_min(1e-300)).max():.3g}"


@pytest.mark.parametrize("shape,cl", REDUCE_CASES)
def test_channel_reduce_edges(dev, shape, cl):
    _check_reduce(dev, shape, cl, special=False)


@pytest.mark.parametrize("shape,cl", REDUCE_CASES)
def test_channel_reduce_nan_inf(dev, shape, cl):
    _check_reduce(dev, shape, cl, special=True)


# --------------------------------------------------------------------------------------------- prefix_mask
MASK_CASES = [((2, 6, 7, 7), False),  # scalar NCHW (S % 4 != 0)
              ((2, 6, 4, 4), False),  # float4 NCHW
              ((2, 6, 4, 4), True),
              ((2, 8, 3, 3), True),   # float4 channels_last (C % 4 == 0)
              ((2, 6, 3, 4), True),   # scalar channels_last (C % 4 != 0)
              ((3, 10), False)]       # the (B, C) MLP case


@pytest.mark.parametrize("shape,cl", MASK_CASES)
def test_prefix_mask_edges(dev, shape, cl):
    """out[k] = z with the channels of rank < p0 + k set to exactly 0.0, everything else copied bit for
    bit; NaN / inf in a masked channel must not survive (a multiply by a 0/1 mask would keep NaN)."""
    B, C = shape[:2]
    gen = torch.Generator().manual_seed(C + len(shape))
    z = torch.randn(shape, generator=gen)
    perm = torch.randperm(C, generator=gen)
    rank = torch.empty(C, dtype=torch.int32)
    rank[perm] = torch.arange(C, dtype=torch.int32)
    first, last = int(perm[0]), int(perm[-1])  # masked from lim = 1 on / only by lim = C
    z[0, first].view(-1)[0] = float("nan")
    z[-1, first].view(-1)[-1] = float("inf")
    z[0, last].view(-1)[-1] = float("-inf")
    for offset in (False, True):
        zd = _on(z, dev, cl, offset)
        for p0, K in ((0, 1), (0, C + 1), (C - 1, 2), (2, 4)):
            out = ops.prefix_mask(zd, rank.to(dev), p0, K)
            ref = z.unsqueeze(0).repeat((K,) + (1,) * z.dim())
            for k in range(K):
                ref[k][:, rank < p0 + k] = 0.0
            ref = ref.reshape((K * B,) + tuple(shape[1:]))
            what = f"{shape} cl={cl} offset={offset} p0={p0} K={K}"
            assert _same_bits(out, ref), what
            if cl and dev.type == "cuda":
                assert out.is_contiguous(memory_format=torch.channels_last), what
        # p0 = 0 copies z unchanged; p0 + k = C zeroes everything
        assert _same_bits(ops.prefix_mask(zd, rank.to(dev), 0, 1), z)
        assert _same_bits(ops.prefix_mask(zd, rank.to(dev), C, 1), torch.zeros_like(z))


# ------------------------------------------------------------------------------------------- cross_entropy
def _ce_ref(x, t, gscale):
    ls = torch.log_softmax(x.double(), 1)
    idx = torch.arange(x.shape[0])
    grad = ls.exp()
    grad[idx, t.long()] -= 1.0
    return -ls[idx, t.long()], grad * gscale


CE_CASES = [(1, 1), (1, 2), (5, 63), (5, 64), (5, 65), (37, 1000)]


@pytest.mark.parametrize("B,NC", CE_CASES)
def test_cross_entropy_edges(dev, B, NC):
    gen = torch.Generator().manual_seed(B * 1000 + NC)
    x = torch.randn(B, NC, generator=gen) * 3
    t = torch.randint(0, NC, (B,), generator=gen)
    for gscale in (1.0, 1 / 37):
        l_ref, g_ref = _ce_ref(x, t, gscale)
        for xd, td in ((x.to(dev), t.to(dev)), (x.to(dev), t.to(dev, torch.int32)),
                       (x.to(dev).t().contiguous().t(), t.to(dev))):  # int32 target, non-contiguous logits
            l, g = ops.cross_entropy(xd, td, gscale, True)
            torch.testing.assert_close(l.double().cpu(), l_ref, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(g.double().cpu(), g_ref, rtol=1e-5, atol=1e-6)
            l2, g2 = ops.cross_entropy(xd, td, gscale, False)
            assert g2 is None and _same_bits(l2, l)


def test_cross_entropy_nan_rows(dev):
    """One NaN in a row: NaN loss and NaN gradient row, the other rows untouched. A row of all -inf:
    NaN, as ATen gives."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(5, 65, generator=gen) * 3
    t = torch.randint(0, 65, (5,), generator=gen)
    l_ref, g_ref = _ce_ref(x, t, 1.0)
    x[1, 64] = float("nan")
    x[3] = float("-inf")
    l, g = (v.cpu() for v in ops.cross_entropy(x.to(dev), t.to(dev), 1.0, True))
    bad = torch.tensor([False, True, False, True, False])
    assert torch.equal(torch.isnan(l), bad)
    assert torch.equal(torch.isnan(g), bad.unsqueeze(1).expand(5, 65))
    torch.testing.assert_close(l[~bad].double(), l_ref[~bad], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(g[~bad].double(), g_ref[~bad], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("B,NC", [(5, 65), (37, 1000)])
def test_cross_entropy_large_logits(dev, B, NC):
    """Logits of randn * 30 (|x - max| up to ~200). The kernel's ``__expf`` / ``__logf`` may err at most
    8x ATen's own fp32 cross-entropy against the same fp64 reference (and never has to beat the tolerance
    of the small-magnitude cases): the argument scaling of ``__expf`` costs about |x - m| * 2^-24 relative
    error, which ATen's ``expf`` does not pay.

    Measured on an MI355X (profiles/numerics/ops_edges.txt), maxima over both cases: loss error kernel
    6.966e-06 vs ATen 1.467e-05; gradient error kernel 1.458e-07 vs ATen 1.458e-07."""
    gen = torch.Generator().manual_seed(B + NC)
    x = torch.randn(B, NC, generator=gen) * 30
    t = torch.randint(0, NC, (B,), generator=gen)
    l_ref, g_ref = _ce_ref(x, t, 1.0)
    l, g = (v.double().cpu() for v in ops.cross_entropy(x.to(dev), t.to(dev), 1.0, True))
    xa = x.to(dev).requires_grad_(True)
    la = F.cross_entropy(xa, t.to(dev), reduction="none")
    la.sum().backward()
    la, ga = la.detach().double().cpu(), xa.grad.double().cpu()
    e_l, e_g = (l - l_ref).abs(), (g - g_ref).abs()
    a_l, a_g = float((la - l_ref).abs().max()), float((ga - g_ref).abs().max())
    print(f"cross_entropy randn*30 ({B}, {NC}) on {dev.type}: max loss error kernel {float(e_l.max()):.3e} "
          f"ATen {a_l:.3e}; max gradient error kernel {float(e_g.max()):.3e} ATen {a_g:.3e}")
    assert bool((e_l <= torch.clamp(1e-5 + 1e-5 * l_ref.abs(), min=8 * a_l)).all())
    assert bool((e_g <= torch.clamp(1e-6 + 1e-5 * g_ref.abs(), min=8 * a_g)).all())


def test_cross_entropy_target_out_of_range(dev):
    """A target outside [0, NC) (``ignore_index = -100`` data, or a corrupt label) reads nothing: NaN loss
    and an all-NaN gradient row there, every other row bit for bit what valid targets give. (Rows 20 and
    5 are chosen so that row * NC + target stays inside the logits whatever the kernel does.)"""
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(37, 10, generator=gen) * 3
    t = torch.randint(0, 10, (37,), generator=gen)
    tb = t.clone()
    tb[20], tb[5] = -100, 13
    l, g = (v.cpu() for v in ops.cross_entropy(x.to(dev), t.to(dev), 1 / 37, True))
    lb, gb = (v.cpu() for v in ops.cross_entropy(x.to(dev), tb.to(dev), 1 / 37, True))
    bad = torch.zeros(37, dtype=torch.bool)
    bad[[5, 20]] = True
    assert torch.equal(torch.isnan(lb), bad)
    assert torch.equal(torch.isnan(gb), bad.unsqueeze(1).expand(37, 10))
    assert _same_bits(lb[~bad], l[~bad]) and _same_bits(gb[~bad], g[~bad])
    l_ref, g_ref = _ce_ref(x, t, 1 / 37)
    torch.testing.assert_close(lb[~bad].double(), l_ref[~bad], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gb[~bad].double(), g_ref[~bad], rtol=1e-5, atol=1e-6)
    lo = ops.cross_entropy(x.to(dev), tb.to(dev), 1.0, False)[0].cpu()
    assert torch.equal(torch.isnan(lo), bad)


# ------------------------------------------------------------------------------------------------- dropout
def _philox4x32_10(ctr, key):
    """Philox4x32-10 in NumPy uint64 arithmetic on counters (ctr_lo, ctr_hi, 0, 0) with a 64-bit key:
    (n,) uint64 counters -> (n, 4) uint32 words."""
    m32 = np.uint64(0xFFFFFFFF)
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0, c1 = ctr & m32, ctr >> np.uint64(32)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


# the generator's first two counters under key 0 (the host validation program asserts the same words)
PHILOX_CTR0 = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
PHILOX_CTR1 = [0xF8E4CCA4, 0x5CB200DB, 0xB1A574EB, 0x097EFF67]


def test_philox_reference_vectors():
    """The NumPy reference itself: the vectors of the kernel's counter form, high counter word included."""
    w = _philox4x32_10([0, 1], 0)
    assert w[0].tolist() == PHILOX_CTR0 and w[1].tolist() == PHILOX_CTR1
    assert _philox4x32_10([2 ** 32 + 5], 0x0123456789ABCDEF)[0].tolist() == [0xB8B243F7, 0xDA8FB9A8, 0x46004299,
                                                                            0xE54C389C]


def _dropout_ref(x, seed, p):
    """x: float32 NumPy vector. Element e uses word e & 3 of counter e >> 2; kept iff word >= floor(p 2^32)."""
    n = x.size
    words = _philox4x32_10(np.arange((n + 3) // 4, dtype=np.uint64), seed).reshape(-1)[:n]
    keep = words >= np.uint32(min(int(p * 2.0 ** 32), 0xFFFFFFFF))
    return x * np.where(keep, np.float32(1.0 / (1.0 - p)), np.float32(0.0)).astype(np.float32), keep


def _bits_np(y, ref):
    """Bit-for-bit equal, except that a NaN only has to be a NaN."""
    y = y.detach().cpu().numpy().reshape(-1)
    nan = np.isnan(ref)
    return y.shape == ref.shape and np.array_equal(np.isnan(y), nan) and \
        np.array_equal(y.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


@pytest.mark.gpu
def test_dropout_known_words(cuda):
    """Counters 0 and 1 under seed 0 through the op: a threshold between every two neighbouring words of
    the table splits the eight elements exactly as the table says (word order, counter order)."""
    T = ops.require()
    words = PHILOX_CTR0 + PHILOX_CTR1
    srt = sorted(words)
    x = torch.ones(8, device=cuda)
    for lo, hi in zip(srt[:-1], srt[1:]):
        th = (lo + hi) // 2 + 1  # lo < th <= hi
        p = th / 2.0 ** 32       # exact in fp64: floor(p * 2^32) == th
        kept = (T.dropout(x, 0, p) != 0).cpu().tolist()
        assert kept == [w >= th for w in words], hex(th)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1026, 1027])
def test_dropout_bits(cuda, n):
    """Body (float4) and tail kernels against the NumPy generator, bit for bit."""
    T = ops.require()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    xn = x.numpy()
    for seed in (0, 2 ** 62 - 1, 0x0123456789ABCDEF):
        for p in (0.0, 0.3, 0.5, 1 - 2.0 ** -20):
            ref, _ = _dropout_ref(xn, seed, p)
            y = T.dropout(x.to(cuda), seed, p)
            assert _bits_np(y, ref), f"n={n} seed={seed:#x} p={p}"
            if p == 0.0:
                assert _same_bits(y, x)


@pytest.mark.gpu
def test_dropout_past_one_grid_sweep(cuda):
    """8192 * 256 float4 per sweep of the body kernel, plus a tail: the grid-stride loop's second step."""
    T = ops.require()
    n = 8192 * 256 * 4 + 1027
    x = torch.randn(n, generator=torch.Generator().manual_seed(1))
    ref, keep = _dropout_ref(x.numpy(), 12345, 0.3)
    assert abs(keep.mean() - 0.7) < 1e-3
    assert _bits_np(T.dropout(x.to(cuda), 12345, 0.3), ref)


@pytest.mark.gpu
def test_dropout_backward_nan_and_misaligned_view(cuda):
    from torchpruner_amd.engine.train import _NativeDropout, native_convs
    T = ops.require()
    gen = torch.Generator().manual_seed(2)
    seed, p = 2 ** 40 + 17, 0.3
    # the backward regenerates the forward's mask on another tensor
    x = torch.randn(1027, generator=gen).to(cuda).requires_grad_(True)
    g = torch.randn(1027, generator=gen)
    y = _NativeDropout.apply(x, p, seed)
    y.backward(g.to(cuda))
    ref_y, keep = _dropout_ref(x.detach().cpu().numpy(), seed, p)
    ref_g, keep_g = _dropout_ref(g.numpy(), seed, p)
    assert _bits_np(y, ref_y) and _bits_np(x.grad, ref_g) and np.array_equal(keep, keep_g)
    # NaN stays NaN in a dropped position (x * 0, not a select)
    xn = torch.full((64,), float("nan"))
    ref_n, keep_n = _dropout_ref(xn.numpy(), 7, 0.5)
    assert not keep_n.all() and torch.isnan(T.dropout(xn.to(cuda), 7, 0.5)).all() and np.isnan(ref_n).all()
    # a contiguous view that is only 4-byte aligned: nn.Dropout on it gives what the kernel gives on an
    # aligned copy (the mask depends on the element index only)
    full = torch.randn(5, 513, generator=gen).to(cuda)
    view = full[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    drop = torch.nn.Dropout(p).train()
    with native_convs(drop):
        assert "forward" in drop.__dict__
        torch.manual_seed(5)
        yv = drop(view)
    torch.manual_seed(5)
    seed5 = int(torch.randint(0, 2 ** 62, (1,)).item())
    aligned = view.clone()
    assert aligned.data_ptr() % 16 == 0
    assert _same_bits(yv, T.dropout(aligned, seed5, p))
    assert _bits_np(yv, _dropout_ref(view.cpu().numpy().reshape(-1), seed5, p)[0])


# -------------------------------------------------------------------------------------------- gather_multi
def test_gather_multi_edges(dev):
    gen = torch.Generator().manual_seed(4)
    # eleven float32 tensors in one call (a launch takes eight: the second flush), every sliced axis of
    # extent 5, axes 0 / 1 / -1 / the last one (inner == 1)
    f32 = [(torch.randn(5, 3, generator=gen), 0), (torch.randn(2, 5, generator=gen), 1),
           (torch.randn(5, generator=gen), 0), (torch.randn(2, 3, 5, generator=gen), -1),
           (torch.randn(4, 5, 2, 2, generator=gen), 1), (torch.randn(3, 5, generator=gen), -1),
           (torch.randn(5, 1, generator=gen), 0), (torch.randn(1, 5, generator=gen), 1),
           (torch.randn(2, 2, 5, generator=gen), 2), (torch.randn(5, 7, generator=gen), -2),
           (torch.randn(6, 5, generator=gen).t(), 0)]  # (5, 6) transposed: non-contiguous
    others = [(torch.randint(0, 256, (5, 3), generator=gen, dtype=torch.uint8), 0),
              (torch.randint(0, 2, (3, 5), generator=gen).bool(), 1),
              (torch.randint(-2 ** 40, 2 ** 40, (2, 5, 2), generator=gen), 1),
              (torch.randn(5, 2, generator=gen).double(), 0),
              (torch.randn(3, 5, generator=gen).half(), -1),
              (torch.randn(5, 4, generator=gen).double().t(), 1)]
    assert not f32[-1][0].is_contiguous() and not others[-1][0].is_contiguous()
    ts, axes = [t for t, _ in f32 + others], [a for _, a in f32 + others]
    for keep in ([3, 1, 1, 0], [4, 3, 2, 1, 0], [2], []):  # duplicates, descending, one, none
        kt = torch.tensor(keep, dtype=torch.long)
        for keep_dev in (dev, torch.device("cpu")):
            outs = ops.gather_multi([t.to(dev) for t in ts], axes, kt.to(keep_dev))
            assert len(outs) == len(ts)
            for t, ax, o in zip(ts, axes, outs):
                ref = torch.from_numpy(np.take(t.numpy(), np.asarray(keep, dtype=np.int64), axis=ax))
                assert o.dtype == t.dtype and torch.equal(o.cpu(), ref), (tuple(t.shape), ax, keep)
                assert torch.equal(ref, t.index_select(ax, kt))


# --------------------------------------------------------------------------------------------- score_fold_
@pytest.mark.parametrize("after", [0, 1, 2])
@pytest.mark.parametrize("take_abs", [False, True])
def test_score_fold_edges(dev, after, take_abs):
    """(B, C) with one thread, with two column chunks of 256 + 1 scalars (513), with five float4 column
    chunks (1056) and rows past one row chunk (65), a float4 slab of 65 quads (260); 2-D, one slot, three
    slots; accumulators that start non-zero, and none. The slab bit for bit; the accumulator within the
    fp64 summation bound B * 2^-53 * sum|v| (the start value 0.5 and fp32 addends keep the final add
    exact to that bound)."""
    gen = torch.Generator().manual_seed(after * 2 + take_abs)
    shapes = [(1, 1), (3, 33, 513), (1, 65, 1056), (3, 260), (33, 513), (3, 3, 260), (1, 1, 1), (65, 1056)]
    has_acc = [True, True, True, True, False, False, True, True]
    Ts = [torch.randn(s, generator=gen) for s in shapes]
    Td = [t.clone().to(dev) for t in Ts]
    accs = [torch.full((s[-1],), 0.5, dtype=torch.float64, device=dev) if h else None for s, h in zip(shapes, has_acc)]
    ops.score_fold_(Td, accs, take_abs, after)
    for T0, Tn, a in zip(Ts, Td, accs):
        slots = T0 if T0.dim() == 3 else T0.unsqueeze(0)
        v = slots[0].clone()
        for r in range(1, slots.shape[0]):  # fp32, in slot order
            v = v + slots[r]
        if take_abs:
            v = v.abs()
        exp = slots.clone()
        if after == 1:
            exp.zero_()
            exp[0] = v
        elif after == 2:
            exp.zero_()
        assert _same_bits(Tn, exp.reshape(T0.shape)), (tuple(T0.shape), after, take_abs)
        if a is not None:
            ref = 0.5 + v.double().sum(0)
            bound = v.shape[0] * U53 * v.double().abs().sum(0)
            assert bool(((a.cpu() - ref).abs() <= bound).all()), tuple(T0.shape)


# ------------------------------------------------------------------------------------------------- shapley
@pytest.mark.parametrize("K,B", [(1, 1), (3, 130), (7, 40)])
def test_shapley_scatter_column_edges(dev, K, B):
    """K * B > 256 (more than one block of the scatter), B > 64 (the column loop's second step), row0 > 0,
    k0 > 0, k0 + K == n, accumulators that start non-zero."""
    gen = torch.Generator().manual_seed(K * 100 + B)
    k0, row0 = 2, 3
    n = k0 + K
    L = torch.randn(K + 1, B, generator=gen)
    perm = torch.randperm(n, generator=gen).int()
    delta = L[1:].double() - L[:-1].double()  # exact in fp64
    cols = perm[k0:k0 + K].long()
    # per-sample form: one product and one add in fp64 (two roundings, one if contracted to an FMA)
    sv0 = torch.randn(row0 + B + 2, n, generator=gen, dtype=torch.float64)
    sv = sv0.clone().to(dev)
    ops.shapley_scatter(L.to(dev), perm.to(dev), sv, row0, k0, 0.2)
    ref = sv0.clone()
    ref[row0:row0 + B, cols] += (delta * 0.2).t()
    touched = torch.zeros_like(sv0, dtype=torch.bool)
    touched[row0:row0 + B, cols] = True
    sv = sv.cpu()
    assert torch.equal(sv[~touched], sv0[~touched])
    bound = 2 * U53 * (ref.abs() + sv0.abs())
    assert bool(((sv - ref).abs() <= bound)[touched].all())
    # column form: the fp64 sum over b is bounded by B * 2^-53 * sum|delta|; the power-of-two scale and the
    # half-integer start values add no rounding of their own at these magnitudes
    col0 = torch.randint(-4, 5, (n,), generator=gen).double() * 0.5
    col = col0.clone().to(dev)
    ops.shapley_column(L.to(dev), perm.to(dev), col, k0, 0.25)
    ref = col0.clone()
    ref[cols] += delta.sum(1) * 0.25
    bound = torch.zeros(n, dtype=torch.float64)
    bound[cols] = B * U53 * delta.abs().sum(1) * 0.25
    assert bool(((col.cpu() - ref).abs() <= bound).all())


# --------------------------------------------------------------------------------------- column_accumulate
@pytest.mark.parametrize("B,C", [(1, 1), (3, 65), (1000, 300)])
def test_column_accumulate_edges(dev, B, C):
    """fp64 column sums of fp32 values (x * x is exact in fp64): B * 2^-53 * sum|term| per column."""
    v = torch.randn(B, C, generator=torch.Generator().manual_seed(B + C))
    v64 = v.double()
    for with_sq in (False, True):
        s = torch.full((C,), 0.5, dtype=torch.float64, device=dev)
        q = torch.full((C,), 0.25, dtype=torch.float64, device=dev) if with_sq else None
        ops.column_accumulate(v.to(dev), s, q)
        assert bool(((s.cpu() - (0.5 + v64.sum(0))).abs() <= (B + 1) * U53 * (0.5 + v64.abs().sum(0))).all())
        if with_sq:
            sq = (v64 * v64).sum(0)
            assert bool(((q.cpu() - (0.25 + sq)).abs() <= (B + 1) * U53 * (0.25 + sq)).all())


# ---------------------------------------------------------------------------- channel_fill_ / nan_channels
@pytest.mark.parametrize("shape", [(3, 5), (2, 5, 4), (2, 5, 3, 3)])
def test_fill_and_nan_channels_edges(dev, shape):
    gen = torch.Generator().manual_seed(len(shape))
    x0 = torch.randn(shape, generator=gen)
    x = x0.clone().to(dev)
    assert ops.channel_fill_(x, [], 7.5) is x and _same_bits(x, x0)  # an empty idx
    ops.channel_fill_(x, [1, 1, 3], 7.5)                             # duplicates
    ref = x0.clone()
    ref[:, 1], ref[:, 3] = 7.5, 7.5
    assert _same_bits(x, ref)
    assert ops.nan_channels(x).cpu().tolist() == [False] * 5
    # +inf and -inf (in one channel) are not NaN; one NaN in the last element of the last sample flags
    # exactly its channel
    ops.channel_fill_(x, [0], float("inf"))
    x[0, 0].view(-1)[0] = float("-inf")
    ops.channel_fill_(x, torch.tensor([4]), float("-inf"))
    assert ops.nan_channels(x).cpu().tolist() == [False] * 5
    x[-1, 2].view(-1)[-1] = float("nan")
    flags = ops.nan_channels(x)
    assert flags.dtype == torch.bool and flags.cpu().tolist() == [False, False, True, False, False]
    if len(shape) == 4:
        xcl = x.contiguous(memory_format=torch.channels_last)
        assert ops.nan_channels(xcl).cpu().tolist() == [False, False, True, False, False]
    ops.channel_fill_(x, [2], float("nan"))
    ops.channel_fill_(x, [2, 0, 4], 0.0)
    assert ops.nan_channels(x).cpu().tolist() == [False] * 5 and bool((x[:, [0, 2, 4]] == 0).all())


# ------------------------------------------------------------------------------------------ training pools
@pytest.mark.gpu
@pytest.mark.parametrize("k,s,p", [(1, 1, 0), (2, 3, 0), (1, 2, 0), (3, 3, 1)])
def test_native_maxpool_edges(cuda, k, s, p):
    """Max-pool forward and gather backward against fp64 ATen on the CPU: a 1x1 window, strides past the
    window (pixels in no window get a gradient of exactly 0), a window that is all -inf."""
    from torchpruner_amd.engine.train import native_convs
    gen = torch.Generator().manual_seed(k * 10 + s)
    x = torch.randn(2, 4, 7, 6, generator=gen)
    x[1, 2, 0:4, 0:4] = float("-inf")  # covers whole windows of every geometry here
    mp = torch.nn.MaxPool2d(k, s, p)
    xd = x.to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with native_convs(mp):
        assert "forward" in mp.__dict__
        y = mp(xd)
    x64 = x.double().requires_grad_(True)
    y64 = F.max_pool2d(x64, k, s, p)
    assert torch.isinf(y64).any() and torch.equal(y.detach().cpu().double(), y64.detach())
    g = torch.randn(y64.shape, generator=gen)
    y.backward(g.to(cuda))
    y64.backward(g.double())
    assert torch.equal(xd.grad.cpu().double(), x64.grad)
    covered = torch.zeros(7, 6, dtype=torch.bool)
    for oh in range(y64.shape[2]):
        for ow in range(y64.shape[3]):
            covered[max(0, oh * s - p):oh * s - p + k, max(0, ow * s - p):ow * s - p + k] = True
    assert (k, s) not in ((2, 3), (1, 2)) or not covered.all()
    assert bool((xd.grad.cpu()[:, :, ~covered] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 4, 1, 1), (2, 8, 3, 5)])
def test_native_global_avgpool_edges(cuda, shape):
    """fp32 sum of HW terms and one division: (HW + 2) * 2^-24 * mean|x|; the backward is g * fl(1 / HW):
    two roundings."""
    from torchpruner_amd.engine.train import native_convs
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen)
    HW = shape[2] * shape[3]
    gap = torch.nn.AdaptiveAvgPool2d(1)
    xd = x.to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with native_convs(gap):
        assert "forward" in gap.__dict__
        y = gap(xd)
    assert y.shape == shape[:2] + (1, 1)
    ref = x.double().mean((2, 3), keepdim=True)
    bound = (HW + 2) * U24 * x.double().abs().mean((2, 3), keepdim=True)
    assert bool(((y.detach().cpu().double() - ref).abs() <= bound).all())
    g = torch.randn(y.shape, generator=gen)
    y.backward(g.to(cuda))
    gref = (g.double() / HW).expand(shape)
    assert bool(((xd.grad.cpu().double() - gref).abs() <= 3 * U24 * gref.abs()).all())
