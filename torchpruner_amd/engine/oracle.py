"""fp64 oracles of the fused VGG engine's Taylor / Sensitivity scores.

A deep ReLU network is discontinuous in its inputs: a pre-activation within rounding of 0, or two
max-pool candidates within rounding of each other, makes the fp32 forward take a different ReLU
mask / pool argmax than the fp64 one, and every score upstream of that unit then differs by far
more than fp32 rounding. Comparing an fp32 kernel against a plain fp64 run therefore measures the
kernel's rounding *and* the conditioning of the input. This module separates the two:

``engine_scores_fp64(engine, x, y, conditioned=True)`` replays the fused engine's own discrete
decisions (every ReLU mask, every 2x2 max-pool argmax, read back from the engine's forward) in
an fp64 forward + input-gradient backward. The fused scores must match it to fp32 rounding of
the arithmetic alone, whatever the input. ``conditioned=False`` is the plain fp64 run (its own
masks and argmaxes), which the reference's semantics define (taylor.py:31-49,
attributions.py:58-68); ``decision_flips`` counts where the two runs' decisions differ.

Runs on the CPU in fp64 on one batch (the per-batch mean loss of the reference,
attributions.py:66): the caller loops batches and reduces.

``mobilenet_scores_fp64`` is the same idea for the MobileNet engine, with ReLU6's three-way
decision (<= 0 / in between / >= 6) replayed through an autograd pass of a float64 copy of the model.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _nchw(t, c):
    """Engine NHWC (padded width) -> NCHW fp64 CPU with the real ``c`` channels."""
    return t.permute(0, 3, 1, 2)[:, :c].double().cpu().contiguous()  # NCHW-contiguous: same conv algorithms


def _affine(blk):
    """Eval-mode BN folded into a per-channel (scale, shift) with the conv bias, in fp64."""
    conv, bn = blk.conv, blk.bn
    c = conv.out_channels
    bias = conv.bias.detach().double().cpu() if conv.bias is not None else torch.zeros(c, dtype=torch.float64)
    if bn is None:
        return torch.ones(c, dtype=torch.float64), bias
    inv = torch.rsqrt(bn.running_var.detach().double().cpu() + bn.eps)
    g = bn.weight.detach().double().cpu() if bn.weight is not None else torch.ones(c, dtype=torch.float64)
    b = bn.bias.detach().double().cpu() if bn.bias is not None else torch.zeros(c, dtype=torch.float64)
    scale = g * inv
    return scale, (bias - bn.running_mean.detach().double().cpu()) * scale + b


def _windows(pre):
    """(B, C, H, W) -> (B, C, H/2, W/2, 4) with q = 2*dy + dx (the engine's argmax byte)."""
    B, C, H, W = pre.shape
    return pre.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def _unpool(gp, q, H, W):
    B, C = gp.shape[:2]
    full = torch.zeros(B, C, H // 2, W // 2, 4, dtype=gp.dtype)
    full.scatter_(-1, q.unsqueeze(-1), gp.unsqueeze(-1))
    return full.view(B, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)


FLIP_RATE_BOUND = 1e-5  # rounding-tie decision flips per decision against fp64 (tests, smoke)


def flip_bound(decisions: int, rate: float = FLIP_RATE_BOUND) -> float:
    """Largest flip count a correct fp32 kernel may show on a block of ``decisions`` units: the
    expected rounding ties ``rate * n`` (an fp32 F(4x4) conv has ~1e-5 relative error, so about
    that fraction of pre-activations sits within rounding of 0) plus a Poisson allowance
    (4 standard deviations + 2), so a 25k-unit block may show its one or two ties while a
    systematic mis-decision — hundreds of flips per 100k units — cannot hide."""
    mu = rate * decisions
    return mu + 4.0 * mu ** 0.5 + 2.0


def flip_violations(flips: dict, totals: dict, rate: float = FLIP_RATE_BOUND) -> dict:
    """Blocks whose engine-vs-fp64 decision flips exceed :func:`flip_bound`: {block: (flips,
    decisions)}. A kernel that systematically mis-decides values near 0 (sign of zero, denormal
    flush, ``>=`` for ``>``) passes the mask-conditioned score check — it compares arithmetic
    given the engine's own decisions — but not this bound."""
    return {b: (flips[b], totals[b]) for b in flips if flips[b] > flip_bound(totals[b], rate)}


@torch.no_grad()
def engine_scores_fp64(engine, x, y, conditioned=True, mode="taylor", totals=None):
    """Per-sample scores {block: (B, C_real) fp64} of one batch: ``mode="taylor"`` the signed
    sum_hw -(dL/da * a), ``"sensitivity"`` sum_hw |dL/da| (a = the block activation's output),
    with L the batch-mean cross-entropy. Returns (scores, flips): ``flips[block]`` counts the
    units whose ReLU mask or pool argmax differs between the engine and fp64 given the same
    upstream decisions (both are computed; ``conditioned`` picks which decisions the returned
    scores use and feed downstream). ``totals`` (a dict, optional) receives each block's number
    of decisions (units of its activation), the denominator of :func:`flip_violations`."""
    plan = engine.plan
    saved = engine.forward(x)[1]
    acts_f = saved["acts"]
    lin_f = saved["lin_acts"]
    h = x.double().cpu()
    B = h.shape[0]
    flips = {}
    convs = []  # per conv block: (act (pooled) NCHW, q or None, mask at act's resolution, scale, H, W)
    for i, blk in enumerate(plan.convs):
        c = blk.conv.out_channels
        scale, shift = _affine(blk)
        pre = F.conv2d(h, blk.conv.weight.detach().double().cpu(), None, padding=1)
        pre = pre * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        H, W = pre.shape[2:]
        hf = _nchw(acts_f[i][0], c)
        if blk.pool is not None:
            win = _windows(pre)
            q_own = win.argmax(-1)
            v_own = win.gather(-1, q_own.unsqueeze(-1)).squeeze(-1)
            m_own = v_own > 0
            q_f = acts_f[i][1].permute(0, 3, 1, 2)[:, :c].long().cpu().contiguous()
            m_f = hf > 0
            flips[i] = int(((m_f != m_own) | ((q_f != q_own) & (m_f | m_own))).sum())
            if totals is not None:
                totals[i] = int(m_f.numel())
            q, m = (q_f, m_f) if conditioned else (q_own, m_own)
            act = torch.where(m, win.gather(-1, q.unsqueeze(-1)).squeeze(-1), torch.zeros((), dtype=pre.dtype))
        else:
            m_own = pre > 0
            m_f = hf > 0
            flips[i] = int((m_f != m_own).sum())
            if totals is not None:
                totals[i] = int(m_f.numel())
            q, m = None, (m_f if conditioned else m_own)
            act = torch.where(m, pre, torch.zeros((), dtype=pre.dtype))
        convs.append((act, q, m, scale, H, W))
        h = act
    nconv = len(plan.convs)
    lin_in = [h.reshape(B, -1) if nconv else x.double().cpu().reshape(B, -1)]
    lmask = {}  # linear index -> ReLU mask (no entry: no activation, identity in the backward)
    for j, lb in enumerate(plan.linears):
        w = lb.linear.weight.detach().double().cpu()
        b = lb.linear.bias.detach().double().cpu() if lb.linear.bias is not None else 0.0
        z = lin_in[-1] @ w.t() + b
        if lb.relu is not None:
            n = lb.linear.out_features
            m_f = lin_f[j + 1].reshape(B, -1)[:, :n].cpu() > 0
            m_own = z > 0
            flips[nconv + j] = int((m_f != m_own).sum())
            if totals is not None:
                totals[nconv + j] = int(m_f.numel())
            m = m_f if conditioned else m_own
            z = torch.where(m, z, z * lb.slope)
            lmask[j] = m
        lin_in.append(z)
    logits = lin_in[-1]
    g = (torch.softmax(logits, 1) - F.one_hot(y.cpu(), logits.shape[1]).double()) / B

    def score(ga, a):
        return (ga.abs() if mode == "sensitivity" else -(ga * a)).reshape(B, a.shape[1], -1).sum(-1)

    scores = {}
    nlin = len(plan.linears)
    g_out = None
    for j in range(nlin - 1, -1, -1):
        ga = g @ plan.linears[j].linear.weight.detach().double().cpu()
        if j > 0:
            scores[nconv + j - 1] = score(ga, lin_in[j])
            m = lmask.get(j - 1)
            g = ga if m is None else torch.where(m, ga, ga * plan.linears[j - 1].slope)
        elif nconv:
            act = convs[-1][0]
            g_out = ga.view(act.shape)
    for ci in range(nconv - 1, -1, -1):
        act, q, m, scale, H, W = convs[ci]
        scores[ci] = score(g_out, act)
        if ci == 0:
            break
        gm = torch.where(m, g_out, torch.zeros((), dtype=g_out.dtype))
        g_full = _unpool(gm, q, H, W) if q is not None else gm
        g_pre = g_full * scale.view(1, -1, 1, 1)
        prev = convs[ci - 1][0]
        g_out = torch.nn.grad.conv2d_input(prev.shape, plan.convs[ci].conv.weight.detach().double().cpu(), g_pre,
                                           padding=1)
    return scores, flips


def mobilenet_scores_fp64(engine, model, x, y, mode="taylor", conditioned=True, criterion=None):
    """fp64 oracle of the MobileNet engine's scores on one batch: a CPU autograd pass of a float64
    copy of ``model`` (every ReLU6 out of place), scored at the ReLU6 modules the engine serves
    (``MobileNetEngine.eval_modules``: post-expand and post-depthwise of every block).

    ``conditioned=True`` replays the engine's own three-way decision of EVERY ReLU6 of the net
    (<= 0 / in between / >= 6, read from the pre-activations and clamped outputs its fp32 forward
    saved) in the fp64 pass: the output is the fp64 pre-activation where the engine passed it, else
    the constant 0 or 6, and the gradient flows exactly where the engine let it. The engine's
    scores must then match to fp32 rounding of the arithmetic alone. ``conditioned=False`` is the
    plain fp64 run (``engine`` may be None: nothing is replayed or counted).

    Returns (scores, flips, totals): ``scores[module]`` (keyed by the modules of ``model``) is the
    (B, C) fp64 per-sample score as ``ops.channel_reduce`` defines ``mode`` ("taylor",
    "taylor_signed", "sensitivity") for the batch-mean loss (cross-entropy, or ``criterion``);
    ``flips[name]`` / ``totals[name]`` count, per ReLU6, the units whose decision differs between
    the engine and fp64 given the same upstream decisions, and the units, for
    :func:`flip_violations`."""
    import copy

    import torch.nn as nn
    assert engine is not None or not conditioned, "replaying decisions needs the engine"
    m64 = copy.deepcopy(model).double().cpu().eval()
    names = {id(m): n for n, m in m64.named_modules()}
    relus = [m for m in m64.modules() if isinstance(m, nn.ReLU6)]
    for m in relus:
        m.inplace = False
    orig = [m for m in model.modules() if isinstance(m, nn.ReLU6)]
    decided = {}  # ReLU6 of the copy -> engine tensor holding its decision (NHWC, padded width)
    if engine is not None:
        with torch.no_grad():
            saved = engine.forward(x, save=True)[1]
        zh, _ = saved[-1]
        eng_mods = {id(o): c for o, c in zip(orig, relus)}
        plan = engine.plan
        decided[eng_mods[id(plan.stem.act)]] = saved[0][0]  # pre-activation, or the clamped output: same regions
        decided[eng_mods[id(plan.head.act)]] = zh
        for blk, (_, z, yd, _) in zip(plan.blocks, saved[:-1]):
            if blk.expand is not None:
                decided[eng_mods[id(blk.expand.act)]] = z
            decided[eng_mods[id(blk.dw.act)]] = yd
    flips, totals, outs = {}, {}, {}

    def hook(mod, inp, out):
        z = inp[0]
        t = decided.get(mod)
        if t is not None:
            tf = _nchw(t, z.shape[1])
            lo_f, hi_f = tf <= 0, tf >= 6
            flips[names[id(mod)]] = int(((lo_f != (z <= 0)) | (hi_f != (z >= 6))).sum())
            totals[names[id(mod)]] = z.numel()
            if conditioned:
                const = torch.where(hi_f, torch.full((), 6.0, dtype=z.dtype), torch.zeros((), dtype=z.dtype))
                out = torch.where(lo_f | hi_f, const, z)
        outs[mod] = out
        if out.requires_grad:
            out.retain_grad()
        return out

    handles = [m.register_forward_hook(hook) for m in relus]
    try:
        with torch.enable_grad():
            xin = x.detach().double().cpu().requires_grad_(True)  # keeps every activation in the graph
            logits = m64(xin)
            loss = F.cross_entropy(logits, y.cpu()) if criterion is None else criterion(logits, y.cpu())
            loss.backward()
    finally:
        for h in handles:
            h.remove()
    if engine is not None:
        served = [eng_mods[id(m)] for m in engine.eval_modules()], engine.eval_modules()
    else:
        from .mobilenet_engine import build_mobilenet_plan
        plan, why = build_mobilenet_plan(model)
        assert plan is not None, why
        p64 = build_mobilenet_plan(m64)[0]
        pick = lambda p: [a for b in p.blocks for a in (([b.expand.act] if b.expand is not None else []) + [b.dw.act])]
        served = pick(p64), pick(plan)
    scores = {}
    for c, o in zip(*served):
        a, g = outs[c].detach(), outs[c].grad
        v = g.abs() if mode == "sensitivity" else -(g * a)
        v = v.flatten(2).sum(-1)
        scores[o] = v.abs() if mode == "taylor" else v
    return scores, flips, totals


def mobilenet_v3_scores_fp64(engine, model, x, y, mode="taylor", conditioned=True, criterion=None):
    """fp64 oracle of the MobileNetV3 engine's scores on one batch, as :func:`mobilenet_scores_fp64`:
    a CPU autograd pass of a float64 copy of ``model`` (every activation out of place), scored at
    the modules the engine serves (``MobileNetV3Engine.eval_modules``).

    ``conditioned=True`` replays the engine's own branch decision of EVERY piecewise activation of
    the net, read from the tensors its fp32 forward saved: a ReLU's ``<= 0`` or live (the gates'
    inner ReLU included), a Hardswish's ``< -3``, middle or ``> 3`` (stem, blocks, head, classifier)
    and a Hardsigmoid gate's ``<= 0``, middle or ``>= 1``. The fp64 pass evaluates the formula of
    the engine's branch at its own fp64 pre-activation (0, v (v + 3) / 6 or v; 0, v / 6 + 0.5 or
    1): the activations are continuous, so the value moves by rounding only while autograd
    differentiates the engine's branch. ``conditioned=False`` is the plain fp64 run (``engine`` may
    be None).

    Returns (scores, flips, totals) as :func:`mobilenet_scores_fp64` does, for
    :func:`flip_violations`."""
    import copy

    import torch.nn as nn
    from .mobilenet_engine import build_mobilenet_v3_plan
    assert engine is not None or not conditioned, "replaying decisions needs the engine"
    m64 = copy.deepcopy(model).double().cpu().eval()
    names = {id(m): n for n, m in m64.named_modules()}
    twin = {id(o): c for o, c in zip(model.modules(), m64.modules())}
    kinds = (nn.ReLU, nn.Hardswish, nn.Hardsigmoid)
    acts = [m for m in m64.modules() if type(m) in kinds]
    for m in acts:
        m.inplace = False
    decided = {}  # activation of the copy -> engine tensor holding its decision
    if engine is not None:
        with torch.no_grad():
            saved = engine.forward(x, save=True)[1]
        zh, z1, z0 = saved[-1]
        plan = engine.plan
        decided[twin[id(plan.stem.act)]] = z0
        decided[twin[id(plan.head.act)]] = zh
        decided[twin[id(list(model.classifier.children())[1])]] = z1
        for blk, (_, z, yd, _, pre, gate) in zip(plan.blocks, saved[:-1]):
            if blk.expand is not None:
                decided[twin[id(blk.expand.act)]] = z
            decided[twin[id(blk.dw.act)]] = pre if pre is not None else yd  # a ReLU's output has its regions
            if gate is not None:
                decided[twin[id(blk.gate.activation)]] = gate[0]
                if type(blk.gate.scale_activation) is nn.Hardsigmoid:
                    decided[twin[id(blk.gate.scale_activation)]] = gate[1]
    flips, totals, outs = {}, {}, {}
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)

    def hook(mod, inp, out):
        z = inp[0]
        t = decided.get(mod)
        if t is not None:
            c = z.shape[1]
            tf = _nchw(t, c) if t.dim() == 4 else t[:, :c].double().cpu().reshape(z.shape)
            if type(mod) is nn.ReLU:
                lo_f, hi_f, lo, hi = tf <= 0, None, z <= 0, None
                branch = z
            elif type(mod) is nn.Hardswish:
                lo_f, hi_f, lo, hi = tf < -3, tf > 3, z < -3, z > 3
                branch = torch.where(hi_f, z, z * (z + 3.0) / 6.0)
            else:  # Hardsigmoid: the engine keeps its output s
                lo_f, hi_f, lo, hi = tf <= 0, tf >= 1, z <= -3, z >= 3
                branch = torch.where(hi_f, one, z / 6.0 + 0.5)
            diff = lo_f != lo
            if hi_f is not None:
                diff = diff | (hi_f != hi)
            flips[names[id(mod)]] = int(diff.sum())
            totals[names[id(mod)]] = z.numel()
            if conditioned:
                out = torch.where(lo_f, zero, branch)
        outs[mod] = out
        if out.requires_grad:
            out.retain_grad()
        return out

    handles = [m.register_forward_hook(hook) for m in acts]
    try:
        with torch.enable_grad():
            xin = x.detach().double().cpu().requires_grad_(True)  # keeps every activation in the graph
            logits = m64(xin)
            loss = F.cross_entropy(logits, y.cpu()) if criterion is None else criterion(logits, y.cpu())
            loss.backward()
    finally:
        for h in handles:
            h.remove()
    if engine is not None:
        served = engine.eval_modules()
    else:
        plan, why = build_mobilenet_v3_plan(model)
        assert plan is not None, why
        served = [a for b in plan.blocks for a in (([b.expand.act] if b.expand is not None else []) + [b.dw.act])]
    scores = {}
    for o in served:
        a, g = outs[twin[id(o)]].detach(), outs[twin[id(o)]].grad
        v = g.abs() if mode == "sensitivity" else -(g * a)
        v = v.flatten(2).sum(-1)
        scores[o] = v.abs() if mode == "taylor" else v
    return scores, flips, totals
