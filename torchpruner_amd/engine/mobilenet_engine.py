"""Attribution engine for MobileNetV2-style nets (torchvision layout: conv3x3-BN-ReLU6 stem,
inverted-residual blocks, conv1x1-BN-ReLU6 head, global average pool, classifier) on the HIP kernels.

The hidden (expanded) activation of a block is the largest tensor of the net; on the generic path an
eval-mode block passes over it eleven times in the forward alone (conv write, BN, ReLU6, depthwise,
BN, ReLU6, each read + write). Here:

  stem     NCHW -> NHWC pad to 4 channels, 3x3 implicit GEMM (``tpamd.conv_gen``) with the eval BN
           folded into the epilogue affine; the PRE-activation z is stored (``relu=False``)
  expand   1x1 ``conv_gen``, BN folded, ``relu=False``: stores z. Its APoZ epilogue counts z > 0,
           which is the ReLU6 output's positive count
  dw       ``tpamd.dwconv_act_fwd``: clamps z to [0, 6] as it loads it, BN folded, ReLU6 on the way
           out, APoZ counts of the output (csrc/kernels/dwconv_act.hip)
  project  1x1 ``conv_gen``, BN folded, linear (its true form), the shortcut as ``res=``
  head     1x1 ``conv_gen`` storing z, then clamp + global average pool + classifier GEMM (two
           elementwise passes over the smallest activation)

ReLU6 never touches the GEMM kernels. The backward runs block by block, last block first: the
project dgrad (``conv_gen_bwd``, BN scale folded into the operand, no mask), the post-depthwise
score as a channel reduction of (y, g), ``tpamd.dwconv_act_dgrad`` (masks g by the stored y, gathers,
reduces the post-expand ReLU6's Taylor / Sensitivity partials from the unmasked gradient, masks by
z), and the expand dgrad with the block's output gradient as ``res=`` when there is a shortcut.

Shapley prefixes are evaluated from inside a block (``forward_to`` / ``prefix_logits`` /
``logits_from``): the K stacked outputs of the linear project conv are a running rank-1 subtraction
per pixel (``ops.prefix_project``, csrc/kernels/prefix_project.hip), and the rest of the network runs
once on them.

Channels are carried zero-padded to a multiple of 32 (``cpad``) as in the ResNet engine, whose conv
plumbing (packing, tuner, classifier GEMMs, partial-slab arena) this engine inherits. One batch at a
time: no two-stream pipeline, no graph replay. fp32 throughout.

MobileNetV3 nets (``build_mobilenet_v3_plan`` / ``MobileNetV3Engine``, second half of this file) run
the same way with ReLU / Hardswish units (``tpamd.dwconv_hs_*``), the squeeze-and-excitation gate
between the depthwise output and the project conv, and a two-layer classifier; Shapley is not
served there.
"""
from __future__ import annotations

import os
import weakref
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .fused_chain import cpad, logits_grad
from .resnet_engine import ResNetEngine, _Conv

_RELU6, _TAY_MODES = 2, {"taylor": 0, "taylor_signed": 0, "sensitivity": 1}


@dataclass
class _Unit:
    """conv -> BN -> ReLU6"""
    conv: nn.Conv2d
    bn: nn.BatchNorm2d
    act: nn.Module


@dataclass
class _IRBlock:
    expand: Optional[_Unit]
    dw: _Unit
    project: _Conv
    shortcut: bool


@dataclass
class MobileNetPlan:
    stem: _Unit
    head: _Unit
    fc: nn.Linear
    blocks: list = field(default_factory=list)


def _conv_kind(conv) -> str:
    """"dense", "depthwise", or the reason the engine cannot run the conv; read from the weight's
    shape (pruning leaves ``in_channels`` / ``out_channels`` stale)."""
    if not isinstance(conv, nn.Conv2d):
        return f"expected a Conv2d, found {type(conv).__name__}"
    if conv.dilation not in (1, (1, 1)):
        return f"dilation {tuple(conv.dilation)} is not supported"
    if conv.padding_mode != "zeros" or isinstance(conv.padding, str):
        return "only explicit zero padding is supported"
    k = conv.weight.shape[2:]
    if k[0] != k[1] or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]:
        return "only square kernels, strides and paddings are supported"
    if conv.groups == 1:
        return "dense"
    cout, cin_g = conv.weight.shape[:2]
    if cin_g != 1:
        return f"grouped conv (groups {conv.groups}, {cin_g} inputs per group) is not supported"
    if cout != conv.groups:
        return f"depth multiplier {cout / conv.groups:g} is not supported (only 1)"
    return "depthwise"


def _unit(seq, what):
    """(_Unit, "") of a conv-BN-ReLU6 Sequential, else (None, reason)."""
    if not isinstance(seq, nn.Sequential) or len(seq) != 3:
        return None, f"{what}: expected a (conv, BN, ReLU6) Sequential"
    conv, bn, act = seq
    kind = _conv_kind(conv)
    if kind not in ("dense", "depthwise"):
        return None, f"{what}: {kind}"
    if not isinstance(bn, nn.BatchNorm2d) or bn.running_mean is None:
        return None, f"{what}: expected a BatchNorm2d with running statistics after the conv"
    if not isinstance(act, nn.ReLU6):
        return None, f"{what}: activation {type(act).__name__} is not supported (only ReLU6)"
    return _Unit(conv, bn, act), ""


def _is_1x1(conv) -> bool:
    return tuple(conv.weight.shape[2:]) == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)


def build_mobilenet_plan(model: nn.Module):
    """Lower a torchvision-layout MobileNetV2, or return (None, reason)."""
    feats, cls = getattr(model, "features", None), getattr(model, "classifier", None)
    if not isinstance(feats, nn.Sequential) or len(feats) < 3 or cls is None or \
            not any(isinstance(getattr(m, "conv", None), nn.Sequential) for m in feats):
        return None, "not a torchvision-layout MobileNetV2 (features / inverted-residual blocks / classifier)"
    pool = getattr(model, "avgpool", None)
    if pool is not None and not (isinstance(pool, nn.AdaptiveAvgPool2d) and pool.output_size in (1, (1, 1))):
        return None, "unsupported pool before the classifier (needs a global AdaptiveAvgPool2d)"
    layers = list(cls.children()) if isinstance(cls, nn.Sequential) else [cls]
    if not layers or not isinstance(layers[-1], nn.Linear) or not all(isinstance(m, nn.Dropout) for m in layers[:-1]):
        return None, "unsupported classifier (needs Dropout layers and a final Linear)"
    stem, why = _unit(feats[0], "stem")
    if stem is None:
        return None, why
    if _conv_kind(stem.conv) != "dense" or stem.conv.weight.shape[2] != 3 or stem.conv.weight.shape[1] > 4 or \
            stem.conv.padding[0] != 1:
        return None, "unsupported stem (needs a 3x3 conv, padding 1, of at most 4 input channels)"
    head, why = _unit(feats[-1], "head")
    if head is None:
        return None, why
    if _conv_kind(head.conv) != "dense" or not _is_1x1(head.conv):
        return None, "unsupported head (needs a 1x1 conv)"
    plan = MobileNetPlan(stem, head, layers[-1])
    width = stem.conv.weight.shape[0]
    for i, blk in enumerate(feats[1:-1], 1):
        seq = getattr(blk, "conv", None)
        what = f"features.{i}"
        if not isinstance(seq, nn.Sequential) or len(seq) not in (3, 4):
            return None, f"{what}: expected an inverted-residual block ([1x1-BN-ReLU6,] depthwise-BN-ReLU6, 1x1, BN)"
        expand = None
        if len(seq) == 4:
            expand, why = _unit(seq[0], f"{what} expand")
            if expand is None:
                return None, why
            if _conv_kind(expand.conv) != "dense" or not _is_1x1(expand.conv):
                return None, f"{what}: the expand conv must be a dense 1x1 conv"
        dw, why = _unit(seq[-3], f"{what} depthwise")
        if dw is None:
            return None, why
        k, s, pd = dw.conv.weight.shape[2], dw.conv.stride[0], dw.conv.padding[0]
        if _conv_kind(dw.conv) != "depthwise" or k not in (3, 5) or s not in (1, 2) or pd > k - 1:
            return None, f"{what}: the depthwise conv must be 3x3 / 5x5, stride 1 / 2, padding < k, depth multiplier 1"
        proj, bn = seq[-2], seq[-1]
        kind = _conv_kind(proj)
        if kind != "dense" or not _is_1x1(proj):
            return None, f"{what}: the project conv must be a dense 1x1 conv" + ("" if kind == "dense" else f" ({kind})")
        if not isinstance(bn, nn.BatchNorm2d) or bn.running_mean is None:
            return None, f"{what}: expected a BatchNorm2d with running statistics after the project conv"
        hidden = dw.conv.weight.shape[0]
        if (expand.conv.weight.shape[:2] if expand else (hidden, width)) != (hidden, width) or \
                proj.weight.shape[1] != hidden:
            return None, f"{what}: channel counts of the block's convs do not chain"
        cout = proj.weight.shape[0]
        shortcut = getattr(blk, "use_res_connect", None)
        if shortcut is None:
            shortcut = s == 1 and cout == width
        if shortcut and (s != 1 or cout != width):
            return None, f"{what}: a shortcut needs stride 1 and equal widths"
        plan.blocks.append(_IRBlock(expand, dw, _Conv(proj, bn), bool(shortcut)))
        width = cout
    if head.conv.weight.shape[1] != width or plan.fc.weight.shape[1] != head.conv.weight.shape[0]:
        return None, "channel counts of the head / classifier do not chain"
    return plan, ""


def _out_hw(conv, H, W):
    k, s, pd = conv.weight.shape[2], conv.stride[0], conv.padding[0]
    return (H + 2 * pd - k) // s + 1, (W + 2 * pd - k) // s + 1


class MobileNetEngine(ResNetEngine):
    pipelined = False  # attributions/base.py: one batch at a time (no _BatchPipeline)

    def __init__(self, model: nn.Module, plan: MobileNetPlan):
        super().__init__(model, plan)

    # ------------------------------------------------------------------ structure
    def _all_convs(self):
        p = self.plan
        out = [p.stem]
        for b in p.blocks:
            out += ([b.expand] if b.expand is not None else []) + [b.dw, b.project]
        return out + [p.head]

    def eval_modules(self):
        """The ReLU6 modules the engine scores: per block the post-expand one (where the block
        expands) and the post-depthwise one."""
        mods = []
        for b in self.plan.blocks:
            mods += ([b.expand.act] if b.expand is not None else []) + [b.dw.act]
        return mods

    def real_width(self, module) -> int:
        """Channels of an evaluation module's output (the engine's slabs are padded past it)."""
        for b in self.plan.blocks:
            if module is b.dw.act or (b.expand is not None and module is b.expand.act):
                return b.dw.conv.weight.shape[0]
        raise KeyError("not a block ReLU6 of this MobileNet")

    def _stem_fused(self) -> bool:
        """The first block's depthwise conv reads the stem's pre-activation and clamps it itself
        (no expand conv and no shortcut need the activated stem output)."""
        b0 = self.plan.blocks[0]
        return b0.expand is None and not b0.shortcut

    def max_batch(self, sample_shape) -> int:
        H, W = tuple(sample_shape)[-2:]
        per = 4 * H * W * 4  # the channel-padded NHWC input
        H, W = _out_hw(self.plan.stem.conv, H, W)
        per = max(per, 4 * H * W * cpad(self.plan.stem.conv.weight.shape[0]))
        for b in self.plan.blocks:
            hid = cpad(b.dw.conv.weight.shape[0])
            # the hidden activation, and the partial slab of its gradient kernel beside it
            per = max(per, 4 * H * W * hid, 4 * ops.dwconv_act_tay_slots(H, W, hid) * hid)
            H, W = _out_hw(b.dw.conv, H, W)
            per = max(per, 4 * H * W * hid, 4 * H * W * cpad(b.project.conv.weight.shape[0]))
        per = max(per, 4 * H * W * cpad(self.plan.head.conv.weight.shape[0]))
        return max(1, ((1 << 31) - 1) // per)

    # ------------------------------------------------------------------ packing
    @torch.no_grad()
    def _pack_dw(self, u: _Unit):
        from .resnet_engine import _fold
        w = u.conv.weight.detach().float()
        c = w.shape[0]
        cp = cpad(c)
        scale, shift = _fold(u.conv, u.bn)
        # padded channels: zero weights and a zero affine -> exact zeros in y, dz and the scores
        return {"w": F.pad(w, (0, 0, 0, 0, 0, 0, 0, cp - c)).contiguous(), "scale": F.pad(scale, (0, cp - c)),
                "shift": F.pad(shift, (0, cp - c)), "stride": u.conv.stride[0], "pad": u.conv.padding[0]}

    def _pack(self):
        key = self._params_key()
        if key == self._key:
            return self._packed
        p = self.plan
        blocks = []
        for b in p.blocks:
            blocks.append({"expand": self._pack_conv(b.expand) if b.expand is not None else None,
                           "dw": self._pack_dw(b.dw), "project": self._pack_conv(b.project)})
        fc_w = p.fc.weight.detach().float()
        fc_w = F.pad(fc_w, (0, cpad(fc_w.shape[1]) - fc_w.shape[1]))
        fc_b = p.fc.bias.detach().float() if p.fc.bias is not None else torch.zeros(fc_w.shape[0], device=fc_w.device)
        n_cls = fc_w.shape[0]
        fc_wt = F.pad(fc_w, (0, 0, 0, cpad(n_cls) - n_cls)).t().contiguous()
        self._packed = {"stem": self._pack_conv(p.stem, stem=True), "blocks": blocks, "head": self._pack_conv(p.head),
                        "fc_w": fc_w.contiguous(), "fc_b": fc_b.contiguous(), "fc_wt": fc_wt}
        self._key = key
        return self._packed

    # ------------------------------------------------------------------ forward
    def _block(self, T, blk, e, h, in_act, apoz=None, saved=None):
        """One inverted-residual block from its (linear, or for a fused stem pre-activation) input
        ``h``; appends (input, z, y, input activation code) to ``saved``."""
        apoz = apoz or {}
        if blk.expand is not None:
            z = self._conv(T, e["expand"], h, False, apoz=apoz.get(blk.expand.act))
            in_act = _RELU6
        else:
            z = h
        d = e["dw"]
        y = T.dwconv_act_fwd(z, d["w"], d["scale"], d["shift"], d["stride"], d["pad"], in_act, _RELU6,
                             apoz.get(blk.dw.act))
        out = self._conv(T, e["project"], y, False, res=h if blk.shortcut else None)
        if saved is not None:
            saved.append((h, z, y, in_act))
        return out

    def forward(self, x: torch.Tensor, apoz: Optional[dict] = None, save: bool = False):
        """Logits of the network; ``apoz`` maps evaluation modules (:meth:`eval_modules`) to zeroed
        (B, C) float tensors that receive the per-sample counts of positive outputs.
        ``save=True`` returns (logits, saved) for :meth:`grad_scores`."""
        T = ops.require()
        P = self._pack()
        apoz = dict(apoz or {})
        padded = []  # (user buffer, padded scratch) for channel counts that are not multiples of 32
        for m, buf in apoz.items():
            if buf.shape[1] % 32:
                tmp = buf.new_zeros(buf.shape[0], cpad(buf.shape[1]))
                padded.append((buf, tmp))
                apoz[m] = tmp
        h = T.nchw_to_nhwc_pad(x.float().contiguous(), 4)
        h = self._conv(T, P["stem"], h, False)  # the stem's pre-activation
        in_act = _RELU6
        if not self._stem_fused():
            h, in_act = h.clamp_(0.0, 6.0), 0
        saved = []
        for blk, e in zip(self.plan.blocks, P["blocks"]):
            h = self._block(T, blk, e, h, in_act, apoz, saved if save else None)
            in_act = 0
        zh = self._conv(T, P["head"], h, False)
        feat = T.avgpool_nhwc(zh.clamp(0.0, 6.0))
        for buf, tmp in padded:
            buf.add_(tmp[:, :buf.shape[1]])
        logits = self._fc(T, P, feat)
        if save:
            saved.append((zh, feat))
            return logits, saved
        return logits

    # ------------------------------------------------------------------ backward (Taylor, Sensitivity)
    def grad_scores(self, x: torch.Tensor, y: torch.Tensor, want, mode: str, criterion=None,
                    loss_batch: Optional[int] = None, raw_slabs: bool = False):
        """One engine forward + input-gradient-only backward of the loss; returns
        {ReLU6 module: (B, C_padded) per-sample ``ops.channel_reduce`` score} for the modules of
        :meth:`eval_modules` in ``want``. No weight gradients, no autograd graph; the backward stops
        at the earliest block holding a wanted module. ``raw_slabs``: a score that came from the
        depthwise gradient kernel's epilogue stays its raw (R, B, C_padded) partial-slot slab for
        ``ops.score_fold_`` to finish (slot sum, and |.| for "taylor")."""
        T = ops.require()
        P = self._pack()
        logits, saved = self.forward(x, save=True)
        zh, feat = saved.pop()
        B = logits.shape[0]
        blocks = self.plan.blocks
        first = min((bi for bi, b in enumerate(blocks)
                     if b.dw.act in want or (b.expand is not None and b.expand.act in want)), default=None)
        out = {}
        if first is None:
            return out
        g_log = logits_grad(logits, y, criterion, loss_batch)
        g_feat = self._fc_bwd(T, P, g_log, feat)  # (B, C_head padded)
        HW = zh.shape[1] * zh.shape[2]
        # avg-pool backward + the head's ReLU6 (zero gradient at exactly 0 and 6)
        g = torch.where((zh > 0) & (zh < 6), (g_feat / HW)[:, None, None, :], torch.zeros((), device=x.device))
        g, _ = self._dgrad(T, P["head"], g.contiguous(), None)  # dL/d(last block's output)
        akey = (tuple(x.shape), mode, tuple(sorted(i for i, m in enumerate(self.eval_modules()) if m in want)))
        size = self._arena_sizes.get(akey)
        arena = [torch.zeros(size, device=x.device) if size else None, 0, 0]
        for bi in range(len(blocks) - 1, first - 1, -1):
            blk, e = blocks[bi], P["blocks"][bi]
            h, z, yd, in_act = saved[bi]
            gy, _ = self._dgrad(T, e["project"], g, None)  # dL/d(depthwise ReLU6 output), unmasked
            if blk.dw.act in want:
                out[blk.dw.act] = ops.channel_reduce(yd.permute(0, 3, 1, 2), gy.permute(0, 3, 1, 2), mode)
            ex_wanted = blk.expand is not None and blk.expand.act in want
            if bi == first and not ex_wanted:
                break
            d = e["dw"]
            _, H, W, C = z.shape
            tay = self._slab(arena, T.dwconv_act_tay_slots(H, W, C), B, C, x.device) if ex_wanted else None
            dz = T.dwconv_act_dgrad(gy, yd, d["w"], d["scale"], z, H, W, d["stride"], d["pad"], in_act, _RELU6, tay,
                                    _TAY_MODES[mode])
            if ex_wanted:
                if raw_slabs:
                    out[blk.expand.act] = tay
                else:
                    sums = tay.sum(0)
                    out[blk.expand.act] = sums.abs_() if mode == "taylor" else sums
            if bi == first:
                break
            if blk.expand is not None:  # the block input is linear: no mask
                g, _ = self._dgrad(T, e["expand"], dz, None, res=g if blk.shortcut else None)
            else:
                g = dz + g if blk.shortcut else dz
        if arena[2] > (size or 0):
            self._arena_sizes[akey] = arena[2]
        return out

    # ------------------------------------------------------------------ partial forward (Shapley)
    # Prefix copies of a block's hidden activation are never built. Copy j of the post-depthwise
    # output y is y with the masked channels set to a per-channel constant ``fill``: 0 when y's own
    # channels are masked, and clamp(shift, 0, 6) when the post-expand ReLU6's are (a zeroed input
    # channel leaves the depthwise conv 0 at every pixel, zero padding included, so BN + ReLU6 give
    # that constant). The project conv is linear, so its K outputs are one conv of the base copy and
    # a running rank-1 subtraction per pixel (``ops.prefix_project``); the shortcut sits in the base.
    def locate(self, module):
        """(block index, "expand" | "dw") of an evaluation module (:meth:`eval_modules`)."""
        for bi, b in enumerate(self.plan.blocks):
            if module is b.dw.act:
                return bi, "dw"
            if b.expand is not None and module is b.expand.act:
                return bi, "expand"
        raise KeyError("not a block ReLU6 of this MobileNet")

    def forward_to(self, x: torch.Tensor, bi: int):
        """(block ``bi``'s input h, its post-depthwise ReLU6 output y), both in engine layout: the
        state :meth:`prefix_logits` continues from."""
        T = ops.require()
        P = self._pack()
        h = T.nchw_to_nhwc_pad(x.float().contiguous(), 4)
        h = self._conv(T, P["stem"], h, False)
        in_act = _RELU6
        if not self._stem_fused():
            h, in_act = h.clamp_(0.0, 6.0), 0
        for b in range(bi):
            h = self._block(T, self.plan.blocks[b], P["blocks"][b], h, in_act)
            in_act = 0
        blk, e = self.plan.blocks[bi], P["blocks"][bi]
        if blk.expand is not None:
            z, in_act = self._conv(T, e["expand"], h, False), _RELU6
        else:
            z = h
        d = e["dw"]
        y = T.dwconv_act_fwd(z, d["w"], d["scale"], d["shift"], d["stride"], d["pad"], in_act, _RELU6, None)
        return h, y

    def prefix_fill(self, bi: int, kind: str) -> torch.Tensor:
        """(C_padded,) value a masked channel of block ``bi``'s post-depthwise output takes: zeros
        for ``"dw"``, clamp(folded depthwise BN shift, 0, 6) for ``"expand"`` (the padded channels'
        shift is 0, and they are never masked)."""
        d = self._pack()["blocks"][bi]["dw"]
        key = "fill_" + kind
        if key not in d:
            d[key] = torch.zeros_like(d["shift"]) if kind == "dw" else d["shift"].clamp(0.0, 6.0).contiguous()
        return d[key]

    def _tail_elems(self, bi: int, H: int, W: int) -> int:
        """Largest padded per-sample activation from block ``bi``'s (H, W) output to the classifier."""
        per = H * W * cpad(self.plan.blocks[bi].project.conv.weight.shape[0])
        for b in self.plan.blocks[bi + 1:]:
            hid = cpad(b.dw.conv.weight.shape[0])
            per = max(per, H * W * hid)
            H, W = _out_hw(b.dw.conv, H, W)
            per = max(per, H * W * hid, H * W * cpad(b.project.conv.weight.shape[0]))
        return max(per, H * W * cpad(self.plan.head.conv.weight.shape[0]))

    def downstream_elems(self, bi: int, sample_shape) -> int:
        """The largest padded per-sample activation downstream of block ``bi``'s output, that output
        included, for (C, H, W) inputs (Shapley sizes its stacked prefix batch from it)."""
        H, W = _out_hw(self.plan.stem.conv, *tuple(sample_shape)[-2:])
        for b in self.plan.blocks[:bi + 1]:
            H, W = _out_hw(b.dw.conv, H, W)
        return self._tail_elems(bi, H, W)

    def logits_from(self, bi: int, out: torch.Tensor) -> torch.Tensor:
        """Logits of the network continued from block ``bi``'s output (possibly K stacked copies
        along the batch), in slices wherever a tensor would reach 2^31 bytes (as :meth:`max_batch`
        does for the whole forward)."""
        T = ops.require()
        P = self._pack()
        step = max(1, ((1 << 31) - 1) // (4 * self._tail_elems(bi, out.shape[1], out.shape[2])))
        logits = []
        for s in range(0, out.shape[0], step):
            h = out[s:s + step]
            for b in range(bi + 1, len(self.plan.blocks)):
                h = self._block(T, self.plan.blocks[b], P["blocks"][b], h, 0)
            zh = self._conv(T, P["head"], h, False)
            logits.append(self._fc(T, P, T.avgpool_nhwc(zh.clamp_(0.0, 6.0))))
        return logits[0] if len(logits) == 1 else torch.cat(logits, 0)

    def block_logits(self, bi: int, h: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Logits from :meth:`forward_to`'s state, nothing masked."""
        blk, e = self.plan.blocks[bi], self._pack()["blocks"][bi]
        return self.logits_from(bi, self._conv(ops.require(), e["project"], y, False, res=h if blk.shortcut else None))

    def prefix_logits(self, bi: int, kind: str, h: torch.Tensor, y: torch.Tensor, perm_t: torch.Tensor,
                      rank_t: torch.Tensor, p0: int, cnt: int) -> torch.Tensor:
        """Logits (cnt * B, classes) of the prefixes p0 .. p0+cnt-1 of one permutation: copy j has the
        channels of rank < p0 + j masked at block ``bi``'s ``kind`` evaluation point. ``perm_t``:
        int32 (n,) over the real channels; ``rank_t``: its rank vector over the padded width (padding
        ranks after every real channel). ``TORCHPRUNER_PREFIX_DELTA=0`` (read per call) builds the
        cnt filled copies and runs the project conv on all of them instead."""
        T = ops.require()
        blk, e = self.plan.blocks[bi], self._pack()["blocks"][bi]
        B, Ho, Wo, C = y.shape
        fill = self.prefix_fill(bi, kind)
        res = h if blk.shortcut else None
        delta = os.environ.get("TORCHPRUNER_PREFIX_DELTA", "1") != "0"
        co = e["project"]["scale"].numel()
        # copies per piece: the stacked project output (and, without the delta, input) below 2^31 bytes
        piece = max(1, ((1 << 31) - 1) // (4 * B * Ho * Wo * (co if delta else max(co, C))))
        if cnt > piece:
            return torch.cat([self.prefix_logits(bi, kind, h, y, perm_t, rank_t, p0 + j, min(piece, cnt - j))
                              for j in range(0, cnt, piece)], 0)
        if delta:
            y_base = torch.where((rank_t < p0).view(1, 1, 1, C), fill, y)
            base = self._conv(T, e["project"], y_base, False, res=res)
            wt = self._bwd_operands(e["project"])["wt"]  # (C, Cout) with the BN scale folded in
            out = ops.prefix_project(base.view(B * Ho * Wo, co), y.view(B * Ho * Wo, C), fill, wt, perm_t, p0, cnt)
            return self.logits_from(bi, out.view(cnt * B, Ho, Wo, co))
        lim = torch.arange(p0, p0 + cnt, device=y.device, dtype=rank_t.dtype).view(cnt, 1, 1, 1, 1)
        ys = torch.where(rank_t.view(1, 1, 1, 1, C) < lim, fill, y.unsqueeze(0)).view(cnt * B, Ho, Wo, C)
        if res is not None and cnt > 1:
            res = res.repeat(cnt, 1, 1, 1)
        return self.logits_from(bi, self._conv(T, e["project"], ys, False, res=res))


# ====================================================================== MobileNetV3
# The same engine for the torchvision / models.mobilenet_v3 layout: units are (conv, BN, ReLU |
# Hardswish), the depthwise unit runs ``tpamd.dwconv_hs_fwd`` / ``dwconv_hs_dgrad`` with the units'
# activation codes (Hardswish keeps the pre-activation of its output for the backward: its derivative
# cannot be read from the output), a squeeze-and-excitation gate sits between the depthwise output
# and the project conv (the kernels of squeeze_excite.hip through ``ops.se_*``, on the padded NHWC
# layout: a padded channel has y = 0, so its gated value and every gradient there are exact zeros),
# and the classifier is Linear, Hardswish, Linear. Shapley prefixes are not served: a gate makes the
# project conv's input non-linear in the channel mask, so the running rank-1 subtraction of
# ``prefix_logits`` does not hold.
_ACT_CODES = {nn.ReLU: 1, nn.Hardswish: 3}
V3_SHAPLEY_REASON = ("mobilenet engine: Shapley on a MobileNetV3 is not served (a squeeze-and-excitation gate makes "
                     "the project conv's input non-linear in the channel mask, so the prefix scan does not hold)")


@dataclass
class _V3Block:
    expand: Optional[_Unit]
    dw: _Unit
    gate: Optional[nn.Module]
    project: _Conv
    shortcut: bool


@dataclass
class MobileNetV3Plan:
    stem: _Unit
    head: _Unit
    fc1: nn.Linear
    fc: nn.Linear
    blocks: list = field(default_factory=list)


def _act_code(act) -> int:
    return _ACT_CODES[type(act)]


def _unit_v3(seq, what):
    """(_Unit, "") of a conv-BN-(ReLU | Hardswish) Sequential, else (None, reason)."""
    if not isinstance(seq, nn.Sequential) or len(seq) != 3:
        return None, f"{what}: expected a (conv, BN, ReLU | Hardswish) Sequential"
    conv, bn, act = seq
    kind = _conv_kind(conv)
    if kind not in ("dense", "depthwise"):
        return None, f"{what}: {kind}"
    if not isinstance(bn, nn.BatchNorm2d) or bn.running_mean is None:
        return None, f"{what}: expected a BatchNorm2d with running statistics after the conv"
    if type(act) not in _ACT_CODES:
        return None, f"{what}: activation {type(act).__name__} is not supported (only ReLU and Hardswish)"
    return _Unit(conv, bn, act), ""


def _gate_reason(gate, hidden: int) -> str:
    """"" for a gate the kernels of squeeze_excite.hip compute (``engine.train.se_eligible``) on
    ``hidden`` channels, else why not."""
    from .train import _se_gate_code
    if _se_gate_code(gate) is None:
        inner = ", ".join(f"{n} {type(getattr(gate, n, None)).__name__}" for n in ("avgpool", "activation",
                                                                                   "scale_activation"))
        return f"unsupported gate ({inner}; needs a global average pool, a ReLU and a Hardsigmoid or Sigmoid)"
    if gate.fc1.weight.shape[1] != hidden or gate.fc2.weight.shape[1] != gate.fc1.weight.shape[0]:
        return "the gate's fc widths do not chain with the block's hidden width"
    if hidden + gate.fc1.weight.shape[0] > ops.se.SE_MAX_FC:
        return f"the gate's widths exceed {ops.se.SE_MAX_FC}"
    return ""


def build_mobilenet_v3_plan(model: nn.Module):
    """Lower a torchvision-layout MobileNetV3 (``models.mobilenet_v3``), or return (None, reason).
    Structural: widths are read from the tensors."""
    from ..utils.graph import is_channel_gate
    feats, cls = getattr(model, "features", None), getattr(model, "classifier", None)
    if not isinstance(feats, nn.Sequential) or len(feats) < 3 or cls is None or \
            not any(isinstance(getattr(m, "block", None), nn.Sequential) for m in feats):
        return None, "not a torchvision-layout MobileNetV3 (features / inverted-residual `.block`s / classifier)"
    pool = getattr(model, "avgpool", None)
    if pool is not None and not (isinstance(pool, nn.AdaptiveAvgPool2d) and pool.output_size in (1, (1, 1))):
        return None, "avgpool: unsupported pool before the classifier (needs a global AdaptiveAvgPool2d)"
    layers = list(cls.children()) if isinstance(cls, nn.Sequential) else [cls]
    if len(layers) < 3 or not isinstance(layers[0], nn.Linear) or type(layers[1]) is not nn.Hardswish or \
            not isinstance(layers[-1], nn.Linear) or not all(isinstance(m, nn.Dropout) for m in layers[2:-1]):
        return None, "classifier: unsupported shape (needs Linear, Hardswish, Dropout layers, Linear)"
    stem, why = _unit_v3(feats[0], "features.0 (stem)")
    if stem is None:
        return None, why
    if _conv_kind(stem.conv) != "dense" or stem.conv.weight.shape[2] != 3 or stem.conv.weight.shape[1] > 4 or \
            stem.conv.padding[0] != 1 or type(stem.act) is not nn.Hardswish:
        return None, "features.0 (stem): needs a 3x3 conv, padding 1, of at most 4 input channels, BN and Hardswish"
    last = len(feats) - 1
    head, why = _unit_v3(feats[-1], f"features.{last} (head)")
    if head is None:
        return None, why
    if _conv_kind(head.conv) != "dense" or not _is_1x1(head.conv) or type(head.act) is not nn.Hardswish:
        return None, f"features.{last} (head): needs a 1x1 conv, BN and Hardswish"
    plan = MobileNetV3Plan(stem, head, layers[0], layers[-1])
    width = stem.conv.weight.shape[0]
    for i, blk in enumerate(feats[1:-1], 1):
        what = f"features.{i}"
        seq = getattr(blk, "block", None)
        shape = "([1x1-BN-act,] depthwise-BN-act, [gate,] (1x1, BN))"
        if not isinstance(seq, nn.Sequential) or not 2 <= len(seq) <= 4:
            return None, f"{what}: expected an inverted-residual `.block` {shape}"
        items = list(seq)
        proj = items.pop()
        gate = items.pop() if len(items) > 1 and is_channel_gate(items[-1]) else None
        if not items or len(items) > 2 or not isinstance(proj, nn.Sequential) or len(proj) != 2:
            return None, f"{what}: expected an inverted-residual `.block` {shape}"
        expand = None
        if len(items) == 2:
            expand, why = _unit_v3(items[0], f"{what}.block.0 (expand)")
            if expand is None:
                return None, why
            if _conv_kind(expand.conv) != "dense" or not _is_1x1(expand.conv):
                return None, f"{what}.block.0: the expand conv must be a dense 1x1 conv"
        di = len(items) - 1
        dw, why = _unit_v3(items[-1], f"{what}.block.{di} (depthwise)")
        if dw is None:
            return None, why
        k, s, pd = dw.conv.weight.shape[2], dw.conv.stride[0], dw.conv.padding[0]
        if _conv_kind(dw.conv) != "depthwise" or k not in (3, 5) or s not in (1, 2) or pd > k - 1:
            return None, (f"{what}.block.{di}: the depthwise conv must be 3x3 / 5x5, stride 1 / 2, padding < k, "
                          "depth multiplier 1")
        hidden = dw.conv.weight.shape[0]
        if gate is not None:
            why = _gate_reason(gate, hidden)
            if why:
                return None, f"{what}.block.{di + 1}: {why}"
        pconv, pbn = proj
        kind = _conv_kind(pconv)
        if kind != "dense" or not _is_1x1(pconv):
            return None, f"{what}: the project conv must be a dense 1x1 conv" + ("" if kind == "dense" else f" ({kind})")
        if not isinstance(pbn, nn.BatchNorm2d) or pbn.running_mean is None:
            return None, f"{what}: expected a BatchNorm2d with running statistics after the project conv"
        if (expand.conv.weight.shape[:2] if expand else (hidden, width)) != (hidden, width) or \
                pconv.weight.shape[1] != hidden:
            return None, f"{what}: channel counts of the block's convs do not chain"
        cout = pconv.weight.shape[0]
        shortcut = getattr(blk, "use_res_connect", None)
        if shortcut is None:
            shortcut = s == 1 and cout == width
        if shortcut and (s != 1 or cout != width):
            return None, f"{what}: a shortcut needs stride 1 and equal widths"
        plan.blocks.append(_V3Block(expand, dw, gate, _Conv(pconv, pbn), bool(shortcut)))
        width = cout
    if head.conv.weight.shape[1] != width or plan.fc1.weight.shape[1] != head.conv.weight.shape[0] or \
            plan.fc.weight.shape[1] != plan.fc1.weight.shape[0]:
        return None, "channel counts of the head / classifier do not chain"
    return plan, ""


def _hs_slope(v: torch.Tensor) -> torch.Tensor:
    """Hardswish's derivative at the pre-activation v (the branch order of dwconv_act.hip)."""
    return torch.where(v < -3.0, torch.zeros_like(v), torch.where(v <= 3.0, v / 3.0 + 0.5, torch.ones_like(v)))


class MobileNetV3Engine(MobileNetEngine):
    shapley = False  # attributions/methods/shapley.py: the generic path serves these nets

    def eval_modules(self):
        """The ReLU / Hardswish modules the engine scores: per block the post-expand one (where the
        block expands) and the post-depthwise one (before the gate)."""
        return super().eval_modules()

    def _params_key(self):
        key = list(super()._params_key())
        extra = [self.plan.fc1.weight, self.plan.fc1.bias]
        for b in self.plan.blocks:
            if b.gate is not None:
                extra += [b.gate.fc1.weight, b.gate.fc1.bias, b.gate.fc2.weight, b.gate.fc2.bias]
        key += [(t.data_ptr(), t._version, tuple(t.shape)) for t in extra if t is not None]
        return tuple(key)

    # ------------------------------------------------------------------ packing
    @torch.no_grad()
    def _pack_gate(self, gate):
        """fc1 / fc2 as (Cs, C_padded) / (C_padded, Cs) matrices with zero columns / rows and a zero
        fc2 bias under the padding."""
        from .train import _se_gate_code
        w1, w2 = gate.fc1.weight.detach().float(), gate.fc2.weight.detach().float()
        cs, c = w1.shape[:2]
        cp = cpad(c)
        w1, w2 = F.pad(w1.reshape(cs, c), (0, cp - c)), F.pad(w2.reshape(c, cs), (0, 0, 0, cp - c))
        b1 = gate.fc1.bias.detach().float() if gate.fc1.bias is not None else torch.zeros(cs, device=w1.device)
        b2 = gate.fc2.bias.detach().float() if gate.fc2.bias is not None else torch.zeros(c, device=w1.device)
        return {"w1": w1.contiguous(), "b1": b1.contiguous(), "w2": w2.contiguous(),
                "b2": F.pad(b2, (0, cp - c)).contiguous(), "code": _se_gate_code(gate)}

    def _pack(self):
        key = self._params_key()
        if key == self._key:
            return self._packed
        p = self.plan
        blocks = []
        for b in p.blocks:
            blocks.append({"expand": self._pack_conv(b.expand) if b.expand is not None else None,
                           "dw": self._pack_dw(b.dw), "gate": self._pack_gate(b.gate) if b.gate is not None else None,
                           "project": self._pack_conv(b.project)})

        def fc(lin, pad_out):
            w = lin.weight.detach().float()
            n, c = w.shape
            npad = cpad(n) if pad_out else n
            w = F.pad(w, (0, cpad(c) - c, 0, npad - n))
            b = lin.bias.detach().float() if lin.bias is not None else torch.zeros(n, device=w.device)
            wt = F.pad(w, (0, 0, 0, cpad(npad) - npad)).t().contiguous()  # backward operand: (C, outputs padded to 32)
            return w.contiguous(), F.pad(b, (0, npad - n)).contiguous(), wt

        w1, b1, wt1 = fc(p.fc1, True)
        w2, b2, wt2 = fc(p.fc, False)
        self._packed = {"stem": self._pack_conv(p.stem, stem=True), "blocks": blocks, "head": self._pack_conv(p.head),
                        "fc1": {"fc_w": w1, "fc_b": b1, "fc_wt": wt1}, "fc_w": w2, "fc_b": b2, "fc_wt": wt2}
        self._key = key
        return self._packed

    # ------------------------------------------------------------------ forward
    def _block(self, T, blk, e, h, in_act, apoz=None, saved=None):
        """One block from its (linear, or for a fused stem pre-activation) input ``h``; appends
        (input, z, y, input activation code, pre-activation of y or None, gate state or None) to
        ``saved``."""
        apoz = apoz or {}
        if blk.expand is not None:
            z = self._conv(T, e["expand"], h, False, apoz=apoz.get(blk.expand.act))
            in_act = _act_code(blk.expand.act)
        else:
            z = h
        d = e["dw"]
        out_act = _act_code(blk.dw.act)
        pre = None
        if saved is not None and out_act == 3:
            s_, pd, k = d["stride"], d["pad"], d["w"].shape[2]
            pre = z.new_empty(z.shape[0], (z.shape[1] + 2 * pd - k) // s_ + 1, (z.shape[2] + 2 * pd - k) // s_ + 1,
                              z.shape[3])
        y = T.dwconv_hs_fwd(z, d["w"], d["scale"], d["shift"], d["stride"], d["pad"], in_act, out_act,
                            apoz.get(blk.dw.act), pre)
        gate, yg = None, y
        if blk.gate is not None:
            q = e["gate"]
            hh, sg = ops.se_gate_fwd(ops.se_pool(y), q["w1"], q["b1"], q["w2"], q["b2"], q["code"])
            yg = ops.se_scale(y, sg)
            gate = (hh, sg)
        out = self._conv(T, e["project"], yg, False, res=h if blk.shortcut else None)
        if saved is not None:
            saved.append((h, z, y, in_act, pre, gate))
        return out

    def _stem_out(self, T, P, x):
        """(the first block's input, its activation code): the stem's pre-activation for a block
        whose depthwise conv applies the Hardswish itself, else the activated output."""
        h = T.nchw_to_nhwc_pad(x.float().contiguous(), 4)
        h = self._conv(T, P["stem"], h, False)
        if self._stem_fused():
            return h, None, 3
        return F.hardswish(h), h, 0

    def _head(self, T, P, h):
        zh = self._conv(T, P["head"], h, False)
        feat = T.avgpool_nhwc(F.hardswish(zh))
        z1 = self._fc(T, P["fc1"], feat)
        return self._fc(T, P, F.hardswish(z1)), zh, z1

    def forward(self, x: torch.Tensor, apoz: Optional[dict] = None, save: bool = False):
        """As :meth:`MobileNetEngine.forward`; the last entry of ``saved`` is (head pre-activation,
        classifier pre-activation, stem pre-activation)."""
        T = ops.require()
        P = self._pack()
        apoz = dict(apoz or {})
        padded = []
        for m, buf in apoz.items():
            if buf.shape[1] % 32:
                tmp = buf.new_zeros(buf.shape[0], cpad(buf.shape[1]))
                padded.append((buf, tmp))
                apoz[m] = tmp
        h, z0, in_act = self._stem_out(T, P, x)
        if z0 is None:
            z0 = h
        saved = []
        for blk, e in zip(self.plan.blocks, P["blocks"]):
            h = self._block(T, blk, e, h, in_act, apoz, saved if save else None)
            in_act = 0
        logits, zh, z1 = self._head(T, P, h)
        for buf, tmp in padded:
            buf.add_(tmp[:, :buf.shape[1]])
        if save:
            saved.append((zh, z1, z0))
            return logits, saved
        return logits

    # ------------------------------------------------------------------ backward (Taylor, Sensitivity)
    def grad_scores(self, x: torch.Tensor, y: torch.Tensor, want, mode: str, criterion=None,
                    loss_batch: Optional[int] = None, raw_slabs: bool = False):
        """As :meth:`MobileNetEngine.grad_scores`. A gated block's post-depthwise score is reduced
        from (y, dL/dy) after the gate's backward (dL/dy = g * s + dp / HW: through the scale and
        through the pooled mean)."""
        T = ops.require()
        P = self._pack()
        logits, saved = self.forward(x, save=True)
        zh, z1, _ = saved.pop()
        B = logits.shape[0]
        blocks = self.plan.blocks
        first = min((bi for bi, b in enumerate(blocks)
                     if b.dw.act in want or (b.expand is not None and b.expand.act in want)), default=None)
        out = {}
        if first is None:
            return out
        g_log = logits_grad(logits, y, criterion, loss_batch)
        # classifier: Linear, Hardswish, Linear (the GEMM kernel's mask operand is all ones: no ReLU here)
        g1 = self._fc_bwd(T, P, g_log, torch.ones_like(z1)) * _hs_slope(z1)
        g_feat = self._fc_bwd(T, P["fc1"], g1, zh.new_ones(B, zh.shape[3]))
        HW = zh.shape[1] * zh.shape[2]
        g = (g_feat / HW)[:, None, None, :] * _hs_slope(zh)  # avg-pool backward + the head's Hardswish
        g, _ = self._dgrad(T, P["head"], g.contiguous(), None)
        akey = (tuple(x.shape), mode, tuple(sorted(i for i, m in enumerate(self.eval_modules()) if m in want)))
        size = self._arena_sizes.get(akey)
        arena = [torch.zeros(size, device=x.device) if size else None, 0, 0]
        for bi in range(len(blocks) - 1, first - 1, -1):
            blk, e = blocks[bi], P["blocks"][bi]
            h, z, yd, in_act, pre, gate = saved[bi]
            gy, _ = self._dgrad(T, e["project"], g, None)  # dL/d(project input), unfactored
            if gate is not None:
                q, (hh, sg) = e["gate"], gate
                _, _, dp = ops.se_gate_bwd(ops.se_bwd_reduce(gy, yd), sg, hh, q["w1"], q["w2"], q["code"])
                gy = ops.se_bwd_dx(gy, sg, dp)  # dL/d(depthwise activation output)
            if blk.dw.act in want:
                out[blk.dw.act] = ops.channel_reduce(yd.permute(0, 3, 1, 2), gy.permute(0, 3, 1, 2), mode)
            ex_wanted = blk.expand is not None and blk.expand.act in want
            if bi == first and not ex_wanted:
                break
            d = e["dw"]
            _, H, W, C = z.shape
            tay = self._slab(arena, T.dwconv_hs_tay_slots(H, W, C), B, C, x.device) if ex_wanted else None
            out_act = _act_code(blk.dw.act)
            dz = T.dwconv_hs_dgrad(gy, pre if out_act == 3 else yd, d["w"], d["scale"], z, H, W, d["stride"], d["pad"],
                                   in_act, out_act, tay, _TAY_MODES[mode])
            if ex_wanted:
                if raw_slabs:
                    out[blk.expand.act] = tay
                else:
                    sums = tay.sum(0)
                    out[blk.expand.act] = sums.abs_() if mode == "taylor" else sums
            if bi == first:
                break
            if blk.expand is not None:  # the block input is linear: no factor
                g, _ = self._dgrad(T, e["expand"], dz, None, res=g if blk.shortcut else None)
            else:
                g = dz + g if blk.shortcut else dz
        if arena[2] > (size or 0):
            self._arena_sizes[akey] = arena[2]
        return out

    # ------------------------------------------------------------------ Shapley: not served
    def forward_to(self, *a, **k):
        raise NotImplementedError(V3_SHAPLEY_REASON)

    prefix_logits = logits_from = block_logits = prefix_fill = forward_to


_ENGINES: "weakref.WeakKeyDictionary[nn.Module, MobileNetEngine]" = weakref.WeakKeyDictionary()


def mobilenet_engine_default() -> bool:
    """``TORCHPRUNER_MOBILENET_ENGINE`` (default 0: the engine is opt-in)."""
    return os.environ.get("TORCHPRUNER_MOBILENET_ENGINE", "0") not in ("0", "")


def _engine_sig(eng):
    return (type(eng), [c.conv for c in eng._all_convs()], [b.shortcut for b in eng.plan.blocks],
            [getattr(b, "gate", None) for b in eng.plan.blocks])


def maybe_mobilenet_engine(model, eval_modules, device, grad=False, why=None, shapley=False):
    """A MobileNetEngine (MobileNetV2 layout) or MobileNetV3Engine when every eval module is a block
    activation the engine serves, else None (``why`` receives the reason). ``grad`` is accepted for
    symmetry with the ResNet engine: the same modules are served forward (APoZ) and backward
    (Taylor, Sensitivity). ``shapley``: the caller wants prefix evaluation, which a MobileNetV3 does
    not get (``V3_SHAPLEY_REASON``)."""
    from .fused_chain import _reject, engines_enabled
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if not engines_enabled():
        return _reject(why, "mobilenet engine: engines disabled (TORCHPRUNER_ENGINES=0)")
    if shapley and build_mobilenet_plan(model)[0] is None and build_mobilenet_v3_plan(model)[0] is not None:
        return _reject(why, V3_SHAPLEY_REASON)
    if dev.type != "cuda" or ops.backend() == "torch" or not ops.available() or model.training:
        return _reject(why, "mobilenet engine: needs an eval-mode model on a GPU with the native extension")
    if any(p.dtype != torch.float32 for p in model.parameters()):
        return _reject(why, "mobilenet engine: parameters are not float32")
    plan, reason = build_mobilenet_plan(model)  # re-validated every run: pruning changes channel counts
    cls = MobileNetEngine
    if plan is None:
        plan, reason3 = build_mobilenet_v3_plan(model)
        cls = MobileNetV3Engine
        if plan is None:  # the reason of the layout the model looks like
            v3 = any(isinstance(getattr(m, "block", None), nn.Sequential) for m in getattr(model, "features", []))
            return _reject(why, f"mobilenet engine: {reason3 if v3 else reason}")
    new = cls(model, plan)
    eng = _ENGINES.get(model)
    if eng is None or _engine_sig(eng) != _engine_sig(new):
        eng = new
        _ENGINES[model] = eng
    ok = set(map(id, eng.eval_modules()))
    if not all(id(m) in ok for m in eval_modules):
        return _reject(why, "mobilenet engine: evaluation modules must be the activation (ReLU6; ReLU / Hardswish "
                            "of a MobileNetV3) after a block's expand or depthwise conv (use "
                            "find_best_evaluation_module=True)")
    return eng
