"""Fused attribution engine for conv chains (VGG-style CNNs and MLP heads) on MI355X.

The reference scores one module per full forward+backward pass, through PyTorch hooks, with
the conv/BN/ReLU/pool ops as separate cuDNN/ATen kernels (attributions.py:58-68,
taylor.py:18-49). This engine lowers an eval-mode chain

    [Conv3x3 -> BN -> ReLU (-> MaxPool2x2)]*  -> flatten -> [Dropout] Linear [ReLU] ...

into a handful of HIP kernels per layer and computes Taylor scores for EVERY layer in ONE
forward + input-gradient-only backward:

forward   conv_first (VALU direct conv, NCHW->NHWC) then conv_fwd per layer: implicit-GEMM
          fp32 MFMA with BN folded into a per-channel affine, NaN-propagating ReLU and the
          2x2 max-pool fused in the epilogue (pooled value + argmax byte stored; the
          full-resolution activation never touches HBM).
loss      fused softmax cross-entropy: per-sample loss and dL/dlogits in one kernel.
backward  conv_dgrad per layer: the same GEMM on flipped/transposed weights; its epilogue
          reads the consumer activation once and emits (a) the Taylor partial
          sum_hw -(dL/da * a) per (sample, channel) and (b) dL/d(pre-activation) masked by
          the ReLU and scaled by the BN scale. Max-pool backward is fused into the NEXT
          dgrad's operand loader (unpool by argmax on the fly).
          No weight gradients, no autograd graph, no activation clones, no host syncs.

Numerics: fp32 end to end (MFMA f32 is a bit-exact fp32 FMA chain); BN folding and GEMM
summation order differ from cuDNN/MIOpen only at rounding level.
"""
from __future__ import annotations

import contextlib
import math
import os
import sys
import weakref
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from . import epochs

# tile configs of conv_mfma.hip: 0=128x128, 1=256x64, 2=64x64, 3=128x64 (4 waves);
# 4=128x128, 5=256x64, 6=128x64 (8 waves)
_CU = 256
_TILES = {0: (128, 128), 1: (256, 64), 2: (64, 64), 3: (128, 64), 4: (128, 128), 5: (256, 64), 6: (128, 64)}
WINO = -1  # pseudo tile cfg: fused Winograd F(2x2,3x3) kernel (winograd.hip), direct patch loads
WINO_LDS = -2  # the same with the block input region staged through LDS
WINO_UNP = -3  # dgrad of a pooled layer: explicit vectorised unpool, then the staged kernel on the
               # dense full-resolution gradient (vs rebuilding it from pooled cells per chunk)
WINO4 = -4  # Winograd F(4x4,3x3) kernel (wino4.hip): square 4/8/16/32-pixel maps, 1.78x fewer MFMAs
# (-5 was the WIDE F(4x4) kernel: measured 0.8x MODE 3 on every VGG layer, removed in round 6)
WINO_BF = -6  # bf16 operands (compute_dtype=bfloat16): the staged F(2x2) kernel with bf16 U images and
              # v_mfma_f32_16x16x16_bf16 (winograd.hip BF); fp32 transforms, accumulation and epilogues
WINO_BF_UNP = -7  # its dgrad of a pooled layer after an explicit unpool (as WINO_UNP)
WINO4S = -8  # F(4x4) MODE 3 with split transform points (wino4.hip variant 3): each wave of a 16-tile
             # pair owns 18 of the 36 points x all 32 outputs, so each wave forms half of V = B^T d B
             # (72 packed VALU ops per 72 MFMAs instead of 168): the default F(4x4) kernel
WINO4S_FU = -11  # its data gradient writing the output unpooled through the previous block's pool
                 # argmax (one K pass): no separate unpooling pass for the next data gradient
WINO4_FU = -12  # the same with the MODE 3 kernel
CFG_SK = 32  # tile-config flag of the GEN implicit GEMM: stream-K (conv_mfma.hip launch_gen)
CFG_SB = 64  # tile-config flag: single-buffered LDS stage (GEN 1 1x1 forward, one K pass; short-K convs)
CFG_RED = 1 << 12  # tuner-only flag (never passed to a kernel): a plain dgrad + the separate channel reduction
CFG_BF16 = 256  # tile-config flag of conv_igemm: bf16 operands / fp32 accumulation (opt-in, compute_dtype)
FAST2 = 200  # pseudo cfg offset: 2x2-map conv as nine batched channel products (conv2x2_fast.hip) on
             # implicit-GEMM tile config cfg - FAST2
_BF16_CFGS = (0, 2, 3)  # the implicit-GEMM tiles built with bf16 variants (conv_mfma.hip launch_any)
            # than F(2x2); dgrads of pooled layers take the explicit unpool first

# Winograd F(2x2,3x3) weight transform G g G^T
_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


@torch.no_grad()
def winograd_weights(w: torch.Tensor) -> torch.Tensor:
    """(K, C, 3, 3) conv weight -> U = G g G^T arranged as the LDS images winograd.hip DMAs:
    (C/8, K/32, 4096), one 16-KB image per (8-input-channel chunk, 32-output-channel block).
    Inside an image, word ((xi*2 + e)*16 + j)*8 + 2*(g ^ 2*(j >> 3)) + n holds
    U[xi][c = 8*cb + 2g + e][k = 32*kb + j + 16n]: one ds_read_b64 feeds both MFMA column
    tiles of lane (j, g) and the XOR keeps lanes j, j+8 on different banks.
    Computed in fp64, rounded once to fp32."""
    K, C = w.shape[0], w.shape[1]
    assert w.shape[2:] == (3, 3) and K % 32 == 0 and C % 8 == 0, \
        "winograd_weights needs 3x3 kernels, K % 32 == 0 and C % 8 == 0"
    G = torch.tensor(_G, dtype=torch.float64, device=w.device)
    u = torch.einsum("ia,kcab,jb->ijck", G, w.double(), G).reshape(16, C // 8, 4, 2, K // 32, 2, 16)
    # (xi, cb, g, e, kb, n, j) -> (cb, kb, xi, e, j, g, n)
    img = u.permute(1, 4, 0, 3, 6, 2, 5).contiguous()
    img[:, :, :, :, 8:] = img[:, :, :, :, 8:, [2, 3, 0, 1]]
    return img.reshape(C // 8, K // 32, 4096).float().contiguous()


# 2x2-map conv as 9 channel products (conv2x2_fast.hip): weight transform U = G w G^T on taps
# [W0, W1, W2], input transform Bt, output transform At (nested 2x2 Toeplitz products, 3 mults each)
_G2 = ((0.0, 1.0, 0.0), (0.0, -1.0, 1.0), (1.0, -1.0, 0.0))
_BT2 = ((1.0, 1.0), (0.0, 1.0), (1.0, 0.0))
_AT2 = ((1.0, 1.0, 0.0), (1.0, 0.0, 1.0))


@torch.no_grad()
def fast2x2_weights(w: torch.Tensor, dgrad: bool = False) -> torch.Tensor:
    """(K, C, 3, 3) conv weight -> U9 (9, K, C), U9[3i + j][k][c] = (G w[k][c] G^T)[i][j]: the nine
    (output rows, input channels) GEMM operands of the 2x2-map conv. ``dgrad``: of the flipped,
    transposed weight (the data gradient's operand, (9, C, K)). Computed in fp64, rounded once."""
    assert w.dim() == 4 and w.shape[2:] == (3, 3), "fast2x2_weights needs (K, C, 3, 3) kernels"
    if dgrad:
        w = w.flip(2, 3).transpose(0, 1)
    G = torch.tensor(_G2, dtype=torch.float64, device=w.device)
    u = torch.einsum("ia,kcab,jb->ijkc", G, w.double(), G)
    return u.reshape(9, w.shape[0], w.shape[1]).float().contiguous()


def taylor_slots(H: int, W: int) -> int:
    """Partial slots R of the (R, B, C) Taylor slab the Winograd dgrad writes for an activation
    of spatial size H x W (one slot per 64-tile block covering an image; mirrors
    wino_taylor_slots() in winograd.hip). score_fold sums the slots in order."""
    if H == 2 and W == 2:
        return 4  # dense-GEMM layers (2x2 images) keep one slot per pixel
    T = ((H + 1) // 2) * ((W + 1) // 2)  # odd sizes: partial last tile row / column
    if T <= 0:
        return 1
    if T % 64 == 0:
        return T // 64
    if 64 % T == 0:
        return 1
    return (T + 63) // 64 + 1


def _wino_ok(H, W, C, K):
    return H % 2 == 0 and W % 2 == 0 and C % 8 == 0 and K % 32 == 0


def _wino4_ok(H, W, C, K):
    return H == W and H in (4, 8, 16, 32) and C % 8 == 0 and K % 32 == 0


_W4_SPLITS = os.environ.get("TORCHPRUNER_W4_SPLITS", "1") != "0"
_TUNER_LOG = os.environ.get("TORCHPRUNER_TUNER_LOG", "0") != "0"  # print every timed kernel choice
_TUNER_LOG_ALL = os.environ.get("TORCHPRUNER_TUNER_LOG", "0") == "2"  # ... and every candidate's time
_TUNE_ROUNDS = int(os.environ.get("TORCHPRUNER_TUNE_ROUNDS", "3"))
_TUNE_MARGIN = float(os.environ.get("TORCHPRUNER_TUNE_MARGIN", "0.02"))


_W4_VARIANT = {WINO4: 0, WINO4S: 3, WINO4S_FU: 3, WINO4_FU: 0}
_W4_FUSED = (WINO4S_FU, WINO4_FU)


def _wino4_cands(B, H, W, K, C):
    """F(4x4) candidates: one K pass, plus channel-chunk split-K (raw slabs + the shared
    deterministic combine) when the tile grid alone cannot fill the chip (small batches); for
    the split-points kernel (the untuned pick) and MODE 3 (32-tile blocks, two per CU)."""
    out = []
    for kind, tb, per_cu in ((WINO4S, 32, 2), (WINO4, 32, 2)):
        blocks = math.ceil(B * (H // 4) * (W // 4) / tb) * (K // 32)
        sp, chunks = 1, C // 8
        while _W4_SPLITS and blocks * sp < per_cu * _CU and sp * 2 <= chunks // 4 and sp < 16:
            sp *= 2
        out += [(kind, 1)] + ([(kind, sp)] if sp > 1 else []) + ([(kind, sp // 2)] if sp > 2 else [])
    return out


def _wino_splits(P, K, C):
    tiles = math.ceil(P / 64) * (K // 32)
    splits, chunks = 1, C // 8
    while tiles * splits < 2 * _CU and splits * 2 <= chunks // 4 and splits < 16:
        splits *= 2
    return splits


def _splits_for(M, N, K, bm, bn):
    tiles = math.ceil(M / bm) * math.ceil(N / bn)
    splits, kt = 1, K // 32
    while tiles * splits < 2 * _CU and splits * 2 <= kt // 4 and splits < 16:
        splits *= 2
    return splits


def sk_candidates(T, cands, ks: int, M: int, N: int, tay: bool = False):
    """Stream-K variants (cfg | CFG_SK, 1) of the GEN implicit-GEMM tile configs in ``cands``
    where stream-K applies at this shape: the tiles x k-slices space is cut into one equal range per
    co-resident block, so the last partial wave of output tiles (ResNet's 1x1 GEMMs at B=256 leave
    up to ~40% of the CUs idle in it) is spread over the whole chip. The C++ side decides
    applicability (T.conv_sk_ws: the fixup workspace, 0 = not applicable)."""
    out = []
    for c in dict.fromkeys(c for c, _ in cands if 0 <= c <= 6):
        if T.conv_sk_ws(c, ks, tay, M, N) > 0:
            out.append((c | CFG_SK, 1))
    return out


def _pick_cfg(M: int, N: int, K: int):
    """Heuristic (tile cfg, split-K) so a launch has enough workgroups for 256 CUs."""
    best = None
    for cfg in (0, 3, 1, 2):
        bm, bn = _TILES[cfg]
        if N <= 64 and bn == 128:
            continue
        tiles = math.ceil(M / bm) * math.ceil(N / bn)
        splits = _splits_for(M, N, K, bm, bn)
        waste = (math.ceil(M / bm) * bm * math.ceil(N / bn) * bn) / (M * N)
        score = (min(tiles * splits, 2 * _CU) / (2 * _CU)) / waste * (1.0 if bm * bn >= 128 * 64 else 0.85)
        score *= 1.0 if splits == 1 else 0.9
        if best is None or score > best[0]:
            best = (score, cfg, splits)
    return best[1], best[2]


class Autotuner:
    """Per-shape choice of (tile cfg, split-K) by timing every candidate once on the real
    operands (the analogue of cudnn.benchmark; disable with TORCHPRUNER_AUTOTUNE=0)."""

    def __init__(self):
        self.cache = {}
        self.enabled = os.environ.get("TORCHPRUNER_AUTOTUNE", "1") != "0"
        self.policy = None
        # bumped whenever a fixed()/pinned() context swaps the choice cache: captured HIP graphs
        # bake in the kernels chosen when they were captured, so their keys include it
        self.gen = 0
        # > 1 while tuning the shapes of small batches that will run ``concurrency`` in flight on
        # as many HIP streams (attributions/base.py _BatchPipeline): candidates are then timed as
        # that many concurrent launches, i.e. by throughput, not by the latency of one launch
        # alone — alone, split-K looks best because it fills the idle CUs; in flight, the other
        # batches fill them and split-K's partial slabs and combine launch are pure extra work
        self.concurrency = 1
        self._streams = []

    @contextlib.contextmanager
    def fixed(self):
        """Untimed heuristic kernel choices with a private cache: every run of the same shapes
        picks the same configs, so results are bit-reproducible across processes (accuracy
        protocols, teacher training). Timing-based choices can differ between runs on a busy
        GPU, and different split-K / tile configs round differently."""
        saved = (self.cache, self.enabled, self.policy)
        self.cache, self.enabled, self.policy = {}, False, None
        self.gen += 1
        try:
            yield self
        finally:
            self.cache, self.enabled, self.policy = saved
            self.gen += 1

    @contextlib.contextmanager
    def pinned(self, policy):
        """Kernel choices made by ``policy(key, candidates, M, N, K) -> (cfg, splits)`` (None: the
        untuned pick) with a private cache, never by timing: numerics tests pin one kernel family
        at a time (:func:`family_policy`), so what they measure cannot depend on the box."""
        saved = (self.cache, self.enabled, self.policy)
        self.cache, self.enabled, self.policy = {}, False, policy
        self.gen += 1
        try:
            yield self
        finally:
            self.cache, self.enabled, self.policy = saved
            self.gen += 1

    def candidates(self, M, N, K, wino=None, wino_only=False):
        """``wino``: (P tiles, C) when the Winograd kernel applies to this conv; ``wino_only``
        drops the implicit-GEMM configs (conv dgrad: the Winograd epilogue's Taylor sums are
        atomic-free and bit-reproducible, the GEMM's are not)."""
        out = []
        if wino is not None:
            sp = _wino_splits(wino[0], N, wino[1])
            for kind in (WINO, WINO_LDS):
                out += [(kind, sp)] + ([(kind, max(1, sp // 2))] if sp > 1 else []) + ([(kind, 1)] if sp > 2 else [])
            if wino_only:
                return out
        for cfg, (bm, bn) in _TILES.items():
            if N <= 64 and bn == 128:
                continue
            sp = _splits_for(M, N, K, bm, bn)
            out.append((cfg, sp))
            if sp > 1:
                out.append((cfg, max(1, sp // 2)))
            if sp > 2:  # small batches: one K pass without the partial-slab combine launch
                out.append((cfg, 1))
        return out

    def choose(self, key, M, N, K, run, wino=None, wino_only=False, cands=None):
        """``run(cfg, splits)`` launches the op once (must be side-effect free); ``cands``
        overrides the candidate list (first entry = the fallback when tuning is off)."""
        hit = self.cache.get(key)
        if hit is not None:
            return hit
        if self.policy is not None:
            lst = cands if cands is not None else self.candidates(M, N, K, wino, wino_only and wino is not None)
            res = self.policy(key, lst, M, N, K) or lst[0]
            self.cache[key] = res
            return res
        if not self.enabled or torch.cuda.is_current_stream_capturing():
            if cands is not None:
                res = cands[0]
            else:
                res = (WINO_LDS, _wino_splits(wino[0], N, wino[1])) if wino is not None else _pick_cfg(M, N, K)
            self.cache[key] = res
            return res
        # every candidate timed round-robin (warm launch, then the min over _TUNE_ROUNDS rounds of 2
        # launches): back-to-back timings of configs within a few % of each other are dominated by
        # clock (DVFS) drift, which made single-shot choices vary from box to box; and the untuned
        # pick (lst[0], what TUNER.fixed() runs) is kept unless another is _TUNE_MARGIN faster
        lst = list(cands if cands is not None else self.candidates(M, N, K, wino, wino_only and wino is not None))
        times = {}
        conc = max(1, int(self.concurrency))
        if conc > 1:
            while len(self._streams) < conc:
                self._streams.append(torch.cuda.Stream())
        for r in range(_TUNE_ROUNDS):
            for cand in lst:
                if r == 0:
                    run(*cand)  # warm
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if conc > 1:  # conc concurrent launch pairs, normalised to one pair
                    cur = torch.cuda.current_stream()
                    for st in self._streams[:conc]:
                        st.wait_event(e0)
                        with torch.cuda.stream(st):
                            for _ in range(2):
                                run(*cand)
                    for st in self._streams[:conc]:
                        cur.wait_stream(st)
                else:
                    for _ in range(2):
                        run(*cand)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1) / conc
                times[cand] = min(times.get(cand, t), t)
        fast = min(lst, key=lambda c: times[c])
        best = (times[fast], fast)
        if times[lst[0]] <= times[fast] * (1.0 + _TUNE_MARGIN):
            best = (times[lst[0]], lst[0])
        self.cache[key] = best[1]
        if _TUNER_LOG:
            print(f"[tuner] {key} -> {best[1]} ({best[0] / 2 * 1e3:.1f} us{f', {conc} in flight' if conc > 1 else ''})",
                  file=sys.stderr, flush=True)
            if _TUNER_LOG_ALL:
                print("[tuner]     " + ", ".join(f"{c}: {times[c] / 2 * 1e3:.1f}" for c in sorted(times, key=times.get)),
                      file=sys.stderr, flush=True)
        return best[1]


TUNER = Autotuner()

_KIND_NAMES = {WINO: "wino2_direct", WINO_LDS: "wino2", WINO_UNP: "wino2_unpool", WINO4: "wino4_m3",
               WINO_BF: "wino2_bf16", WINO_BF_UNP: "wino2_bf16_unpool", WINO4S: "wino4", -10: "first_direct",
               WINO4S_FU: "wino4_fused_unpool", WINO4_FU: "wino4_m3_fused_unpool"}


def kernel_name(cfg: int) -> str:
    """Readable name of a tuner choice: a Winograd kind, ``igemm<tile>`` (``_TILES``), ``dense2x2``
    igemm (2x2 layers as one dense GEMM), ``fast2x2`` igemm (2x2 layers as nine batched channel
    products), ``bf16`` igemm variants, or a persistent 1x1 GEMM."""
    if cfg in _KIND_NAMES:
        return _KIND_NAMES[cfg]
    if cfg >= CFG_RED:
        return kernel_name(cfg - CFG_RED) + "+reduce"
    if CFG_SK <= cfg < CFG_SK + 7:
        return kernel_name(cfg - CFG_SK) + "_streamk"
    if CFG_SB <= cfg < CFG_SB + 7:
        return kernel_name(cfg - CFG_SB) + "_1stage"
    if FAST2 <= cfg < FAST2 + 7:
        bm, bn = _TILES[cfg - FAST2]
        return f"fast2x2_igemm{bm}x{bn}"
    if cfg >= 100 and cfg < CFG_BF16:
        bm, bn = _TILES.get(cfg - 100, (0, 0))
        return f"dense2x2_igemm{bm}x{bn}"
    if cfg >= CFG_BF16:
        bm, bn = _TILES.get(cfg - CFG_BF16, (0, 0))
        return f"igemm{bm}x{bn}_bf16"
    if cfg in _TILES:
        bm, bn = _TILES[cfg]
        return f"igemm{bm}x{bn}" + ("_8w" if cfg >= 4 else "")
    return f"cfg{cfg}"


def tuner_choices(cache=None) -> dict:
    """The autotuner's per-shape picks as ``{key: [kernel, splits]}`` (bench JSON ``tuner_choices``:
    which kernel family / split each layer ran on this box, so box-to-box spread is diagnosable)."""
    cache = TUNER.cache if cache is None else cache
    out = {}
    for key, (cfg, sp) in cache.items():
        out["/".join(str(k).replace(" ", "") for k in key)] = [kernel_name(cfg), int(sp)]
    return out


def cpad(c: int, q: int = 32) -> int:
    """Channel count rounded up to the MFMA K-slice / column-tile granule the kernels need."""
    return -(-c // q) * q


@dataclass
class ConvBlock:
    conv: nn.Conv2d
    bn: Optional[nn.BatchNorm2d]
    relu: Optional[nn.Module]
    pool: Optional[nn.MaxPool2d]
    first: bool = False
    width: int = 0  # padded output width carried by the engine's activations


@dataclass
class LinearBlock:
    linear: nn.Linear
    relu: Optional[nn.Module]  # the block's activation: nn.ReLU or nn.LeakyReLU (slope >= 0)
    width: int = 0

    @property
    def slope(self) -> float:
        return _act_slope(self.relu)


def _act_slope(m) -> float:
    """Negative-side slope of a block activation (0 for ReLU)."""
    return float(m.negative_slope) if isinstance(m, nn.LeakyReLU) else 0.0


def _is_block_act(m) -> bool:
    return isinstance(m, nn.ReLU) or (isinstance(m, nn.LeakyReLU) and m.negative_slope >= 0)


@dataclass
class Plan:
    convs: list = field(default_factory=list)
    linears: list = field(default_factory=list)
    flatten: bool = False  # the chain has an explicit Flatten stage

    def input_error(self, shape) -> Optional[str]:
        """Why an input of ``shape`` is not what this chain computes on (None when it is): the
        engine would otherwise silently read a differently shaped input as the planned one."""
        shape = tuple(shape)
        if self.convs:
            npool = sum(b.pool is not None for b in self.convs)
            side = 1 << npool
            cin = self.convs[0].conv.in_channels
            if len(shape) != 4 or shape[1] != cin or shape[2] != side or shape[3] != side:
                return f"input {shape} is not (B, {cin}, {side}, {side}) (features must end at 1x1)"
            return None
        fin = self.linears[0].linear.in_features
        feat = math.prod(shape[1:]) if len(shape) > 1 else 0
        if feat != fin or (len(shape) != 2 and not self.flatten):
            return f"input {shape} is not (B, {fin})" + ("" if self.flatten else " (no Flatten stage)")
        return None

    def eval_module_of(self, i):
        blk = self.blocks[i]
        return blk.relu

    @property
    def blocks(self):
        return self.convs + self.linears


def _stages(model):
    if hasattr(model, "_stages"):
        return list(model._stages())
    if isinstance(model, nn.Sequential):
        return list(model.children())
    return None


def build_plan(model: nn.Module):
    """Lower ``model`` to a Plan, or return (None, reason)."""
    stages = _stages(model)
    if stages is None:
        return None, "model has no linear stage list (forward_partial chain or nn.Sequential)"
    plan = Plan()
    i = 0
    n = len(stages)
    while i < n and isinstance(stages[i], nn.Conv2d):
        conv = stages[i]
        if conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.padding != (1, 1) or \
                conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros":
            return None, f"unsupported conv {conv}"
        i += 1
        bn = relu = pool = None
        if i < n and isinstance(stages[i], nn.BatchNorm2d):
            bn = stages[i]
            i += 1
        if i < n and isinstance(stages[i], nn.ReLU):
            relu = stages[i]
            i += 1
        if relu is None:
            return None, "conv block without ReLU"
        if i < n and isinstance(stages[i], nn.MaxPool2d):
            pool = stages[i]
            k = pool.kernel_size if isinstance(pool.kernel_size, int) else pool.kernel_size[0]
            s = pool.stride if isinstance(pool.stride, int) else pool.stride[0]
            if k != 2 or s != 2 or pool.padding not in (0, (0, 0)) or pool.dilation not in (1, (1, 1)) \
                    or pool.ceil_mode:
                return None, f"unsupported pool {pool}"
            i += 1
        first = len(plan.convs) == 0
        # pruned (odd) channel counts are carried zero-padded to a multiple of 32: padded
        # filters have zero weights and a zero BN affine, so their outputs, gradients and
        # scores are exactly 0 and never influence the real channels
        width = cpad(conv.out_channels)
        if first and conv.in_channels % 32 != 0:
            if conv.out_channels > 64:
                return None, "first (tiny-Cin) conv must have at most 64 outputs"
            width = 16 if conv.out_channels <= 16 else width
        plan.convs.append(ConvBlock(conv, bn, relu, pool, first=first and conv.in_channels % 32 != 0,
                                    width=width))
    # flatten (a conv-less MLP may start with it or take flattened inputs)
    if i < n and (isinstance(stages[i], nn.Flatten) or getattr(stages[i], "__name__", "") == "_flatten"):
        i += 1
        plan.flatten = True
    elif plan.convs:
        return None, "expected flatten after the conv stack"
    while i < n:
        st = stages[i]
        if isinstance(st, nn.Dropout):
            i += 1
            continue
        if isinstance(st, nn.Linear):
            i += 1
            act = None
            if i < n and _is_block_act(stages[i]):
                act = stages[i]
                i += 1
            plan.linears.append(LinearBlock(st, act, cpad(st.out_features)))
            continue
        return None, f"unsupported classifier stage {st}"
    if not plan.linears or any(b.relu is None for b in plan.linears[:-1]) or plan.linears[-1].relu is not None:
        return None, "classifier must be Linear(+ReLU/LeakyReLU) blocks ending in a plain Linear"
    if plan.convs and plan.linears[0].linear.in_features != plan.convs[-1].conv.out_channels:
        return None, "features must end at 1x1 spatial resolution"
    plan.linears[-1].width = plan.linears[-1].linear.out_features  # logits stay unpadded
    return plan, ""


class FusedChainEngine:
    """Executes a Plan with the HIP kernels. Weights are re-packed lazily whenever a
    parameter changes identity, storage or version (e.g. after pruning / training)."""

    def __init__(self, model: nn.Module, plan: Plan):
        self.plan = plan
        self._key = None
        self._packed = None
        self._arenas = {}
        self._graphs = {}  # HIP graphs of taylor() per (shapes, blocks, mode)
        self.use_wino = os.environ.get("TORCHPRUNER_WINOGRAD", "1") != "0"
        # opt-in bf16 operands for the 3x3 convs (compute_dtype=torch.bfloat16): products on
        # v_mfma_f32_32x32x16_bf16 with fp32 accumulation; activations, epilogues, gradients and
        # score accumulators stay fp32 / fp64. Never the default (the headline is exact fp32).
        self.bf16 = False

    # ------------------------------------------------------------------ weights
    def _params_key(self):
        key = []
        for b in self.plan.convs:
            for t in (b.conv.weight, b.conv.bias) + ((b.bn.weight, b.bn.bias, b.bn.running_mean, b.bn.running_var)
                                                     if b.bn is not None else ()):
                if t is not None:
                    key.append((t.data_ptr(), t._version, tuple(t.shape)))
        for b in self.plan.linears:
            for t in (b.linear.weight, b.linear.bias):
                if t is not None:
                    key.append((t.data_ptr(), t._version, tuple(t.shape)))
        key.append(epochs.engine_key())  # fused optimizers / native BN stats leave versions alone
        return tuple(key)

    @torch.no_grad()
    def _pack(self):
        key = self._params_key()
        if key == self._key:
            return self._packed
        convs = []
        cin_p = None  # padded width of the previous block's activation
        for b in self.plan.convs:
            w = b.conv.weight.detach().float()
            cout = w.shape[0]
            bias = b.conv.bias.detach().float() if b.conv.bias is not None else torch.zeros(cout, device=w.device)
            if b.bn is not None:
                inv = torch.rsqrt(b.bn.running_var.float() + b.bn.eps)
                g = b.bn.weight.float() if b.bn.weight is not None else torch.ones_like(inv)
                beta = b.bn.bias.float() if b.bn.bias is not None else torch.zeros_like(inv)
                scale = g * inv
                shift = (bias - b.bn.running_mean.float()) * scale + beta
            else:
                scale = torch.ones(cout, device=w.device)
                shift = bias
            wp = b.width - cout
            w = F.pad(w, (0, 0, 0, 0, 0, (cin_p - w.shape[1]) if cin_p is not None else 0, 0, wp))
            scale, shift = F.pad(scale, (0, wp)), F.pad(shift, (0, wp))
            cin_p, cout = b.width, b.width
            entry = {"scale": scale.contiguous(), "shift": shift.contiguous(), "pool": b.pool is not None,
                     "w4d": w.contiguous()}
            if b.first:
                entry["w_first"] = w.contiguous()
                entry["w_first_t"] = w.permute(1, 2, 3, 0).contiguous()  # tap-major VALU operand, packed once
                if self.use_wino and w.shape[1] <= 8 and cout % 32 == 0:
                    # tiny-Cin first layer on the Winograd MFMA kernel: input padded to 8 channels
                    entry["u_first"] = winograd_weights(F.pad(w, (0, 0, 0, 0, 0, 8 - w.shape[1])))
            else:
                entry["w"] = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()  # [n][(kh,kw,ci)]
            # dgrad operand: flipped taps, transposed channels -> [ci][(kh,kw,co)]
            entry["wt"] = w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous()
            if self.use_wino:
                if not b.first and cout % 32 == 0 and w.shape[1] % 8 == 0:
                    entry["u"] = winograd_weights(w)
                if w.shape[1] % 32 == 0 and cout % 8 == 0:
                    entry["ut"] = winograd_weights(w.flip(2, 3).transpose(0, 1))
            convs.append(entry)
        lins = []
        if cin_p is None:  # conv-less MLP: input features zero-padded to the 32-wide K granule
            cin_p = cpad(self.plan.linears[0].linear.in_features)
        for b in self.plan.linears:
            w = b.linear.weight.detach().float()
            n_out = w.shape[0]
            bias = b.linear.bias.detach().float() if b.linear.bias is not None else torch.zeros(n_out, device=w.device)
            w = F.pad(w, (0, cin_p - w.shape[1], 0, b.width - n_out))
            bias = F.pad(bias, (0, b.width - n_out))
            cin_p = n_out = b.width
            pad = (-n_out) % 32
            wt = w.t()
            if pad:
                wt = torch.cat([wt, torch.zeros(wt.shape[0], pad, device=w.device)], 1)
            lins.append({"w": w.contiguous(), "bias": bias.contiguous(), "wt": wt.contiguous(), "pad": pad,
                         "relu": b.relu is not None, "slope": b.slope})
        self._packed = {"convs": convs, "lins": lins}
        self._key = key
        return self._packed

    # ------------------------------------------------------------------ execution
    FIRST_DIRECT = -10  # pseudo cfg: VALU direct first-layer kernel

    def _first_run(self, T, e, xf, cfg, sp, apoz=None):
        """First (tiny-Cin) conv block -> (output, argmax or None): the block's 2x2 max-pool is
        fused into the Winograd epilogue, or applied after the VALU direct conv."""
        if cfg == self.FIRST_DIRECT:
            h = T.conv_first(xf, e["w_first"], e["scale"], e["shift"], True, e["w_first_t"])
            if apoz is not None:
                apoz += ops.channel_reduce(h.permute(0, 3, 1, 2), None, "apoz")
            return T.maxpool2_nhwc(h) if e["pool"] else (h, None)
        xp = T.nchw_to_nhwc_pad(xf, 8)
        return T.conv_wino_fwd(xp, e["u_first"], e["scale"], e["shift"], True, e["pool"], sp, cfg == WINO_LDS, apoz)

    def _first(self, T, e, x, apoz=None):
        xf = x.float().contiguous()
        B, _, H, W = xf.shape
        N = e["scale"].numel()
        if "u_first" not in e or not _wino_ok(H, W, 8, N):
            return self._first_run(T, e, xf, self.FIRST_DIRECT, 1, apoz)
        cands = [(WINO_LDS, 1), (self.FIRST_DIRECT, 1), (WINO, 1)]
        cfg, sp = TUNER.choose(("first", tuple(xf.shape), N, e["pool"]), B * H * W, N, 27,
                               lambda c, s_, e=e, xf=xf: self._first_run(T, e, xf, c, s_), cands=cands)
        return self._first_run(T, e, xf, cfg, sp, apoz)

    @staticmethod
    def _u4(e, dgrad=False):
        """F(4x4,3x3) U images of the entry's weight (forward, or the flipped/transposed data-gradient
        operand), built on first use and cached in the packed entry."""
        key = "ut4" if dgrad else "u4"
        u = e.get(key)
        if u is None:
            u = e[key] = ops.require().wino4_weights(e["w4d"], dgrad, 0, 0)
        return u

    # A 3x3/pad-1 conv on a 2x2 image is a dense GEMM: every output pixel q sees input pixel p
    # through tap (p - q + 1): y(B, 4K) = x(B, 4C) @ Wbig^T with Wbig (4K, 4C) — the same 2.25x
    # fewer multiplies as Winograd, on the implicit-GEMM kernel (ks=1) with no transforms.
    DENSE = 100  # pseudo cfg offset: cfg = DENSE + implicit-GEMM tile config

    @staticmethod
    def _dense(e):
        d = e.get("dense")
        if d is None:
            N = e["scale"].numel()
            C = e["w"].shape[1] // 9
            w9 = e["w"].view(N, 3, 3, C)
            wb = e["w"].new_zeros(4, N, 4, C)  # [q][k][p][c]
            for q in range(4):
                for p in range(4):
                    wb[q, :, p, :] = w9[:, p // 2 - q // 2 + 1, p % 2 - q % 2 + 1, :]
            wb = wb.reshape(4 * N, 4 * C)
            d = {"w": wb.contiguous(), "wt": wb.t().contiguous(), "scale4": e["scale"].repeat(4).contiguous(),
                 "shift4": e["shift"].repeat(4).contiguous()}
            e["dense"] = d
        return d

    @staticmethod
    def _u9(e, dgrad=False):
        """U9 = G w G^T operands of the nine-product 2x2-map conv (forward, or the flipped/transposed
        data-gradient operand), built on first use and cached in the packed entry."""
        key = "u9t" if dgrad else "u9"
        u = e.get(key)
        if u is None:
            u = e[key] = fast2x2_weights(e["w4d"], dgrad)
        return u

    @staticmethod
    def _fast2_cands(B, N, C):
        """Nine-product candidates of a 2x2-map conv (B x C).(C x N) x 9: every implicit-GEMM tile in
        one K pass and with the split-K that fills the chip (nine batches quantise badly on 256 CUs:
        128x128 tiles of B=2048, N=512 are 576 blocks, so a 2-way split is offered as well)."""
        out = []
        for cfg, (bm, bn) in _TILES.items():
            if N <= 64 and bn == 128:
                continue
            tiles = 9 * math.ceil(B / bm) * math.ceil(N / bn)
            sp, kt = 1, C // 32
            while tiles * sp < 2 * _CU and sp * 2 <= kt // 4 and sp < 16:
                sp *= 2
            sps = {sp, max(1, sp // 2), 1}
            if sp == 1 and kt >= 8:
                sps.add(2)
            out += [(FAST2 + cfg, s_) for s_ in sorted(sps)]
        return out

    @staticmethod
    def _ubf(e, dgrad=False):
        """bf16 F(2x2) U images (the WINO_BF kernels) of the entry's weight, built on first use."""
        key = "utb" if dgrad else "ub"
        u = e.get(key)
        if u is None:
            u = e[key] = ops.require().wino_weights(e["w4d"], dgrad, 0, 0, True)
        return u

    @staticmethod
    def _wino_bf_cands(T, B, H, W, N, C, pooled_grad=False):
        """bf16 Winograd candidates ([0] = the untuned pick) when the staged kernels cover the
        map (the BF kernels exist for the staged input modes only)."""
        if not T.wino_staged_ok(H, W, False):
            return []
        sp = _wino_splits(B * (H // 2) * (W // 2), N, C)
        sps = sorted({sp, max(1, sp // 2), 1}, reverse=True)
        kinds = [WINO_BF]
        if pooled_grad:
            kinds = ([WINO_BF] if T.wino_staged_ok(H, W, True) else []) + [WINO_BF_UNP]
        return [(k, s_) for k in kinds for s_ in sps]

    def _conv_run(self, T, e, h, cfg, sp, apoz=None):
        """``apoz``: (B, N) buffer that receives the counts of positive (pre-pool) outputs."""
        if cfg == WINO_BF:
            return T.conv_wino_fwd(h, self._ubf(e), e["scale"], e["shift"], True, e["pool"], sp, True, apoz)
        if cfg >= CFG_BF16:
            return T.conv_fwd(h, e["w"], e["scale"], e["shift"], True, e["pool"], 3, cfg, sp, apoz)
        if cfg in _W4_VARIANT:
            return T.conv_wino4_fwd(h, self._u4(e), e["scale"], e["shift"], True, e["pool"], apoz, sp,
                                    _W4_VARIANT[cfg])
        if cfg in (WINO, WINO_LDS):
            return T.conv_wino_fwd(h, e["u"], e["scale"], e["shift"], True, e["pool"], sp, cfg == WINO_LDS, apoz)
        if cfg >= FAST2:
            if apoz is None:  # the pool (value + argmax byte) is part of the combine
                return T.conv2x2_fast_fwd(h, self._u9(e), e["scale"], e["shift"], True, e["pool"], cfg - FAST2, sp)
            y, _ = T.conv2x2_fast_fwd(h, self._u9(e), e["scale"], e["shift"], True, False, cfg - FAST2, sp)
            apoz += ops.channel_reduce(y.permute(0, 3, 1, 2), None, "apoz")
            return T.maxpool2_nhwc(y) if e["pool"] else (y, None)
        if cfg >= self.DENSE:
            d = self._dense(e)
            B, N = h.shape[0], e["scale"].numel()
            y, _ = T.conv_fwd(h.reshape(B, 1, 1, -1), d["w"], d["scale4"], d["shift4"], True, False, 1,
                              cfg - self.DENSE, sp)
            y = y.view(B, 2, 2, N)
            if apoz is not None:
                apoz += ops.channel_reduce(y.permute(0, 3, 1, 2), None, "apoz")
            return T.maxpool2_nhwc(y) if e["pool"] else (y, None)
        return T.conv_fwd(h, e["w"], e["scale"], e["shift"], True, e["pool"], 3, cfg, sp, apoz)

    def _conv(self, T, e, h, apoz=None):
        B, H, W, C = h.shape
        M = B * H * W
        N, K = e["scale"].numel(), e["w"].shape[1]
        wino = (B * (H // 2) * (W // 2), C) if "u" in e and _wino_ok(H, W, C, N) else None
        cands = None
        if self.bf16 and C % 32 == 0:
            cands = self._bf16_cands(M, N, K)
            if wino is not None:  # [0] (the untuned / TUNER.fixed() pick): bf16 F(2x2), bf16-rounded V
                cands = self._wino_bf_cands(T, B, H, W, N, C) + cands
        elif H == 2 and W == 2 and C % 32 == 0:
            cands = [(self.DENSE + c, s_) for c, s_ in TUNER.candidates(B, 4 * N, 4 * C)] + \
                TUNER.candidates(M, N, K, wino) + self._fast2_cands(B, N, C)
        elif self.use_wino and _wino4_ok(H, W, C, N) and "w4d" in e:
            cands = _wino4_cands(B, H, W, N, C) + TUNER.candidates(M, N, K, wino)  # [0] = the untuned pick
        cfg, sp = TUNER.choose(("fwd", tuple(h.shape), N, e["pool"], wino is not None, self.bf16), M, N, K,
                               lambda c, s_, e=e, hh=h: self._conv_run(T, e, hh, c, s_), wino, cands=cands)
        return self._conv_run(T, e, h, cfg, sp, apoz)

    @staticmethod
    def _bf16_cands(M, N, K):
        """bf16-operand implicit-GEMM candidates ([0] = the untuned pick)."""
        return [(CFG_BF16 + c, s_) for c, s_ in TUNER.candidates(M, N, K) if c in _BF16_CFGS]

    def _dgrad_run(self, T, e, g, am, act, sc, taylor, want_out, cfg, sp, sc4=None, tm=0, unp=None):
        """``tm``: score partials the epilogue writes — 0 Taylor -(g*a), 1 Sensitivity |g|.
        ``unp``: argmax bytes of the 2x2 pool that produced ``act``: an F(4x4) kernel in one K
        pass then writes its output unpooled (full resolution, the previous layer's operand)."""
        assert (unp is not None) == (cfg in _W4_FUSED) and (unp is None or (sp == 1 and want_out)), \
            "fused unpooling: the F(4x4) *_FU kinds, splits=1, with an output"
        if cfg in (WINO_BF, WINO_BF_UNP):
            if cfg == WINO_BF_UNP:
                g, am = T.unpool2_nhwc(g, am), None
            return T.conv_wino_dgrad(g, am, self._ubf(e, True), act, sc, taylor, want_out, sp, True, tay_mode=tm)
        if cfg >= CFG_BF16:
            return T.conv_dgrad(g, am, e["wt"], act, sc, taylor, want_out, 3, cfg, sp, tay_mode=tm)
        if cfg in _W4_VARIANT:
            if am is not None:
                g = T.unpool2_nhwc(g, am)
            return T.conv_wino4_dgrad(g, self._u4(e, True), act, sc, taylor, want_out, tm, sp,
                                      _W4_VARIANT[cfg], unp)
        if cfg == WINO_UNP:
            return T.conv_wino_dgrad(T.unpool2_nhwc(g, am), None, e["ut"], act, sc, taylor, want_out, sp, True,
                                     tay_mode=tm)
        if cfg in (WINO, WINO_LDS):
            return T.conv_wino_dgrad(g, am, e["ut"], act, sc, taylor, want_out, sp, cfg == WINO_LDS, tay_mode=tm)
        if cfg >= FAST2:  # a pooled gradient is unpooled by the input transform
            out = T.conv2x2_fast_dgrad(g, am, self._u9(e, True), act, sc, taylor, want_out, cfg - FAST2, sp, tm)
            return out if want_out else None
        if cfg >= self.DENSE:
            d = self._dense(e)
            if am is not None:
                g = T.unpool2_nhwc(g, am)
            B, C = act.shape[0], act.shape[3]
            out = T.conv_dgrad(g.reshape(B, 1, 1, -1), None, d["wt"], act.reshape(B, 1, 1, -1), sc4, taylor,
                               want_out, 1, cfg - self.DENSE, sp, C, tay_mode=tm)
            return out.view(B, 2, 2, C) if want_out else out
        return T.conv_dgrad(g, am, e["wt"], act, sc, taylor, want_out, 3, cfg, sp, tay_mode=tm)

    def _linear(self, T, e, xin):
        B = xin.shape[0]
        cfg, sp = TUNER.choose(("lin", tuple(xin.shape), e["w"].shape[0]), B, e["w"].shape[0], e["w"].shape[1],
                               lambda c, s_, e=e, xin=xin: T.conv_fwd(xin, e["w"], None, e["bias"], e["relu"],
                                                                    False, 1, c, s_, slope=e["slope"]))
        out, _ = T.conv_fwd(xin, e["w"], None, e["bias"], e["relu"], False, 1, cfg, sp, slope=e["slope"])
        return out

    def _mlp_input(self, x: torch.Tensor) -> torch.Tensor:
        """Flattened fp32 input of a conv-less chain, zero-padded to the packed K: (B, 1, 1, Kp)."""
        B = x.shape[0]
        kp = self._pack()["lins"][0]["w"].shape[1]
        h = x.reshape(B, -1).float()
        if h.shape[1] != kp:
            h = F.pad(h, (0, kp - h.shape[1]))
        return h.contiguous().view(B, 1, 1, kp)

    def forward(self, x: torch.Tensor, stop_after: Optional[int] = None, apoz: Optional[dict] = None):
        """Forward pass; returns (logits, saved) where saved holds what backward needs.
        With ``stop_after=k`` returns (output of block k in engine layout, saved) instead:
        NHWC (pooled when the block pools) for conv blocks, (B,1,1,N) for linear blocks.
        ``apoz`` maps block indices to zeroed (B, padded width) buffers that receive, per sample
        and unit, the count of positive outputs of the block's ReLU (before pooling)."""
        err = self.plan.input_error(x.shape)
        if err:
            raise ValueError(f"fused chain engine: {err}")
        T = ops.require()
        P = self._pack()
        B = x.shape[0]
        apoz = apoz or {}
        acts = []  # per conv: (activation NHWC (pooled if pool), argmax or None)
        h = None
        for ci, (blk, e) in enumerate(zip(self.plan.convs, P["convs"])):
            if ci == 0 and blk.first:
                h, am = self._first(T, e, x, apoz.get(ci))
            else:
                if ci == 0:
                    h = x.float().permute(0, 2, 3, 1).contiguous()
                h, am = self._conv(T, e, h, apoz.get(ci))
            acts.append((h, am if e["pool"] else None))
            if stop_after == ci:
                return h, {"acts": acts}
        lin_acts = [h.reshape(B, 1, 1, -1) if h is not None else self._mlp_input(x)]
        nconv = len(self.plan.convs)
        for li, e in enumerate(P["lins"]):
            lin_acts.append(self._linear(T, e, lin_acts[-1]))
            if nconv + li in apoz:
                apoz[nconv + li] += ops.channel_reduce(lin_acts[-1].permute(0, 3, 1, 2), None, "apoz")
            if stop_after == nconv + li:
                return lin_acts[-1], {"acts": acts, "lin_acts": lin_acts}
        logits = lin_acts[-1].reshape(B, -1)
        return logits, {"acts": acts, "lin_acts": lin_acts}

    def forward_from(self, k: int, h: torch.Tensor) -> torch.Tensor:
        """Logits of the network given the output ``h`` of block ``k`` (engine layout)."""
        T = ops.require()
        P = self._pack()
        nconv = len(self.plan.convs)
        B = h.shape[0]
        for ci in range(k + 1, nconv):
            h, _ = self._conv(T, P["convs"][ci], h)
        if k < nconv:
            h = h.reshape(B, 1, 1, -1)
        for li in range(max(0, k + 1 - nconv), len(P["lins"])):
            h = self._linear(T, P["lins"][li], h)
        return h.reshape(B, -1)

    # ------------------------------------------------------------------ Shapley prefix deltas
    def prefix_delta_ok(self, k: int) -> bool:
        """Whether prefixes masked at block ``k``'s output can be evaluated by the prefix-delta GEMM:
        the next block is a Linear fed by that output (classifier blocks, or the last conv block
        at 1x1 resolution)."""
        nconv = len(self.plan.convs)
        return nconv - 1 <= k < len(self.plan.blocks) - 1 and os.environ.get("TORCHPRUNER_PREFIX_DELTA", "1") != "0"

    def _lin4(self, j):
        """Linear j's packed operands with rows padded to a multiple of 4 (the GEN epilogue's
        float4 columns) and the -1 scale vector of the delta GEMM; cached in the packed entry."""
        e = self._pack()["lins"][j]
        if "w4" not in e:
            n = e["w"].shape[0]
            n4 = -(-n // 4) * 4
            e["w4"] = F.pad(e["w"], (0, 0, 0, n4 - n)).contiguous()
            e["b4"] = F.pad(e["bias"], (0, n4 - n)).contiguous()
            e["neg1"] = torch.full((n4,), -1.0, device=e["w"].device)
        return e

    def prefix_delta_loss(self, k: int, zk: torch.Tensor, perm_t: torch.Tensor, rank_t: torch.Tensor, p0: int,
                          cnt: int, y: torch.Tensor, criterion=None) -> torch.Tensor:
        """Per-sample losses (cnt, B) of prefixes p0 .. p0+cnt-1 (units of rank < p0+j zeroed in
        copy j) of block ``k``'s output ``zk``, without materialising the cnt masked copies:

          Y_{p0+j} = Y_{p0} - sum_{i<j} z[:, perm[p0+i]] W[:, perm[p0+i]]^T
                   = Y_{p0} - (T @ Wsub^T)[j]        (T lower-triangular, cnt x Kc per sample)

        Y_{p0} is one (B x C) GEMM of the base-masked input; the deltas are one (cnt*B x Kc) GEMM
        whose epilogue subtracts from the broadcast Y_{p0} and applies the next block's
        activation — cnt*Kc/C of the FLOPs of the masked-copy GEMM, and no (cnt*B x C) copies.
        ``rank_t`` covers the padded width (padding ranks after every real unit)."""
        T = ops.require()
        nconv = len(self.plan.convs)
        j = k + 1 - nconv
        e = self._lin4(j)
        B = zk.shape[0]
        z2 = zk.reshape(B, -1)
        N4, C = e["w4"].shape
        zm = T.prefix_mask(z2.reshape(B, C, 1, 1), rank_t, int(p0), 1).view(B, 1, 1, C)
        cfg, sp = TUNER.choose(("pd0", B, C, N4), B, N4, C,
                               lambda c, s_: T.conv_fwd(zm, e["w4"], None, e["b4"], False, False, 1, c, s_))
        y0 = T.conv_fwd(zm, e["w4"], None, e["b4"], False, False, 1, cfg, sp)[0].view(B, N4)
        kc = cpad(cnt)
        tri, wsub = T.prefix_tri_operands(z2, e["w4"], perm_t, int(p0), int(cnt), kc)
        cfg2, _ = TUNER.choose(("pd1", cnt * B, kc, N4), cnt * B, N4, kc,
                               lambda c, s_: T.prefix_delta(tri, wsub, e["neg1"], y0, e["relu"], e["slope"], c),
                               cands=[(c, 1) for c in (0, 3, 1, 4, 5, 6, 2)])
        out = T.prefix_delta(tri, wsub, e["neg1"], y0, e["relu"], e["slope"], cfg2)  # (cnt*B, N4)
        yy = y.repeat(cnt)
        if j == len(self.plan.linears) - 1:  # the delta GEMM produced the logits
            n = self.plan.linears[-1].linear.out_features
            logits = out if n == N4 else out[:, :n].contiguous()
            loss = per_sample_loss(logits, yy, criterion)
        else:
            loss = self.loss_from(k + 1, out.view(cnt * B, 1, 1, N4), yy, criterion)
        return loss.view(cnt, B)

    def loss_from(self, k: int, h: torch.Tensor, y: torch.Tensor, criterion=None) -> torch.Tensor:
        """Per-sample loss (cross-entropy, or ``criterion``: :func:`per_sample_loss`) of the
        network continued from block ``k``'s output."""
        return per_sample_loss(self.forward_from(k, h), y, criterion)

    def _block_hw(self, b, H0, W0):
        """Spatial size of block b's output activation for an H0 x W0 input."""
        H, W = H0, W0
        for i, blk in enumerate(self.plan.convs):
            if blk.pool is not None:
                H, W = H // 2, W // 2
            if i == b:
                return H, W
        return 1, 1

    def max_batch(self, sample_shape) -> int:
        """Largest batch whose activations stay inside the kernels' 32-bit buffer descriptors
        (every tensor < 2^31 bytes) for inputs of per-sample shape ``sample_shape`` ((C, H, W)
        images or flat features); larger batches are run in slices (attributions/base.py)."""
        shape = tuple(sample_shape)
        per = 4 * 8 * max(1, math.prod(shape))  # the (channel-padded) input
        if self.plan.convs and len(shape) == 3:
            H, W = shape[1], shape[2]
            for blk in self.plan.convs:
                per = max(per, 4 * H * W * blk.width)  # the conv output, before its pooling
                if blk.pool is not None:
                    H, W = H // 2, W // 2
        for blk in self.plan.linears:
            per = max(per, 4 * blk.width)
        return max(1, ((1 << 31) - 1) // per)

    def _arena_shapes(self, B, want, H0, W0):
        shapes = {}
        nconv = len(self.plan.convs)
        for b in sorted(want):
            c = self._block_width(b)
            if b < nconv:
                shapes[b] = (taylor_slots(*self._block_hw(b, H0, W0)), B, c)
            else:
                shapes[b] = (B, c)
        return shapes

    def score_arena(self, B: int, want, device, hw=(32, 32), slot: int = 0):
        """Persistent zeroed score slabs for the blocks in ``want`` (one allocation): (R, B, C)
        partial slots for conv blocks (see taylor_slots), (B, C) for linear blocks. The caller
        must leave them zeroed (ops.score_fold_ with after=2) for reuse. ``slot``: independent
        arenas for batches in flight on different streams."""
        key = (B, tuple(sorted(want)), str(device), tuple(hw), slot)
        arena = self._arenas.get(key)
        if arena is None:
            shapes = self._arena_shapes(B, want, *hw)
            flat = torch.zeros(sum(math.prod(sh) for sh in shapes.values()), device=device)
            arena, off = {}, 0
            for b, sh in shapes.items():
                n = math.prod(sh)
                arena[b] = flat[off:off + n].view(sh)
                off += n
            self._arenas[key] = arena
        return arena

    @staticmethod
    def per_sample(t: torch.Tensor) -> torch.Tensor:
        """(B, C) view of a folded score slab (slot 0 of an (R, B, C) arena entry)."""
        return t[0] if t.dim() == 3 else t

    def _block_width(self, b):
        """Padded width of block b's output in engine layout (score slabs use it too)."""
        return self.plan.blocks[b].width

    def real_width(self, b):
        """Number of real (unpadded) units of block b."""
        blk = self.plan.blocks[b]
        return blk.conv.out_channels if isinstance(blk, ConvBlock) else blk.linear.out_features

    # HIP-graph replay of the fused step (TORCHPRUNER_GRAPHS): "auto" (default) = for batches up to
    # GRAPH_MAX_B when two or more batches are in flight on the stream pipeline; "1" = also for
    # one batch at a time; "all" = any batch size; "0" = never. One batch at a time the step is
    # GPU-bound down to B=8 (profiles/archive/hip_graphs_taylor_step.txt), but with two batches in flight
    # the GPU finishes a B=100 step (~55 launches) faster than Python enqueues it: the host spent
    # 0.77-0.99 ms per batch in the pipeline against 0.85-1.04 ms of wall
    # (scripts/probes/b100_host_probe.py), so the pipelined launches replay one graph per slot. Large
    # batches are GPU-bound: replay trims ~1% at B=2048, but the graphs' multi-GB private pools
    # then slowed later small-batch work in the same process by 7-17%
    # (profiles/bench/large_batch_graphs_vs_eager.txt), so the default stops at 1024.
    GRAPH_MAX_B = int(os.environ.get("TORCHPRUNER_GRAPH_MAX_B", "1024"))

    def _bound_graph_cache(self, limit: int = 64):
        """Bound the captured graphs (each holds a private memory pool). Replays of the graphs
        being dropped may still run on the pipeline's streams, and dropping a graph returns its
        pool to the allocator: wait for the device first (rare: only past ``limit`` entries)."""
        if len(self._graphs) > limit:
            torch.cuda.synchronize()
            self._graphs.clear()

    def graphs_enabled(self, B: int, pipelined: bool = False) -> bool:
        mode = os.environ.get("TORCHPRUNER_GRAPHS", "auto")
        if mode == "all":
            return True
        if mode == "auto":
            return pipelined and B <= self.GRAPH_MAX_B
        return mode == "1" and B <= self.GRAPH_MAX_B

    def taylor_graphed(self, x: torch.Tensor, y: torch.Tensor, want: set, arena: dict, mode="taylor",
                       criterion=None, warm: bool = False, loss_batch: Optional[int] = None):
        """``taylor()`` replayed from a captured HIP graph: the ~40 launches of one fused
        forward + input-gradient backward become one graph launch, which is what small,
        launch-bound batches need. One graph per (input shapes, blocks, mode, score arena,
        packed weights): the first call of a new key runs eagerly (it also autotunes the kernels
        and builds the lazily packed operands), the second captures, later calls copy the batch
        into the graph's static inputs and replay. Re-packed weights (pruning, training) or a
        new arena invalidate the graph. ``arena`` must be zero before each call, as for
        ``taylor()`` (ops.score_fold_ with after=2 leaves it so). ``warm=True``: the caller ran
        this shape eagerly already (kernels tuned, operands packed): capture on the first call
        (the stream pipeline's first batch of a shape runs alone, eagerly)."""
        if criterion is not None:  # a user criterion runs through autograd: eager launches
            return self.taylor(x, y, want, arena, mode, criterion, loss_batch)
        P = self._pack()
        # one graph per score arena: the stream pipeline replays slot k's graph into slot k's arena
        key = (tuple(x.shape), x.dtype, tuple(y.shape), y.dtype, tuple(sorted(want)), mode, str(x.device), self.bf16,
               loss_batch, TUNER.gen, id(arena))
        g = self._graphs.get(key)
        if g is not None and (g["P"] is not P or g["arena"] is not arena):
            torch.cuda.synchronize()  # its replays must finish before the stale graph (and pool) goes
            g = None
        if g is None:
            seen = self._graphs.get(("seen",) + key)
            if not warm and (seen is None or seen[0] is not P or seen[1] is not arena):
                self._graphs[("seen",) + key] = (P, arena)
                return self.taylor(x, y, want, arena, mode, loss_batch=loss_batch)
            sx, sy = x.clone(), y.clone()
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                self.taylor(sx, sy, want, arena, mode, loss_batch=loss_batch)
            torch.cuda.current_stream(x.device).wait_stream(side)
            self._bound_graph_cache()
            g = self._graphs[key] = {"graph": graph, "x": sx, "y": sy, "P": P, "arena": arena}
        g["x"].copy_(x)
        g["y"].copy_(y)
        g["graph"].replay()
        return {b: arena[b] for b in want}

    # ------------------------------------------------------------------ Shapley prefix evaluations
    def shapley_static(self, k: int, zk: torch.Tensor, y: torch.Tensor) -> dict:
        """Static device buffers of a Shapley prefix evaluation of block ``k``'s output (one
        batch): the activation, the labels and the shifted rank vector that the captured graphs
        of :meth:`shapley_eval` read. Copies this batch in (two launches per batch)."""
        key = ("sv_static", k, tuple(zk.shape), tuple(y.shape), str(zk.device), self.bf16, TUNER.gen)
        st = self._graphs.get(key)
        if st is None:
            self._bound_graph_cache()
            st = self._graphs[key] = {"z": torch.empty_like(zk), "y": torch.empty_like(y), "rank": None,
                                      "graphs": {}, "seen": {}, "k": k}
        st["z"].copy_(zk)
        st["y"].copy_(y)
        return st

    def shapley_eval(self, st: dict, rank_padded: torch.Tensor, p_first: int, cnt: int) -> torch.Tensor:
        """Per-sample losses (cnt, B) of prefixes p_first .. p_first+cnt-1 (units of rank < p
        zeroed) of the activation in ``st``, replayed from a HIP graph per ``cnt``: the prefix
        offset enters as a shifted rank vector (rank - p_first, one eager launch) so the graph
        holds the mask kernel with p0 = 0 (rank < p0 + j <=> rank - p0 < j: the same mask, the
        same losses bit for bit). A prefix chunk is otherwise ~20-40 launches of small work:
        shallow layers were host-bound (profiles/bench/host_bound_probe_paths.txt)."""
        P = self._pack()
        if st["rank"] is None or st["rank"].shape != rank_padded.shape:
            if st["graphs"]:
                torch.cuda.synchronize()
            st["rank"] = torch.empty_like(rank_padded)
            st["graphs"].clear()
        torch.sub(rank_padded, p_first, out=st["rank"])
        B = st["z"].shape[0]

        def run():
            z_cl = st["z"].permute(0, 3, 1, 2)  # channels_last view
            masked = ops.prefix_mask(z_cl, st["rank"], 0, cnt)
            return self.loss_from(st["k"], masked.permute(0, 2, 3, 1), st["y"].repeat(cnt)).view(cnt, B)

        g = st["graphs"].get(cnt)
        if g is not None and g["P"] is not P:
            torch.cuda.synchronize()  # its replays must finish before the stale graph (and pool) goes
            g = None
        if g is None:
            if st["seen"].get(cnt) is not P:  # first use of this chunk size: eager (autotunes, allocates)
                st["seen"][cnt] = P
                return run()
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(st["z"].device)
            side.wait_stream(torch.cuda.current_stream(st["z"].device))
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                out = run()
            torch.cuda.current_stream(st["z"].device).wait_stream(side)
            g = st["graphs"][cnt] = {"graph": graph, "out": out, "P": P}
        g["graph"].replay()
        return g["out"].clone()  # the caller keeps the last row across the next replay

    def apoz_graphed(self, x: torch.Tensor, blocks, slot: int = 0, warm: bool = False) -> dict:
        """``forward(x, stop_after=max(blocks), apoz=zeroed (B, width) count buffers)`` replayed from
        a captured HIP graph (one per input shape, blocks and pipeline slot; the first call of a
        key runs eagerly). Returns the count buffers: graph outputs that stay valid until this
        slot's next replay (the stream pipeline folds them on the same stream first). ``warm``:
        as for :meth:`taylor_graphed`."""
        P = self._pack()
        blocks = tuple(sorted(blocks))
        key = ("apoz", tuple(x.shape), x.dtype, str(x.device), blocks, slot, self.bf16, TUNER.gen)
        g = self._graphs.get(key)
        if g is not None and g["P"] is not P:
            torch.cuda.synchronize()  # its replays must finish before the stale graph (and pool) goes
            g = None

        def run(xx):
            bufs = {b: torch.zeros(xx.shape[0], self._block_width(b), device=xx.device) for b in blocks}
            self.forward(xx, stop_after=blocks[-1], apoz=bufs)
            return bufs

        if g is None:
            if not warm and self._graphs.get(("seen",) + key) is not P:
                self._graphs[("seen",) + key] = P
                return run(x)
            sx = x.clone()
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                bufs = run(sx)
            torch.cuda.current_stream(x.device).wait_stream(side)
            self._bound_graph_cache()
            g = self._graphs[key] = {"graph": graph, "x": sx, "P": P, "bufs": bufs}
        g["x"].copy_(x)
        g["graph"].replay()
        return g["bufs"]

    def taylor(self, x: torch.Tensor, y: torch.Tensor, want: Optional[set] = None, arena=None, mode="taylor",
               criterion=None, loss_batch: Optional[int] = None):
        """One fused forward+backward (``criterion``: see :func:`logits_grad`); returns {block index: per-sample signed Taylor sums
        sum_hw -(dL/da * a)} (``mode="sensitivity"``: sum_hw |dL/da|) for every requested block
        (conv blocks first, then linear blocks; the final linear has none) as (R, B, C) partial
        slots for conv blocks (sum over R, or fold with ops.score_fold_) and (B, C) for linear
        blocks. Deterministic: no atomics."""
        tm = 1 if mode == "sensitivity" else 0
        T = ops.require()
        P = self._pack()
        nconv, nlin = len(self.plan.convs), len(self.plan.linears)
        if want is None:
            want = set(range(nconv + nlin - 1))
        if arena is None:
            arena = {b: torch.zeros(sh, device=x.device)
                     for b, sh in self._arena_shapes(x.shape[0], want, x.shape[2], x.shape[3]).items()}
        logits, saved = self.forward(x)
        B = logits.shape[0]
        g = logits_grad(logits, y, criterion, loss_batch)
        lin_acts = saved["lin_acts"]
        acts = saved["acts"]
        res = {}
        # classifier (dgrad of linear j produces the grad at its input = output of block j-1)
        e_last = P["lins"][-1]
        if e_last["pad"]:
            g = F.pad(g, (0, e_last["pad"]))  # one kernel (zeros + cat was two)
        g = g.reshape(B, 1, 1, -1).contiguous()
        for j in range(nlin - 1, -1, -1):
            e = P["lins"][j]
            act = lin_acts[j]  # input of linear j
            blk_index = nconv + j - 1  # the block whose output is `act`
            taylor = None
            if blk_index in want:
                taylor = arena[blk_index]
                res[blk_index] = taylor
            bn_scale = P["convs"][-1]["scale"] if j == 0 and nconv else None
            slope = P["lins"][j - 1]["slope"] if j > 0 else 0.0  # activation whose output is `act`
            want_out = j > 0 or nconv > 0  # the input of a conv-less chain needs no gradient
            if not want_out and taylor is None:
                break
            gg = g
            cfg, sp = TUNER.choose(("lin_bwd", tuple(g.shape), tuple(act.shape)), B, act.shape[3], e["wt"].shape[1],
                                   lambda c, s_, e=e, gg=gg, act=act, bn=bn_scale, sl=slope: T.conv_dgrad(
                                       gg, None, e["wt"], act, bn, None, True, 1, c, s_, slope=sl))
            g = T.conv_dgrad(g, None, e["wt"], act, bn_scale, taylor, want_out, 1, cfg, sp, tay_mode=tm, slope=slope)
        # conv stack: g is dL/d(pre-activation of conv nconv-1) * bn_scale, at the
        # (pooled, if pooled) output resolution of that block
        unpooled = False  # the previous data gradient already wrote g at full resolution
        for ci in range(nconv - 1, 0, -1):
            e = P["convs"][ci]
            prev_act = acts[ci - 1][0]
            _, am = acts[ci]
            if unpooled:
                am = None
            taylor = None
            if (ci - 1) in want:
                taylor = arena[ci - 1]
                res[ci - 1] = taylor
            H, W = prev_act.shape[1], prev_act.shape[2]
            M = B * H * W
            need_out = ci - 1 > 0
            sc_prev = P["convs"][ci - 1]["scale"]
            gg = g
            Cin, Cg = prev_act.shape[3], g.shape[3]
            wino = (B * (H // 2) * (W // 2), Cg) if "ut" in e and _wino_ok(H, W, Cg, Cin) else None
            sc4, cands = None, None
            if self.bf16 and Cg % 32 == 0:
                cands = self._bf16_cands(M, Cin, e["wt"].shape[1])
                if wino is not None:
                    cands = self._wino_bf_cands(T, B, H, W, Cin, Cg, am is not None) + cands
            elif H == 2 and W == 2 and Cg % 32 == 0 and Cin % 32 == 0:
                pe = P["convs"][ci - 1]
                sc4 = pe.get("scale4")
                if sc4 is None:
                    sc4 = pe["scale4"] = sc_prev.repeat(4).contiguous()
                # dense GEMM dgrad: one writer per Taylor element (deterministic as well)
                cands = [(self.DENSE + c, s_) for c, s_ in TUNER.candidates(B, 4 * Cin, 4 * Cg)] + \
                    TUNER.candidates(M, Cin, e["wt"].shape[1], wino, True) + self._fast2_cands(B, Cin, Cg)
            elif wino is not None and am is not None:
                wc = TUNER.candidates(M, Cin, e["wt"].shape[1], wino, True)
                wc = [c for c in wc if c[0] == WINO_LDS] + [c for c in wc if c[0] != WINO_LDS]
                unp = [(WINO_UNP, s_) for k, s_ in wc if k == WINO_LDS]
                # [0] = the untuned pick: explicit unpool from 16x16 down (measured faster at
                # B=2048 for the 16/8/4-pixel layers, slower at 32x32); bit-identical either way
                cands = unp + wc if H <= 16 else wc + unp
            if not self.bf16 and self.use_wino and _wino4_ok(H, W, Cg, Cin) and "w4d" in e and cands is None \
                    and wino is not None:
                cands = TUNER.candidates(M, Cin, e["wt"].shape[1], wino, True)
            if not self.bf16 and self.use_wino and _wino4_ok(H, W, Cg, Cin) and "w4d" in e and cands is not None:
                cands = _wino4_cands(B, H, W, Cin, Cg) + cands  # [0] = the untuned pick
            # the previous block pools: an F(4x4) data gradient in one K pass writes its output unpooled
            # through that pool's argmax (no separate unpooling pass: its read of the pooled
            # gradient and the second write are saved); other kernels hand the pooled gradient on
            unp = acts[ci - 1][1] if need_out and not self.bf16 else None
            if unp is not None and cands is not None and any(c[0] in (WINO4S, WINO4) for c in cands):
                cands = cands + [(WINO4S_FU, 1), (WINO4_FU, 1)]  # timed against unfused + explicit unpool

            def fuse(c, s_, unp=unp):
                return unp if c in _W4_FUSED else None

            def trial(c, s_, e=e, gg=gg, am=am, pa=prev_act, sc=sc_prev, no=need_out, s4=sc4, unp=unp):
                out = self._dgrad_run(T, e, gg, am, pa, sc, None, no, c, s_, s4, unp=fuse(c, s_))
                if unp is not None and c not in _W4_FUSED:
                    T.unpool2_nhwc(out, unp)  # the unpooling pass the next data gradient then runs
                return out

            cfg, sp = TUNER.choose(("bwd", tuple(g.shape), tuple(prev_act.shape), am is not None, wino is not None,
                                    self.bf16, unp is not None),
                                   M, Cin, e["wt"].shape[1], trial, wino, wino_only=True, cands=cands)
            g = self._dgrad_run(T, e, g, am, prev_act, sc_prev, taylor, need_out, cfg, sp, sc4, tm, unp=fuse(cfg, sp))
            unpooled = fuse(cfg, sp) is not None
        return res


KERNEL_FAMILIES = ("wino4", "wino4_fused", "wino4_m3", "wino2", "wino2_direct", "igemm", "wino2_bf16", "fast2x2")


def family_policy(family: str, split: str = "min"):
    """A :meth:`Autotuner.pinned` policy that runs every layer it can on one kernel family:
    ``wino4`` F(4x4,3x3) (split-points kernel), ``wino4_fused`` the same with the data gradients of
    pooled blocks unpooling in their epilogue, ``wino4_m3`` its MODE 3 kernel, ``wino2`` F(2x2,3x3) LDS-staged (+ explicit unpool), ``wino2_direct``
    F(2x2) with direct patch loads, ``igemm`` the implicit GEMM (dense 2x2 GEMM, VALU first
    layer; with bf16 operands the bf16 implicit GEMM), ``wino2_bf16`` the bf16 F(2x2) kernels
    (compute_dtype=bfloat16 only), ``fast2x2`` the nine-product kernels of the 2x2-map layers
    (conv2x2_fast.hip). ``split``: the fewest ("min") or most ("max") channel splits of
    that family. Layers the family does not cover keep the untuned pick."""
    eng = FusedChainEngine

    def member(c):
        k = c[0]
        if family == "wino4":
            return k == WINO4S
        if family == "wino4_fused":  # the split-points kernel, data gradients unpooling in their epilogue
            return k in (WINO4S_FU, WINO4S)
        if family == "wino4_m3":
            return k == WINO4
        if family == "wino2":
            return k in (WINO_LDS, WINO_UNP)
        if family == "wino2_direct":
            return k == WINO
        if family == "igemm":
            return 0 <= k <= 6 or eng.DENSE <= k < FAST2 or CFG_BF16 <= k or k == eng.FIRST_DIRECT
        if family == "fast2x2":
            return FAST2 <= k < FAST2 + 7
        if family == "wino2_bf16":
            return k in (WINO_BF, WINO_BF_UNP)
        raise ValueError(f"unknown kernel family {family!r}")

    def policy(key, cands, M, N, K):
        hit = [c for c in cands if member(c)]
        if not hit and family == "igemm" and key[0] == "bwd":
            return _pick_cfg(M, N, K)  # dgrad lists hold the Winograd kinds only
        if not hit:
            return None
        if family == "wino4_fused" and any(c[0] == WINO4S_FU for c in hit):
            return (WINO4S_FU, 1)
        return (min if split == "min" else max)(hit, key=lambda c: c[1])

    return policy


def logits_grad(logits: torch.Tensor, y: torch.Tensor, criterion=None, loss_batch: Optional[int] = None) -> torch.Tensor:
    """dL/dlogits of the batch loss the engines back-propagate: the fused HIP log-softmax + NLL
    kernel for mean cross-entropy (``criterion=None``), else autograd through the user's
    criterion on the (detached) logits, with its default reduction — exactly the gradient the
    reference's ``criterion(out, y).backward()`` feeds into the network (attributions.py:64-68).
    ``loss_batch``: the mean is over batches of this size (coalesced loader batches, cross-entropy
    only): every sample's gradient is what its own loader batch's backward gives it."""
    if criterion is None:
        return ops.cross_entropy(logits, y, 1.0 / (loss_batch or logits.shape[0]), True)[1]
    assert loss_batch is None or loss_batch == logits.shape[0], "coalesced batches need the fused cross-entropy"
    lg = logits.detach().requires_grad_(True)
    with torch.enable_grad():
        loss = criterion(lg, y)
    return torch.autograd.grad(loss, lg)[0].float().contiguous()


def per_sample_loss(logits: torch.Tensor, y: torch.Tensor, criterion=None) -> torch.Tensor:
    """Per-sample losses (B,) of ``criterion(out, y, reduction="none")`` (attributions.py:50,87),
    trailing dims summed as on the generic path; the fused HIP cross-entropy for ``None``."""
    if criterion is None:
        return ops.cross_entropy(logits, y, 1.0, False)[0]
    with torch.no_grad():
        loss = criterion(logits, y, reduction="none")
    return loss.reshape(logits.shape[0], -1).sum(-1).float()


def engine_criterion(criterion, device):
    """``None`` (the fused cross-entropy) when ``criterion`` is plain mean cross-entropy, else the
    criterion itself (engines then differentiate it with autograd on the logits)."""
    return None if criterion is None or criterion_is_cross_entropy(criterion, device) else criterion


def criterion_is_cross_entropy(criterion, device) -> bool:
    """Numerically probe whether ``criterion(out, y[, reduction])`` is plain mean cross-entropy.

    The probe uses in-range labels only, so ``F.cross_entropy`` itself passes it and runs on the fused
    kernel, which does not implement ``ignore_index``: a label outside ``[0, classes)`` (``-100``
    included) gives a NaN loss and a NaN gradient row there (``ops.cross_entropy``)."""
    try:
        g = torch.Generator(device="cpu").manual_seed(1234)
        logits = (torch.randn(6, 5, generator=g) * 2).to(device)
        y = torch.randint(0, 5, (6,), generator=g).to(device)
        ref = F.cross_entropy(logits, y)
        got = criterion(logits, y)
        return bool(torch.allclose(got.float(), ref.float(), rtol=1e-5, atol=1e-6))
    except Exception:
        return False


def engines_enabled() -> bool:
    """``TORCHPRUNER_ENGINES=0`` sends every metric to the generic module/hook path (the
    same-algorithm library baseline of bench.py: one pass, PyTorch modules; add
    ``TORCHPRUNER_GENERIC_NATIVE=0`` for MIOpen / hipBLASLt convolutions)."""
    return os.environ.get("TORCHPRUNER_ENGINES", "1") != "0"


def _reject(why, reason):
    """Record why an engine did not apply (path transparency) and return None."""
    if why is not None:
        why.append(reason)
    return None


def maybe_engine(model, eval_modules, criterion, device, need_ce=True, why=None, pre_act_ok=False,
                 input_shape=None):
    """Return (engine, block indices of eval_modules) when the fused path applies, else None.
    ``need_ce=False``: forward-only use (APoZ) or gradient metrics with any criterion (the caller
    passes ``engine_criterion(criterion)`` to :meth:`FusedChainEngine.taylor`). ``why``: a list that receives the
    rejection reason when the engine does not apply. ``pre_act_ok``: a classifier block's Linear
    may stand for its activation output (valid for sign counts (APoZ) and zero-masking
    (Shapley): ReLU / LeakyReLU keep the sign and map 0 to 0; not for Taylor / Sensitivity).
    ``input_shape``: shape of a data batch; an input the chain does not compute on (e.g. a
    (B, T, F) batch for a Linear MLP) rejects the engine."""
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if dev.type != "cuda":
        return _reject(why, f"device {dev} is not a GPU")
    if ops.backend() == "torch":
        return _reject(why, "native extension disabled (TORCHPRUNER_BACKEND=torch)")
    if not ops.available():
        from ..ops import _native
        return _reject(why, f"native extension failed to load: {_native.load_error()!r}")
    if not engines_enabled():
        return _reject(why, "fused engines disabled (TORCHPRUNER_ENGINES=0)")
    if model.training:
        return _reject(why, "model is in training mode (engines fold eval-mode BatchNorm)")
    if any(p.dtype != torch.float32 for p in model.parameters()):
        return _reject(why, "parameters are not float32")
    plan, reason = build_plan(model)
    if plan is None:
        return _reject(why, f"fused chain: {reason}")
    if input_shape is not None:
        err = plan.input_error(input_shape)
        if err:
            return _reject(why, f"fused chain: {err}")
    idx = []
    blocks = plan.blocks
    for m in eval_modules:
        found = None
        for k, b in enumerate(blocks[:-1]):
            if b.relu is m or (pre_act_ok and isinstance(b, LinearBlock) and b.linear is m):
                found = k
                break
        if found is None:
            return _reject(why, f"fused chain: evaluation module {type(m).__name__} is not a block activation "
                                "(use find_best_evaluation_module=True)")
        idx.append(found)
    if need_ce and not criterion_is_cross_entropy(criterion, dev):
        return _reject(why, "criterion is not mean cross-entropy")
    eng = _ENGINES.get(model)
    if eng is None or len(eng.plan.blocks) != len(plan.blocks) or any(
            (a.conv is not b.conv if isinstance(a, ConvBlock) else a.linear is not b.linear) or a.width != b.width
            for a, b in zip(eng.plan.blocks, plan.blocks)):
        eng = FusedChainEngine(model, plan)
        _ENGINES[model] = eng
    eng.bf16 = False  # exact fp32 unless the caller opts in (AttributionMetric compute_dtype=bfloat16)
    return eng, idx


_ENGINES: "weakref.WeakKeyDictionary[nn.Module, FusedChainEngine]" = weakref.WeakKeyDictionary()
