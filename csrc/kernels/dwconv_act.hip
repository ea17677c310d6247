// Depthwise convolutions of the attribution path (eval mode), fp32 NHWC, with the activations on
// both sides and the BN affine fused, so a MobileNet inverted-residual block's hidden activation is
// read once and written once per pass:
//
//   forward  y  = out_act(scale[c] * dwconv(in_act(x))[c] + shift[c])   (+ APoZ counts of y > 0)
//   dgrad    dA = gather(mask_out(y) * g * scale[c])                    (dL/d in_act(z), unmasked)
//            tay[slot, b, c] = sum over the block's pixels of -(dA * a) or |dA|, a = in_act(z)
//            dz = mask_in(z) * dA
//
// Activation codes are bn_train_fwd's: 0 none, 1 ReLU, 2 ReLU6. The score partials are reduced
// from the UNMASKED dA: a saturated unit (a == 6) contributes 6 * dA to Taylor and |dA| to
// Sensitivity although its gradient stops there (the scored module is the activation's output).
// Masks follow hardtanh_backward: the gradient is zero at exactly 0 and exactly 6.
//
// The tp_dwconv_hs_* entry points add code 3, Hardswish hs(v) = v * min(max(v + 3, 0), 6) / 6
// (MobileNetV3), on either side. Hardswish is not monotonic, so its derivative d(v) (0 if v < -3,
// v / 3 + 0.5 if v <= 3, else 1: ATen's branch order) cannot be read from the stored output: the
// forward optionally stores the pre-activation v of the output next to y (`pre`), and the dgrad
// takes that as its y operand when out_act == 3. The masks become factors:
//
//   dgrad    dA = gather(g * scale[c] * d_out),  dz = dA * d_in(z)       (partials from dA as above)
//
// with d the 0/1 mask for codes 0..2. These kernels are the HS = true instantiations of the same
// templates; a call without a code 3 and without `pre` runs the HS = false one, which is the code
// of the tp_dwconv_act_* entry points unchanged.
//
// Geometry is dwconv.hip's float4 path (C % 4 == 0 only: the engine pads channels; padded channels
// carry zero weights and a zero affine, so their y, dz and partials are exact zeros for any finite
// input): one block per (image row, 256-wide slice of the row's strips x channel quads), a thread
// owns a quad and a strip of DW_SW columns. k in {3, 5}, stride in {1, 2}, pad 0..k-1, every
// operand below 2^31 bytes. The activations reach the kernels as clamp bounds (DwAct), so one
// instantiation serves every pair without a branch.
//
// Score partials: the threads of a block that share a channel quad (the strips of the slice) are
// summed in strip order through the LDS after each thread summed its columns in order; the block
// stores the result into its own slot (row of the image x slice) of the (R, B, C) slab: one writer
// per element, a slot never mixes images, no float atomics, bit-identical from run to run. The
// caller passes a zeroed slab (with more than 256 quads per pixel a block covers only part of the
// channels of its slot) and sums the slots. APoZ counts are integers, added with float atomics
// after the same block reduction (exact and order independent up to 2^24).
#include "tp_dwconv.h"
#include "tp_launchers.h"

#include <initializer_list>

namespace tp {

// An activation as its clamp bounds: none, ReLU (0, .), ReLU6 (0, 6). lo / hi are the bounds of the
// gradient mask with NaN for "unbounded on that side" (a comparison with NaN is false), clo / chi the
// same bounds for the clamp with -inf / +inf there. Everything below is branch-free in the code
// (selects only), so one instantiation serves every pair of activations.
struct DwAct {
  float lo, hi, clo, chi;
  int hs;  // Hardswish (read by the HS instantiations only; the bounds are then "none")
};
// NaN-propagating activation (torch.clamp / nan_relu semantics): IEEE 754-2019 maximum / minimum
// (v_maximum3_f32 / v_minimum3_f32 on gfx950) return NaN for a NaN operand
__device__ __forceinline__ float dwa_act(DwAct a, float x) {
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(x, a.clo), a.chi);
}
// d act / d x given a value v with the sign / saturation of the pre-activation (the stored clamped
// output works as well): hardtanh_backward / threshold_backward zero the gradient where v <= lo or
// v >= hi and pass it everywhere else (a comparison with a NaN bound is false)
__device__ __forceinline__ bool dwa_live(DwAct a, float v) { return !(v <= a.lo) && !(v >= a.hi); }
// The same two with Hardswish as a further activation, selected by a.hs (a wave-uniform select,
// no branch). hs(v) is NaN for a NaN v (and for -inf, as ATen's expression is); its derivative has
// the branch order of ATen's hardswish_backward (a NaN v passes the gradient).
template <bool HS>
__device__ __forceinline__ float dwa_apply(DwAct a, float x) {
  const float c = dwa_act(a, x);
  if constexpr (!HS) return c;
  // x * clamp(x / 6 + 0.5, 0, 1): no division (the forward activates every loaded tap), within an
  // ulp or two of ATen's x * clamp(x + 3, 0, 6) / 6
  const float r = fmaf(x, 1.f / 6.f, 0.5f);
  return a.hs ? x * __builtin_elementwise_minimum(__builtin_elementwise_maximum(r, 0.f), 1.f) : c;
}
// d act / d x as a factor: the 0 / 1 mask of dwa_live, or Hardswish's derivative of the pre-activation v
__device__ __forceinline__ float dwa_slope(DwAct a, float v) {
  const float m = dwa_live(a, v) ? 1.f : 0.f;
  const float d = v < -3.f ? 0.f : v <= 3.f ? fmaf(v, 1.f / 3.f, 0.5f) : 1.f;
  return a.hs ? d : m;
}

// Sum of the 4-channel values of the threads that share a channel quad (threads t, t + CV, ... of
// the block, strip order) -> thread t < min(CV, 256); `mine` is zero for threads past nq
__device__ __forceinline__ bool dwa_block_fold(float (*red)[4], const float* mine, int CV, float* out) {
  DwVec<4>::store(red[threadIdx.x], mine);
  __syncthreads();
  if ((int)threadIdx.x >= CV) return false;
#pragma unroll
  for (int v = 0; v < 4; ++v) out[v] = 0.f;
#pragma unroll 4
  for (int t = threadIdx.x; t < 256; t += CV) {
    float r[4];
    DwVec<4>::load(red[t], r);
#pragma unroll
    for (int v = 0; v < 4; ++v) out[v] += r[v];
  }
  return true;
}

template <int K, int S, bool APOZ, bool HS>
__global__ __launch_bounds__(256) void dwconv_act_fwd_k(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ y,
                                                        float* __restrict__ apoz, float* __restrict__ pre, int H,
                                                        int W, int C, int pad, int Ho, int Wo, int cpr, FastDiv dcv,
                                                        int nq, DwAct in_act, DwAct out_act) {
  constexpr int KK = K * K, NIN = (DW_SW - 1) * S + K;
  const int CV = C / 4;
  const int row = blockIdx.x / cpr, chunk = blockIdx.x - row * cpr;  // row = b * Ho + oh
  const int q = chunk * 256 + threadIdx.x;
  const bool valid = q < nq;
  if (!APOZ && !valid) return;
  const int strip = dcv.div(q), c = (q - strip * CV) * 4;
  const int b = row / Ho, oh = row - b * Ho;
  float cnt[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid) {
    const int ow0 = strip * DW_SW, ih0 = oh * S - pad, iw0 = ow0 * S - pad;
    float* yr = y + row * Wo * C + c;
    float wf[4 * KK];
    dw_load_w<4, KK>(w, c, wf);
    float acc[DW_SW][4];
#pragma unroll
    for (int j = 0; j < DW_SW; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[j][v] = 0.f;
#pragma unroll
    for (int kh = 0; kh < K; ++kh) {
      const int ih = ih0 + kh;
      if (ih < 0 || ih >= H) continue;  // block-uniform
      const float* xr = x + (b * H + ih) * W * C + c;
      float in[NIN][4];
#pragma unroll
      for (int i = 0; i < NIN; ++i) {
        const int iw = iw0 + i;
#pragma unroll
        for (int v = 0; v < 4; ++v) in[i][v] = 0.f;
        if (iw >= 0 && iw < W) {  // zero padding is applied after the activation: act(0) == 0 anyway
          DwVec<4>::load(xr + iw * C, in[i]);
#pragma unroll
          for (int v = 0; v < 4; ++v) in[i][v] = dwa_apply<HS>(in_act, in[i][v]);
        }
      }
#pragma unroll
      for (int j = 0; j < DW_SW; ++j)
#pragma unroll
        for (int kw = 0; kw < K; ++kw)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[j][v] = fmaf(in[j * S + kw][v], wf[v * KK + kh * K + kw], acc[j][v]);
    }
    float sc[4], sh[4];
    DwVec<4>::load(scale + c, sc);
    DwVec<4>::load(shift + c, sh);
#pragma unroll
    for (int j = 0; j < DW_SW; ++j) {
      if (ow0 + j >= Wo) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[j][v] = fmaf(sc[v], acc[j][v], sh[v]);
      if constexpr (HS)
        if (pre != nullptr) DwVec<4>::store(pre + row * Wo * C + c + (ow0 + j) * C, acc[j]);  // block-uniform
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        acc[j][v] = dwa_apply<HS>(out_act, acc[j][v]);
        if (APOZ) cnt[v] += acc[j][v] > 0.f ? 1.f : 0.f;
      }
      DwVec<4>::store(yr + (ow0 + j) * C, acc[j]);
    }
  }
  if constexpr (APOZ) {
    __shared__ float red[256][4];
    float tot[4];
    if (!dwa_block_fold(red, cnt, CV, tot)) return;
    float* ap = apoz + b * C + c;  // c: this thread's quad, valid or not
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (tot[v] != 0.f) atomicAdd(ap + v, tot[v]);
  }
}

// Gather form of dwconv_dgrad_k (same strips, taps and column range) with the output activation's
// mask and the BN scale applied to g as it is loaded, and the input activation's mask applied to
// the result after the score partials were taken from it. HS: the masks are factors (dwa_slope) and
// y holds the output's pre-activation where out_act is Hardswish; a zero factor still gives an exact
// zero whatever g or dA is, as the masks do.
template <int K, int S, int PB, bool TAY, bool HS>
__global__ __launch_bounds__(256) void dwconv_act_dgrad_k(const float* __restrict__ g, const float* __restrict__ y,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ z, float* __restrict__ dz,
                                                          float* __restrict__ tay, int Bn, int H, int W, int C,
                                                          int pad, int Ho, int Wo, int cpr, FastDiv dcv, int nq,
                                                          DwAct in_act, DwAct out_act, int use_y, int tay_mode) {
  constexpr int KK = K * K, DMIN = DwTaps<K, S, PB>::lo(), ND = DwTaps<K, S, PB>::hi() - DMIN + 1;
  const int CV = C / 4;
  const int row = blockIdx.x / cpr, chunk = blockIdx.x - row * cpr;  // row = b * H + ih
  const int q = chunk * 256 + threadIdx.x;
  const bool valid = q < nq;
  if (!TAY && !valid) return;
  const int strip = dcv.div(q), c = (q - strip * CV) * 4;
  const int b = row / H, ih = row - b * H;
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid) {
    const int iw0 = strip * DW_SW;
    const int ow_lo = (iw0 + pad - PB) / S + DMIN;  // exact division: (iw0 + pad) % S == PB
    float wf[4 * KK], sc[4];
    dw_load_w<4, KK>(w, c, wf);
    DwVec<4>::load(scale + c, sc);
    float acc[DW_SW][4];
#pragma unroll
    for (int j = 0; j < DW_SW; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[j][v] = 0.f;
#pragma unroll
    for (int kh = 0; kh < K; ++kh) {
      const int n = ih + pad - kh;  // block-uniform row tests
      if (n < 0 || (S == 2 && (n & 1))) continue;
      const int oh = n / S;
      if (oh >= Ho) continue;
      const int ro = (b * Ho + oh) * Wo * C + c;
      float gv[ND][4];
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const int ow = ow_lo + d;
#pragma unroll
        for (int v = 0; v < 4; ++v) gv[d][v] = 0.f;
        if (ow >= 0 && ow < Wo) {
          float yv[4] = {1.f, 1.f, 1.f, 1.f};  // without an output activation y is not read: any live value
          DwVec<4>::load(g + ro + ow * C, gv[d]);
          if (use_y) DwVec<4>::load(y + ro + ow * C, yv);  // block-uniform
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            if constexpr (HS) {
              const float f = dwa_slope(out_act, yv[v]);
              gv[d][v] = f != 0.f ? gv[d][v] * sc[v] * f : 0.f;
            } else {
              gv[d][v] = dwa_live(out_act, yv[v]) ? gv[d][v] * sc[v] : 0.f;
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < DW_SW; ++j)
#pragma unroll
        for (int kw = 0; kw < K; ++kw)
          if ((PB + j - kw) % S == 0) {
#pragma unroll
            for (int v = 0; v < 4; ++v)
              acc[j][v] = fmaf(gv[(PB + j - kw) / S - DMIN][v], wf[v * KK + kh * K + kw], acc[j][v]);
          }
    }
    const int zo = row * W * C + c;
#pragma unroll
    for (int j = 0; j < DW_SW; ++j) {
      if (iw0 + j >= W) continue;
      float zv[4];
      DwVec<4>::load(z + zo + (iw0 + j) * C, zv);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (TAY) part[v] += tay_term(tay_mode, acc[j][v], dwa_apply<HS>(in_act, zv[v]));
        if constexpr (HS) {
          const float f = dwa_slope(in_act, zv[v]);
          acc[j][v] = f != 0.f ? acc[j][v] * f : 0.f;
        } else {
          acc[j][v] = dwa_live(in_act, zv[v]) ? acc[j][v] : 0.f;
        }
      }
      DwVec<4>::store(dz + zo + (iw0 + j) * C, acc[j]);
    }
  }
  if constexpr (TAY) {
    __shared__ float red[256][4];
    float tot[4];
    if (!dwa_block_fold(red, part, CV, tot)) return;
    DwVec<4>::store(tay + ((ih * cpr + chunk) * Bn + b) * C + c, tot);  // c: the quad, valid or not
  }
}

static bool dwa_acts_ok(int in_act, int out_act, int last) {
  return in_act >= 0 && in_act <= last && out_act >= 0 && out_act <= last;
}

static DwAct dwa_bounds(int act) {
  const float none = __builtin_nanf(""), inf = __builtin_inff();
  return DwAct{act == 1 || act == 2 ? 0.f : none, act == 2 ? 6.f : none, act == 1 || act == 2 ? 0.f : -inf,
               act == 2 ? 6.f : inf, act == 3};
}

static bool dwa_all_aligned(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

static int dwa_tay_slots(int H, int W, int C) {
  if (H < 1 || W < 1 || C < 4 || C % 4 != 0) return 0;
  const long long q = (long long)ceil_div(W, DW_SW) * (C / 4);
  const long long per = (q + 255) / 256;  // below 2^53: no overflow in the product with H < 2^31
  if (per >= (1ll << 24)) return 0;
  const long long r = (long long)H * per;
  return r < (1ll << 24) ? (int)r : 0;
}

// Both forward entry points: codes 0..last; `pre` (Hardswish entry point only) takes the HS kernels
static hipError_t dwa_fwd(const float* x, const float* w, const float* scale, const float* shift, float* y,
                          float* apoz, float* pre, int B, int H, int W, int C, int k, int s, int pad, int in_act,
                          int out_act, int last, hipStream_t st) {
  int Ho, Wo, cpr, nq;
  long long blocks;
  if (C < 4 || C % 4 != 0 || !dwa_acts_ok(in_act, out_act, last) || !dw_geometry(B, H, W, C, k, s, pad, &Ho, &Wo))
    return hipErrorInvalidValue;
  if (x == nullptr || w == nullptr || scale == nullptr || shift == nullptr || y == nullptr ||
      !dwa_all_aligned({x, w, scale, shift, y, apoz, pre}))
    return hipErrorInvalidValue;
  if (!dw_row_grid(B * Ho, Wo, C, 4, &cpr, &nq, &blocks)) return hipErrorInvalidValue;
  const FastDiv dcv((unsigned)(C / 4));
  const bool hs = in_act == 3 || out_act == 3 || pre != nullptr;
#define TP_DWA_FWD(K_, S_, AP_, HS_)                                                                             \
  dwconv_act_fwd_k<K_, S_, AP_, HS_><<<(unsigned)blocks, 256, 0, st>>>(x, w, scale, shift, y, apoz, pre, H, W, C, \
                                                                       pad, Ho, Wo, cpr, dcv, nq,                 \
                                                                       dwa_bounds(in_act), dwa_bounds(out_act))
  if (hs) {
    if (apoz != nullptr) TP_DW_KS(TP_DWA_FWD, true, true);
    else TP_DW_KS(TP_DWA_FWD, false, true);
  } else {
    if (apoz != nullptr) TP_DW_KS(TP_DWA_FWD, true, false);
    else TP_DW_KS(TP_DWA_FWD, false, false);
  }
#undef TP_DWA_FWD
  return hipGetLastError();
}

static hipError_t dwa_dgrad(const float* g, const float* y, const float* w, const float* scale, const float* z,
                            float* dz, float* tay, int R, int tay_mode, int B, int H, int W, int C, int k, int s,
                            int pad, int in_act, int out_act, int last, hipStream_t st) {
  int Ho, Wo, cpr, nq;
  long long blocks;
  if (C < 4 || C % 4 != 0 || !dwa_acts_ok(in_act, out_act, last) || !dw_geometry(B, H, W, C, k, s, pad, &Ho, &Wo))
    return hipErrorInvalidValue;
  if (g == nullptr || w == nullptr || scale == nullptr || z == nullptr || dz == nullptr ||
      (out_act != 0 && y == nullptr) || !dwa_all_aligned({g, y, w, scale, z, dz, tay}))
    return hipErrorInvalidValue;
  if (!dw_row_grid(B * H, W, C, 4, &cpr, &nq, &blocks)) return hipErrorInvalidValue;
  if (tay != nullptr) {
    long long nt = 1;
    if (tay_mode < 0 || tay_mode > 1 || R < 1 || R != dwa_tay_slots(H, W, C)) return hipErrorInvalidValue;
    if (!(dw_grow(nt, R) && dw_grow(nt, B) && dw_grow(nt, C))) return hipErrorInvalidValue;
  }
  const FastDiv dcv((unsigned)(C / 4));
  const int pb = pad % s;  // parity of iw0 + pad (strips start at multiples of 4)
  const DwAct ia = dwa_bounds(in_act), oa = dwa_bounds(out_act);
  const bool hs = in_act == 3 || out_act == 3;
#define TP_DWA_DG(K_, S_, TAY_, HS_)                                                                                \
  do {                                                                                                              \
    if (S_ == 2 && pb == 1)                                                                                         \
      dwconv_act_dgrad_k<K_, S_, S_ - 1, TAY_, HS_><<<(unsigned)blocks, 256, 0, st>>>(                              \
          g, y, w, scale, z, dz, tay, B, H, W, C, pad, Ho, Wo, cpr, dcv, nq, ia, oa, out_act != 0, tay_mode);        \
    else                                                                                                            \
      dwconv_act_dgrad_k<K_, S_, 0, TAY_, HS_><<<(unsigned)blocks, 256, 0, st>>>(                                   \
          g, y, w, scale, z, dz, tay, B, H, W, C, pad, Ho, Wo, cpr, dcv, nq, ia, oa, out_act != 0, tay_mode);        \
  } while (0)
  if (hs) {
    if (tay != nullptr) TP_DW_KS(TP_DWA_DG, true, true);
    else TP_DW_KS(TP_DWA_DG, false, true);
  } else {
    if (tay != nullptr) TP_DW_KS(TP_DWA_DG, true, false);
    else TP_DW_KS(TP_DWA_DG, false, false);
  }
#undef TP_DWA_DG
  return hipGetLastError();
}

}  // namespace tp

// y = out_act(scale * dwconv(in_act(x)) + shift): x (B, H, W, C), w (C, 1, k, k), scale / shift (C),
// y (B, Ho, Wo, C); apoz (optional, (B, C)) += count(y > 0). C % 4 == 0.
extern "C" hipError_t tp_dwconv_act_fwd(const float* x, const float* w, const float* scale, const float* shift,
                                        float* y, float* apoz, int B, int H, int W, int C, int k, int s, int pad,
                                        int in_act, int out_act, hipStream_t st) {
  return tp::dwa_fwd(x, w, scale, shift, y, apoz, nullptr, B, H, W, C, k, s, pad, in_act, out_act, 2, st);
}

// Slots R of the (R, B, C) score-partial slab of tp_dwconv_act_dgrad for (H, W, C) inputs: one per
// (input row, 256-wide slice of the row's strips x channel quads); 0 for shapes the kernel rejects
extern "C" int tp_dwconv_act_tay_slots(int H, int W, int C) { return tp::dwa_tay_slots(H, W, C); }

// dz (B, H, W, C) from g / y (B, Ho, Wo, C) (g unmasked, y the stored forward output), w, scale and
// the forward input z; tay (optional): a zeroed (R, B, C) slab, R = tp_dwconv_act_tay_slots(H, W, C),
// tay_mode 0 Taylor -(dA * a), 1 Sensitivity |dA|
extern "C" hipError_t tp_dwconv_act_dgrad(const float* g, const float* y, const float* w, const float* scale,
                                          const float* z, float* dz, float* tay, int R, int tay_mode, int B, int H,
                                          int W, int C, int k, int s, int pad, int in_act, int out_act,
                                          hipStream_t st) {
  return tp::dwa_dgrad(g, y, w, scale, z, dz, tay, R, tay_mode, B, H, W, C, k, s, pad, in_act, out_act, 2, st);
}

// The same three with activation code 3 (Hardswish) allowed on either side. pre (optional, the shape
// of y) receives the output's pre-activation scale * dwconv(in_act(x)) + shift in the same pass.
extern "C" hipError_t tp_dwconv_hs_fwd(const float* x, const float* w, const float* scale, const float* shift,
                                       float* y, float* apoz, float* pre, int B, int H, int W, int C, int k, int s,
                                       int pad, int in_act, int out_act, hipStream_t st) {
  return tp::dwa_fwd(x, w, scale, shift, y, apoz, pre, B, H, W, C, k, s, pad, in_act, out_act, 3, st);
}

extern "C" int tp_dwconv_hs_tay_slots(int H, int W, int C) { return tp::dwa_tay_slots(H, W, C); }

// y: the stored forward output for out_act 1 / 2, the stored pre-activation (`pre`) for out_act 3
extern "C" hipError_t tp_dwconv_hs_dgrad(const float* g, const float* y, const float* w, const float* scale,
                                         const float* z, float* dz, float* tay, int R, int tay_mode, int B, int H,
                                         int W, int C, int k, int s, int pad, int in_act, int out_act,
                                         hipStream_t st) {
  return tp::dwa_dgrad(g, y, w, scale, z, dz, tay, R, tay_mode, B, H, W, C, k, s, pad, in_act, out_act, 3, st);
}
