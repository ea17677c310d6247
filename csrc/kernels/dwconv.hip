// Depthwise convolutions (depth multiplier 1: groups == Cin == Cout) of the training path, fp32
// NHWC: forward, input gradient and weight (+ bias) gradient for square k in {3, 5}, stride in
// {1, 2}, zero padding 0..k-1 and ANY channel count (pruned widths such as 67 or 103 are the
// normal case): a float4 path when C % 4 == 0 and a per-element path otherwise, as batchnorm.hip.
// These layers are memory-bound stencils (k*k MACs per element): no MFMA, no tuner, no weight
// pack. The weights are read from the parameter in place ((C, 1, k, k): a channel's k*k taps are
// contiguous) by the thread that owns the channel quad, as float4 loads, and held in registers in
// that channel-major order (wf[v * k*k + tap]; every index is a compile-time constant after
// unrolling, so the order costs nothing and no transposed staging copy is made).
//
// forward / dgrad: one block per (image row, 256-wide slice of the row's strips x channel vectors).
// The row is block-uniform and the per-thread index math is 32-bit (see the max-pool backward in
// train_ops.hip). A thread owns one channel vector and a strip of DW_SW consecutive columns, so the
// overlapping columns of neighbouring windows are loaded once; consecutive lanes take consecutive
// channel vectors (full float4 accesses, contiguous across the wave).
// wgrad: grid (channel slice of up to 64 channels x chunk of output-row strips); every block
// reduces its chunk in a fixed order (registers, then LDS) into one fp64 partial row
// [chunk][k*k + 1][C] (the last row is the bias gradient); a second kernel folds the chunks in a
// fixed order and writes dW with the parameter's own strides. No atomics anywhere: every result
// is deterministic.
//
// Carried widths (CARRY): the activations of a pruned block flow at a padded width C (a multiple of
// 4) while the parameter has Cw < C channels. The float4 kernels then read x / g / y / dx at pitch
// C; a quad wholly past Cw loads nothing and stores exact zeros, the quad that straddles Cw loads
// its weights and bias per channel (guarded, zeros past Cw: a float4 load would run past the end of
// the parameter) and stores exact zeros in its padding lanes whatever the inputs hold there; the
// weight gradient reduces and writes the channels below Cw only.
#include "tp_dwconv.h"
#include "tp_launchers.h"

namespace tp {

// dw_load_w for the quad that straddles Cw: per-channel loads, zero weights for c + v >= Cw
template <int KK>
__device__ __forceinline__ void dw_load_w_edge(const float* __restrict__ w, int c, int Cw, float* wf) {
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int i = 0; i < KK; ++i) wf[v * KK + i] = c + v < Cw ? w[(c + v) * KK + i] : 0.f;
}

// exact zeros for a strip's quad (the padding quads of a carried width)
__device__ __forceinline__ void dw_store_zeros(float* p, int col0, int cols, int C) {
  const float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < DW_SW; ++j)
    if (col0 + j < cols) DwVec<4>::store(p + (col0 + j) * C, z);
}

// y[b, oh, ow, c] = bias[c] + sum_{kh, kw} x[b, oh*S - pad + kh, ow*S - pad + kw, c] * w[c, kh, kw]
template <int K, int S, int V, bool CARRY = false>
__global__ __launch_bounds__(256) void dwconv_fwd_k(const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ y, int H,
                                                    int W, int C, int pad, int Ho, int Wo, int cpr, FastDiv dcv,
                                                    int nq, int Cw = 0) {
  static_assert(!CARRY || V == 4, "carried widths run on the float4 path");
  constexpr int KK = K * K, NIN = (DW_SW - 1) * S + K;
  const int row = blockIdx.x / cpr, chunk = blockIdx.x - row * cpr;  // row = b * Ho + oh
  const int q = chunk * 256 + threadIdx.x;
  if (q >= nq) return;
  const int strip = dcv.div(q), c = (q - strip * (C / V)) * V;
  const int b = row / Ho, oh = row - b * Ho;
  const int ow0 = strip * DW_SW, ih0 = oh * S - pad, iw0 = ow0 * S - pad;
  float* yr = y + row * Wo * C + c;
  bool edge = false;  // the quad straddles Cw
  if constexpr (CARRY) {
    if (c >= Cw) {
      dw_store_zeros(yr, ow0, Wo, C);
      return;
    }
    edge = c + 4 > Cw;
  }
  float wf[V * KK];
  if constexpr (CARRY) {
    if (edge) dw_load_w_edge<KK>(w, c, Cw, wf);
    else dw_load_w<V, KK>(w, c, wf);
  } else {
    dw_load_w<V, KK>(w, c, wf);
  }
  float acc[DW_SW][V];
  {
    float bv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) bv[v] = 0.f;
    if (bias != nullptr) {
      if (edge) {
#pragma unroll
        for (int v = 0; v < V; ++v) bv[v] = c + v < Cw ? bias[c + v] : 0.f;
      } else {
        DwVec<V>::load(bias + c, bv);
      }
    }
#pragma unroll
    for (int j = 0; j < DW_SW; ++j)
#pragma unroll
      for (int v = 0; v < V; ++v) acc[j][v] = bv[v];
  }
#pragma unroll
  for (int kh = 0; kh < K; ++kh) {
    const int ih = ih0 + kh;
    if (ih < 0 || ih >= H) continue;  // block-uniform
    const float* xr = x + (b * H + ih) * W * C + c;
    float in[NIN][V];
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      const int iw = iw0 + i;
#pragma unroll
      for (int v = 0; v < V; ++v) in[i][v] = 0.f;
      if (iw >= 0 && iw < W) DwVec<V>::load(xr + iw * C, in[i]);
    }
#pragma unroll
    for (int j = 0; j < DW_SW; ++j)
#pragma unroll
      for (int kw = 0; kw < K; ++kw)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[j][v] = fmaf(in[j * S + kw][v], wf[v * KK + kh * K + kw], acc[j][v]);
  }
  if constexpr (CARRY) {
    if (edge) {  // exact zeros in the padding lanes, whatever x holds there (0 * inf would be NaN)
#pragma unroll
      for (int j = 0; j < DW_SW; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[j][v] = c + v < Cw ? acc[j][v] : 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < DW_SW; ++j)
    if (ow0 + j < Wo) DwVec<V>::store(yr + (ow0 + j) * C, acc[j]);
}

// Input gradient as a gather: dx[b, ih, iw, c] = sum over the windows that contain the pixel of
// g[b, oh, ow, c] * w[c, kh, kw], kh then kw ascending, with oh = (ih + pad - kh) / S and
// ow = (iw + pad - kw) / S where the divisions are exact (stride 2: only the taps of the matching
// parity are visited). A strip starts at a multiple of 4 columns, so (iw0 + pad) % S == PB for
// every thread: the g columns a strip needs are ow = (iw0 + pad - PB) / S + d for the
// compile-time range d in [DMIN, DMAX]. Pixels no window covers get exact zeros.
template <int K, int S, int PB, int V, bool CARRY = false>
__global__ __launch_bounds__(256) void dwconv_dgrad_k(const float* __restrict__ g, const float* __restrict__ w,
                                                      float* __restrict__ dx, int H, int W, int C, int pad, int Ho,
                                                      int Wo, int cpr, FastDiv dcv, int nq, int Cw = 0) {
  static_assert(!CARRY || V == 4, "carried widths run on the float4 path");
  constexpr int KK = K * K, DMIN = DwTaps<K, S, PB>::lo(), ND = DwTaps<K, S, PB>::hi() - DMIN + 1;
  const int row = blockIdx.x / cpr, chunk = blockIdx.x - row * cpr;  // row = b * H + ih
  const int q = chunk * 256 + threadIdx.x;
  if (q >= nq) return;
  const int strip = dcv.div(q), c = (q - strip * (C / V)) * V;
  const int b = row / H, ih = row - b * H;
  const int iw0 = strip * DW_SW;
  const int ow_lo = (iw0 + pad - PB) / S + DMIN;  // exact division: (iw0 + pad) % S == PB
  float* dr = dx + row * W * C + c;
  bool edge = false;  // the quad straddles Cw
  if constexpr (CARRY) {
    if (c >= Cw) {
      dw_store_zeros(dr, iw0, W, C);
      return;
    }
    edge = c + 4 > Cw;
  }
  float wf[V * KK];
  if constexpr (CARRY) {
    if (edge) dw_load_w_edge<KK>(w, c, Cw, wf);
    else dw_load_w<V, KK>(w, c, wf);
  } else {
    dw_load_w<V, KK>(w, c, wf);
  }
  float acc[DW_SW][V];
#pragma unroll
  for (int j = 0; j < DW_SW; ++j)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[j][v] = 0.f;
#pragma unroll
  for (int kh = 0; kh < K; ++kh) {
    const int n = ih + pad - kh;  // block-uniform row tests
    if (n < 0 || (S == 2 && (n & 1))) continue;
    const int oh = n / S;
    if (oh >= Ho) continue;
    const float* gr = g + (b * Ho + oh) * Wo * C + c;
    float gv[ND][V];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int ow = ow_lo + d;
#pragma unroll
      for (int v = 0; v < V; ++v) gv[d][v] = 0.f;
      if (ow >= 0 && ow < Wo) DwVec<V>::load(gr + ow * C, gv[d]);
    }
#pragma unroll
    for (int j = 0; j < DW_SW; ++j)
#pragma unroll
      for (int kw = 0; kw < K; ++kw)
        if ((PB + j - kw) % S == 0) {
#pragma unroll
          for (int v = 0; v < V; ++v)
            acc[j][v] = fmaf(gv[(PB + j - kw) / S - DMIN][v], wf[v * KK + kh * K + kw], acc[j][v]);
        }
  }
  if constexpr (CARRY) {
    if (edge) {  // exact zeros in the padding lanes, whatever g holds there
#pragma unroll
      for (int j = 0; j < DW_SW; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[j][v] = c + v < Cw ? acc[j][v] : 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < DW_SW; ++j)
    if (iw0 + j < W) DwVec<V>::store(dr + (iw0 + j) * C, acc[j]);
}

// Weight / bias gradient partials of one (channel slice, chunk of work units). A unit is a strip
// of DW_SW consecutive output pixels of one output row, so a thread loads the overlapping input
// columns of the strip's windows once per kernel row. A block holds 2^cxs channel vectors (up to
// 64 channels) x PT = 256 >> cxs unit lanes: thread (cx, py) owns a channel vector and the
// chunk's units u0 + py, u0 + py + PT, ...; the PT unit lanes of a channel are then summed in
// lane order in fp64 through the LDS, DW_FOLD_TAPS taps per round.
template <int K, int S, int V>
__global__ __launch_bounds__(256) void dwconv_wgrad_k(const float* __restrict__ g, const float* __restrict__ x,
                                                      double* __restrict__ ws, int H, int W, int C, int pad, int Ho,
                                                      int Wo, int U, int upc, int nstr, int cxs, FastDiv dstr,
                                                      FastDiv dho, int Cw) {
  constexpr int KK = K * K, NT = KK + 1, NIN = (DW_SW - 1) * S + K;
  const int PT = 256 >> cxs;
  const int cx = threadIdx.x & ((1 << cxs) - 1), py = threadIdx.x >> cxs;
  const int c = ((blockIdx.x << cxs) + cx) * V;
  // C % V == 0: a channel vector is inside or outside the pitch C as a whole. Cw <= C: the channels
  // with parameters; a quad wholly past Cw does no work (its workspace rows stay unwritten and the
  // fold never reads them), the padding lanes of the quad that straddles Cw are reduced like any
  // other lane (whatever g / x hold there) and dropped by the fold
  const bool active = c < Cw;
  const int chunk = blockIdx.y;
  const int u0 = chunk * upc, u1 = min(U, u0 + upc);
  float acc[NT][V];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[t][v] = 0.f;
  if (active) {
    for (int u = u0 + py; u < u1; u += PT) {
      const int r = dstr.div(u), ow0 = (u - r * nstr) * DW_SW;  // r = b * Ho + oh
      const int b = dho.div(r), oh = r - b * Ho;
      float gv[DW_SW][V];
      const float* gr = g + (r * Wo + ow0) * C + c;
#pragma unroll
      for (int j = 0; j < DW_SW; ++j) {
#pragma unroll
        for (int v = 0; v < V; ++v) gv[j][v] = 0.f;
        if (ow0 + j < Wo) DwVec<V>::load(gr + j * C, gv[j]);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[KK][v] += gv[j][v];
      }
      const int ih0 = oh * S - pad, iw0 = ow0 * S - pad;
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        const int ih = ih0 + kh;
        if (ih < 0 || ih >= H) continue;
        const float* xr = x + (b * H + ih) * W * C + c;
        float in[NIN][V];
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
          const int iw = iw0 + i;
#pragma unroll
          for (int v = 0; v < V; ++v) in[i][v] = 0.f;
          if (iw >= 0 && iw < W) DwVec<V>::load(xr + iw * C, in[i]);
        }
#pragma unroll
        for (int j = 0; j < DW_SW; ++j)
#pragma unroll
          for (int kw = 0; kw < K; ++kw)
#pragma unroll
            for (int v = 0; v < V; ++v)
              acc[kh * K + kw][v] = fmaf(gv[j][v], in[j * S + kw][v], acc[kh * K + kw][v]);
      }
    }
  }
  __shared__ float red[DW_FOLD_TAPS][256 * V];
#pragma unroll
  for (int t0 = 0; t0 < NT; t0 += DW_FOLD_TAPS) {
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < DW_FOLD_TAPS; ++tt)
      if (t0 + tt < NT) {
#pragma unroll
        for (int v = 0; v < V; ++v) red[tt][threadIdx.x * V + v] = acc[t0 + tt][v];
      }
    __syncthreads();
    if (active && py < DW_FOLD_TAPS && t0 + py < NT) {  // (PT >= DW_FOLD_TAPS: cxs <= 6)
      double* out = ws + (chunk * NT + t0 + py) * C + c;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        double s = 0.0;
        for (int i = 0; i < PT; ++i) s += (double)red[py][((i << cxs) + cx) * V + v];
        out[v] = s;
      }
    }
  }
}

// dW[c, kh, kw] (the parameter's strides) / db[c] = the chunks' partials folded in a fixed order.
// A block folds 16 consecutive (tap, channel) elements: thread (e, l) sums the chunks l, l + 16, ...
// in index order (16 independent load streams per element: one serial pass over up to 1024 chunks
// is bound by load latency), then lane 0 adds the 16 partials in lane order; all in fp64.
__global__ __launch_bounds__(256) void dwconv_wgrad_fold(const double* __restrict__ ws, float* __restrict__ dw,
                                                         float* __restrict__ db, int chunks, int C, int K,
                                                         long long s0, long long s2, long long s3, int Cw) {
  const int KK = K * K, NT = KK + 1, n = NT * C;
  const int e = threadIdx.x & 15, l = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + e;
  const int t = i / C, c = i - t * C;
  const bool real = i < n && c < Cw;  // dW / db have Cw channels: the padding of a carried width is skipped
  double s = 0.0;
  if (real)
    for (int ch = l; ch < chunks; ch += 16) s += ws[ch * n + i];
  __shared__ double part[16][16];
  part[l][e] = s;
  __syncthreads();
  if (l != 0 || !real) return;
  s = 0.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) s += part[j][e];
  if (t < KK) {
    const int kh = t / K, kw = t - kh * K;
    dw[c * s0 + kh * s2 + kw * s3] = (float)s;
  } else if (db != nullptr) {
    db[c] = (float)s;
  }
}

}  // namespace tp

// A carried width: the activations have C channels per pixel, the parameter Cw <= C of them; the
// float4 path (C % 4 == 0) is the only one that takes Cw < C
static bool dw_carried_ok(int C, int Cw) { return Cw > 0 && Cw <= C && (Cw == C || C % 4 == 0); }

// y = dwconv(x, w) (+ bias): x (B, H, W, C), w (Cw, 1, k, k), bias (Cw), y (B, Ho, Wo, C); the channels
// c >= Cw of y are exact zeros, whatever x holds there
extern "C" hipError_t tp_dwconv_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H,
                                    int W, int C, int Cw, int k, int s, int pad, hipStream_t st) {
  int Ho, Wo, cpr, nq;
  long long blocks;
  if (!dw_carried_ok(C, Cw) || !tp::dw_geometry(B, H, W, C, k, s, pad, &Ho, &Wo) || !tp::dw_aligned(C, x, w, bias, y))
    return hipErrorInvalidValue;
  const int V = C % 4 == 0 ? 4 : 1;
  if (!tp::dw_row_grid(B * Ho, Wo, C, V, &cpr, &nq, &blocks)) return hipErrorInvalidValue;
  const tp::FastDiv dcv((unsigned)(C / V));
#define TP_DW_FWD(K_, S_, V_, CARRY_)                                                                                \
  tp::dwconv_fwd_k<K_, S_, V_, CARRY_><<<(unsigned)blocks, 256, 0, st>>>(x, w, bias, y, H, W, C, pad, Ho, Wo, cpr, dcv, \
                                                                         nq, Cw)
  if (Cw < C) TP_DW_KS(TP_DW_FWD, 4, true);
  else if (V == 4) TP_DW_KS(TP_DW_FWD, 4, false);
  else TP_DW_KS(TP_DW_FWD, 1, false);
#undef TP_DW_FWD
  return hipGetLastError();
}

// dx (B, H, W, C) from g (B, Ho, Wo, C) and w (Cw, 1, k, k); the channels c >= Cw of dx are exact zeros
extern "C" hipError_t tp_dwconv_dgrad(const float* g, const float* w, float* dx, int B, int H, int W, int C, int Cw,
                                      int k, int s, int pad, hipStream_t st) {
  int Ho, Wo, cpr, nq;
  long long blocks;
  if (!dw_carried_ok(C, Cw) || !tp::dw_geometry(B, H, W, C, k, s, pad, &Ho, &Wo) || !tp::dw_aligned(C, g, w, dx))
    return hipErrorInvalidValue;
  const int V = C % 4 == 0 ? 4 : 1;
  if (!tp::dw_row_grid(B * H, W, C, V, &cpr, &nq, &blocks)) return hipErrorInvalidValue;
  const tp::FastDiv dcv((unsigned)(C / V));
  const int pb = pad % s;  // parity of iw0 + pad (strips start at multiples of 4)
#define TP_DW_DG(K_, S_, V_, CARRY_)                                                                               \
  do {                                                                                                             \
    if (S_ == 2 && pb == 1)                                                                                        \
      tp::dwconv_dgrad_k<K_, S_, S_ - 1, V_, CARRY_><<<(unsigned)blocks, 256, 0, st>>>(g, w, dx, H, W, C, pad, Ho, Wo, \
                                                                                       cpr, dcv, nq, Cw);          \
    else                                                                                                           \
      tp::dwconv_dgrad_k<K_, S_, 0, V_, CARRY_><<<(unsigned)blocks, 256, 0, st>>>(g, w, dx, H, W, C, pad, Ho, Wo, cpr, \
                                                                                  dcv, nq, Cw);                    \
  } while (0)
  if (Cw < C) TP_DW_KS(TP_DW_DG, 4, true);
  else if (V == 4) TP_DW_KS(TP_DW_DG, 4, false);
  else TP_DW_KS(TP_DW_DG, 1, false);
#undef TP_DW_DG
  return hipGetLastError();
}

// Chunks of the wgrad grid for P = B * Ho * Wo output pixels: about eight blocks per CU over the
// (channel slices x chunks) grid, at least 256 pixels per chunk (a few strips per thread before the
// block's LDS reduction), at most 1024 chunks. The workspace holds chunks * (k*k + 1) * C doubles.
extern "C" int tp_dwconv_wgrad_chunks(int P, int C) {
  if (P < 1 || C < 1) return 1;
  const int slices = (int)(((long long)C + tp::DW_SLICE - 1) / tp::DW_SLICE);
  const int chunks = std::min(1024, std::max(1, 2048 / slices));
  return std::min(chunks, std::max(1, P / 256));
}

// dW[c, 0, kh, kw] at dw[c * s0 + kh * s2 + kw * s3] (the parameter's own strides, in elements) for
// the Cw channels of the parameter and, with db, db[c] = sum g (Cw entries); g / x carry C >= Cw
// channels per pixel. ws: tp_dwconv_wgrad_chunks(P, C) * (k*k + 1) * C doubles (sized by the carried
// width), chunks = that count
extern "C" hipError_t tp_dwconv_wgrad(const float* g, const float* x, float* dw, float* db, double* ws, int chunks,
                                      int B, int H, int W, int C, int Cw, int k, int s, int pad, long long s0,
                                      long long s2, long long s3, hipStream_t st) {
  int Ho, Wo;
  if (!dw_carried_ok(C, Cw) || !tp::dw_geometry(B, H, W, C, k, s, pad, &Ho, &Wo) || !tp::dw_aligned(C, g, x, ws))
    return hipErrorInvalidValue;
  const int P = B * Ho * Wo;
  if (dw == nullptr || ws == nullptr || ((uintptr_t)ws & 7) || ((uintptr_t)dw & 3) || ((uintptr_t)db & 3))
    return hipErrorInvalidValue;
  if (chunks != tp_dwconv_wgrad_chunks(P, C) || s0 < 1 || s2 < 1 || s3 < 1) return hipErrorInvalidValue;
  if (s0 >= tp::DW_MAX_BYTES || s2 >= tp::DW_MAX_BYTES || s3 >= tp::DW_MAX_BYTES) return hipErrorInvalidValue;
  if ((s0 * (Cw - 1) + s2 * (k - 1) + s3 * (k - 1) + 1) * 4 >= tp::DW_MAX_BYTES) return hipErrorInvalidValue;
  if (tp::ceil_div((long long)(k * k + 1) * C, 16) >= tp::DW_MAX_BLOCKS) return hipErrorInvalidValue;  // the fold's grid
  const int V = C % 4 == 0 ? 4 : 1, CV = C / V;
  int cxs = 0;  // 2^cxs channel vectors per block: up to 64 channels, no more than the layer has
  while ((1 << cxs) < CV && (V << cxs) < tp::DW_SLICE) ++cxs;
  const int nstr = (int)tp::ceil_div(Wo, tp::DW_SW), U = B * Ho * nstr;  // work units: strips of output rows
  const int upc = (U + chunks - 1) / chunks;
  const dim3 grid((CV + (1 << cxs) - 1) >> cxs, chunks);
  const tp::FastDiv dstr((unsigned)nstr), dho((unsigned)Ho);
#define TP_DW_WG(K_, S_, V_)                                                                                          \
  tp::dwconv_wgrad_k<K_, S_, V_><<<grid, 256, 0, st>>>(g, x, ws, H, W, C, pad, Ho, Wo, U, upc, nstr, cxs, dstr, dho, \
                                                       Cw)
  if (V == 4) TP_DW_KS(TP_DW_WG, 4);
  else TP_DW_KS(TP_DW_WG, 1);
#undef TP_DW_WG
  const int n = (k * k + 1) * C;
  tp::dwconv_wgrad_fold<<<tp::ceil_div(n, 16), 256, 0, st>>>(ws, dw, db, chunks, C, k, s0, s2, s3, Cw);
  return hipGetLastError();
}
