// Squeeze-and-excitation gates (MobileNetV3 / EfficientNet) of the training path, fp32 NHWC:
//   out = x * s,  s = gate(W2 . relu(W1 . mean_hw(x) + b1) + b2),  gate = Hardsigmoid | Sigmoid
// x is (B, H, W, C) at its real width. ANY channel count is taken (pruned widths are arbitrary): a
// float4 path when C % 4 == 0 and a per-element path otherwise, as dwconv.hip. The passes over
// the activation are memory-bound and are the only ones that matter: forward reads x twice (pool,
// scale) and writes once; backward reads g and x once (product-reduce), g once more and writes dx
// once, so the pool's broadcast gradient and the scale's gradient never exist as tensors. The two
// FCs run on (B, C) / (B, Cs) rows in one launch each way, with the weights read in the
// parameters' own layout (Conv2d (Cs, C, 1, 1) and Linear (Cs, C) are the same bytes).
//
// Every sum runs in a fixed order (registers, then LDS, then per-block partial slots folded in slot
// order; wave reductions are fixed butterflies) and there are no atomics: results are bit-identical
// run to run.
//
// reduce (pool / product-reduce): a block holds 2^cxs channel vectors (up to 64) x PT = 256 >> cxs
// pixel lanes and one chunk of one image's pixels: thread (cx, py) owns a channel vector and the
// pixels p0 + py, p0 + py + PT, ...; the PT lanes of a channel are then summed in lane order in
// fp64 through the LDS. When B x C alone does not fill the chip (7- and 14-pixel maps at small
// batches, narrow layers) the pixels of an image are split over `splits` blocks which write
// partial slots [split][b][c], folded in slot order by a second small kernel.
#include "tp_common.h"
#include "tp_launchers.h"

namespace tp {

constexpr long long SE_MAX_BYTES = 1ll << 31;  // operands are indexed with 32-bit element offsets
constexpr long long SE_MAX_BLOCKS = 1ll << 22;  // blocks of up to 1024 threads: below HIP's 2^32 threads per grid
constexpr int SE_MAX_GRID_YZ = 65535;
constexpr int SE_MAX_SPLITS = 64;
constexpr int SE_MAX_FC = 12288;  // C + Cs floats of a gate kernel's LDS rows (48 KiB)

template <int V>
struct SeVec;
template <>
struct SeVec<4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <>
struct SeVec<1> {
  static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float* v) { *p = v[0]; }
};

// out[(split * B + b) * C + c] = scale * sum over the split's pixels of a (PROD: a * x)
template <int V, bool PROD>
__global__ __launch_bounds__(256) void se_reduce_k(const float* __restrict__ a, const float* __restrict__ x,
                                                   float* __restrict__ out, int B, int HW, int C, int ppc, int cxs,
                                                   double scale) {
  const int PT = 256 >> cxs;
  const int cx = threadIdx.x & ((1 << cxs) - 1), py = threadIdx.x >> cxs;
  const int c = ((blockIdx.x << cxs) + cx) * V;
  const bool active = c < C;  // C % V == 0: a channel vector is inside or outside as a whole
  const int b = blockIdx.z, split = blockIdx.y;
  const int p0 = split * ppc, p1 = min(HW, p0 + ppc);
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.f;
  if (active) {
    const int base = b * HW * C + c;
#pragma unroll 4
    for (int p = p0 + py; p < p1; p += PT) {
      float av[V];
      SeVec<V>::load(a + base + p * C, av);
      if constexpr (PROD) {
        float xv[V];
        SeVec<V>::load(x + base + p * C, xv);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = fmaf(av[v], xv[v], acc[v]);
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += av[v];
      }
    }
  }
  __shared__ float red[256 * V];
#pragma unroll
  for (int v = 0; v < V; ++v) red[threadIdx.x * V + v] = acc[v];
  __syncthreads();
  if (!active || py != 0) return;
  float r[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    double s = 0.0;
    for (int i = 0; i < PT; ++i) s += (double)red[((i << cxs) + cx) * V + v];
    r[v] = (float)(s * scale);
  }
  SeVec<V>::store(out + (split * B + b) * C + c, r);
}

// out[i] = scale * (ws[0][i] + ws[1][i] + ...), i < n = B * C, in slot order
__global__ __launch_bounds__(256) void se_fold_k(const float* __restrict__ ws, float* __restrict__ out, int splits,
                                                 int n, double scale) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = 0; k < splits; ++k) s += (double)ws[k * n + i];
  out[i] = (float)(s * scale);
}

// out = a * s[b, c] (ADD: + dp[b, c] * inv_hw); one block column per image, q = pixel * CV + channel vector
template <int V, bool ADD>
__global__ __launch_bounds__(256) void se_apply_k(const float* __restrict__ a, const float* __restrict__ s,
                                                  const float* __restrict__ dp, float* __restrict__ out, int nq,
                                                  int C, FastDiv dcv, float inv_hw) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int b = blockIdx.y;
  const int pix = dcv.div(q), c = (q - pix * (C / V)) * V;
  const int off = b * nq * V + q * V;  // q * V == pix * C + c
  float av[V], sv[V], r[V];
  SeVec<V>::load(a + off, av);
  SeVec<V>::load(s + b * C + c, sv);
  if constexpr (ADD) {
    float dv[V];
    SeVec<V>::load(dp + b * C + c, dv);
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = fmaf(av[v], sv[v], dv[v] * inv_hw);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = av[v] * sv[v];
  }
  SeVec<V>::store(out + off, r);
}

// sum over groups of G consecutive lanes (G a power of two <= 64): a fixed butterfly
__device__ __forceinline__ float se_group_sum(float v, int G) {
  for (int off = G >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float se_gate(float z, int gate) {
  if (z != z) return z;  // NaN passes through (the pruner's probe)
  if (gate == 0) return fminf(fmaxf(z + 3.f, 0.f), 6.f) / 6.f;  // exactly 0 / 1 outside (-3, 3)
  return 1.f / (1.f + expf(-z));
}

constexpr int SE_FC_THREADS = 1024;  // threads of a gate kernel's block (16 waves: the FCs are latency-bound)
constexpr int SE_FC_ROWS = 4;         // rows a lane group takes at once (independent loads in flight)

// Dot products of the rows of a row-major (nrows, len) matrix with a vector in the LDS. A group of G
// lanes (G = the power of two >= len, at most 64) takes SE_FC_ROWS rows at once, lane l of the group
// over the elements l, l + G, ... of each, then a butterfly over the group; emit(row, value) runs on
// the group's lane 0. Every lane of the block must call this (the butterflies).
template <typename Emit>
__device__ __forceinline__ void se_rows_dot(const float* __restrict__ w, const float* vec, int nrows, int len, int G,
                                            Emit emit) {
  const int l = threadIdx.x & (G - 1), grp = threadIdx.x / G, ngrp = SE_FC_THREADS / G;
  for (int r0 = 0; r0 < nrows; r0 += ngrp * SE_FC_ROWS) {  // block-uniform trip count
    const int rbase = r0 + grp * SE_FC_ROWS;
    float acc[SE_FC_ROWS];
    const float* wr[SE_FC_ROWS];
#pragma unroll
    for (int r = 0; r < SE_FC_ROWS; ++r) {
      acc[r] = 0.f;
      wr[r] = w + min(rbase + r, nrows - 1) * len;  // (rows past the end recompute the last one; not emitted)
    }
#pragma unroll 2
    for (int k = l; k < len; k += G) {
      const float v = vec[k];
#pragma unroll
      for (int r = 0; r < SE_FC_ROWS; ++r) acc[r] = fmaf(wr[r][k], v, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < SE_FC_ROWS; ++r) {
      acc[r] = se_group_sum(acc[r], G);
      if (l == 0 && rbase + r < nrows) emit(rbase + r, acc[r]);
    }
  }
}

// One block per image: h = relu(W1 . p + b1) (Cs), s = gate(W2 . h + b2) (C), the rows of both
// weights by se_rows_dot.
__global__ __launch_bounds__(SE_FC_THREADS) void se_gate_fwd_k(const float* __restrict__ p,
                                                               const float* __restrict__ w1,
                                                               const float* __restrict__ b1,
                                                               const float* __restrict__ w2,
                                                               const float* __restrict__ b2, float* __restrict__ h,
                                                               float* __restrict__ s, int C, int Cs, int g1, int g2,
                                                               int gate) {
  extern __shared__ float lds[];
  float* pl = lds;      // C
  float* hl = lds + C;  // Cs
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += SE_FC_THREADS) pl[c] = p[b * C + c];
  __syncthreads();
  se_rows_dot(w1, pl, Cs, C, g1, [&](int j, float acc) {
    const float v = nan_relu(acc + (b1 != nullptr ? b1[j] : 0.f));
    hl[j] = v;
    h[b * Cs + j] = v;
  });
  __syncthreads();
  se_rows_dot(w2, hl, C, Cs, g2,
              [&](int c, float acc) { s[b * C + c] = se_gate(acc + (b2 != nullptr ? b2[c] : 0.f), gate); });
}

// One block per image: dz2 = ds * gate'(s) (C), dz1 = (dz2 . W2) * [h > 0] (Cs), dp = dz1 . W1 (C).
// Both products run down the columns of a row-major weight: a thread owns a column (consecutive
// lanes read consecutive addresses); for dz1 the rows are dealt to `parts` = threads / tj threads
// per column, whose partial sums are folded in part order through the LDS.
__global__ __launch_bounds__(SE_FC_THREADS) void se_gate_bwd_k(const float* __restrict__ ds,
                                                               const float* __restrict__ s,
                                                               const float* __restrict__ h,
                                                               const float* __restrict__ w1,
                                                               const float* __restrict__ w2, float* __restrict__ dz2,
                                                               float* __restrict__ dz1, float* __restrict__ dp, int C,
                                                               int Cs, int tj, int gate) {
  extern __shared__ float lds[];
  float* z2 = lds;             // C
  float* z1 = lds + C;         // Cs
  float* part = lds + C + Cs;  // SE_FC_THREADS
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += SE_FC_THREADS) {
    const float sv = s[b * C + c];
    const float d = gate == 0 ? ((sv > 0.f && sv < 1.f) ? 1.f / 6.f : 0.f) : sv * (1.f - sv);
    const float v = ds[b * C + c] * d;
    z2[c] = v;
    dz2[b * C + c] = v;
  }
  __syncthreads();
  const int parts = SE_FC_THREADS / tj, jl = threadIdx.x & (tj - 1), pt = threadIdx.x / tj;
  for (int j0 = 0; j0 < Cs; j0 += tj) {  // block-uniform trip count (the barriers)
    const int j = j0 + jl;
    float acc = 0.f;
    if (j < Cs) {
#pragma unroll 8
      for (int c = pt; c < C; c += parts) acc = fmaf(z2[c], w2[c * Cs + j], acc);
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (pt == 0 && j < Cs) {
      float t = 0.f;
      for (int i = 0; i < parts; ++i) t += part[i * tj + jl];
      const float v = h[b * Cs + j] > 0.f ? t : 0.f;
      z1[j] = v;
      dz1[b * Cs + j] = v;
    }
    __syncthreads();
  }
  for (int c = threadIdx.x; c < C; c += SE_FC_THREADS) {
    float acc = 0.f;
#pragma unroll 8
    for (int j = 0; j < Cs; ++j) acc = fmaf(z1[j], w1[j * C + c], acc);
    dp[b * C + c] = acc;
  }
}

// dW[r, k] = sum_b a[b, r] * m[b, k] at dw[r * s0 + k * s1] (the parameter's strides) and, with db,
// db[r] = sum_b a[b, r]; b ascending. One thread per element of dW.
__global__ __launch_bounds__(256) void se_wgrad_k(const float* __restrict__ a, const float* __restrict__ m,
                                                  float* __restrict__ dw, float* __restrict__ db, int B, int R, int K,
                                                  long long s0, long long s1, FastDiv dk) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R * K) return;
  const int r = dk.div(i), k = i - r * K;
  float acc = 0.f, bias = 0.f;
#pragma unroll 8
  for (int b = 0; b < B; ++b) {
    const float av = a[b * R + r];
    acc = fmaf(av, m[b * K + k], acc);
    bias += av;
  }
  dw[r * s0 + k * s1] = acc;
  if (db != nullptr && k == 0) db[r] = bias;
}

// n * m * 4 bytes below 2^31 (n below it already): no overflow for any int arguments
static inline bool se_grow(long long& n, int m) {
  if (m < 1) return false;
  n *= m;
  return n * 4 < SE_MAX_BYTES;
}

// a (B, HW, C) activation below 2^31 bytes that the grids take
static inline bool se_act_ok(int B, int HW, int C) {
  long long n = 1;
  return se_grow(n, B) && se_grow(n, HW) && se_grow(n, C) && B <= SE_MAX_GRID_YZ;
}

// the FC operands: (B, C), (B, Cs) rows and (Cs, C) weights below 2^31 bytes, the LDS rows in range
static inline bool se_fc_ok(int B, int C, int Cs) {
  long long n = 1, w = 1;
  if (!(se_grow(n, B) && se_grow(n, C) && se_grow(w, C) && se_grow(w, Cs))) return false;
  n = 1;
  if (!(se_grow(n, B) && se_grow(n, Cs))) return false;
  return (long long)C + Cs <= SE_MAX_FC && B < SE_MAX_BLOCKS;
}

static inline bool se_aligned(int C, const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d;
  return (bits & (C % 4 == 0 ? 15 : 3)) == 0;
}

static inline int se_pow2_at_least(int n, int cap) {
  int g = 1;
  while (g < n && g < cap) g <<= 1;
  return g;
}

// 2^cxs channel vectors per reduce block: up to 64, no more than the layer has
static inline int se_cxs(int CV) {
  int cxs = 0;
  while ((1 << cxs) < CV && cxs < 6) ++cxs;
  return cxs;
}

}  // namespace tp

// Pixel splits of the reduce kernels for a (B, HW, C) activation: 1 when the (image, channel slice)
// blocks alone give about two blocks per CU; else enough splits for that, each with at least four
// pixels per pixel lane, at most 64. The workspace holds splits * B * C floats when splits > 1.
extern "C" int tp_se_splits(int B, int HW, int C) {
  if (B < 1 || HW < 1 || C < 1) return 1;
  const int V = C % 4 == 0 ? 4 : 1, CV = C / V, cxs = tp::se_cxs(CV), PT = 256 >> cxs;
  const long long blocks = (((long long)CV + (1 << cxs) - 1) >> cxs) * B;  // (64-bit: any int arguments)
  if (blocks >= 512) return 1;
  const long long want = (512 + blocks - 1) / blocks, most = std::max(1, HW / (PT * 4));
  const long long splits = std::min<long long>(std::min(want, most), tp::SE_MAX_SPLITS);
  const long long ppc = (HW + splits - 1) / splits;
  return (int)((HW + ppc - 1) / ppc);  // no empty split
}

// shared body of the pool and the product-reduce: out (B, C) = scale * sum_hw a (* x)
static hipError_t se_reduce(const float* a, const float* x, float* out, float* ws, int splits, int B, int HW, int C,
                            bool prod, double scale, hipStream_t st) {
  if (a == nullptr || out == nullptr || (prod && x == nullptr) || !tp::se_act_ok(B, HW, C)) return hipErrorInvalidValue;
  if (splits != tp_se_splits(B, HW, C) || (splits > 1 && ws == nullptr)) return hipErrorInvalidValue;
  if (!tp::se_aligned(C, a, x, out, ws)) return hipErrorInvalidValue;
  const int V = C % 4 == 0 ? 4 : 1, CV = C / V, cxs = tp::se_cxs(CV);
  const int ppc = (HW + splits - 1) / splits;
  const dim3 grid((CV + (1 << cxs) - 1) >> cxs, splits, B);
  if ((long long)grid.x * splits * B >= tp::SE_MAX_BLOCKS) return hipErrorInvalidValue;
  if ((long long)splits * B * C * 4 >= tp::SE_MAX_BYTES) return hipErrorInvalidValue;
  float* dst = splits > 1 ? ws : out;
  const double sc = splits > 1 ? 1.0 : scale;
  if (V == 4 && prod) tp::se_reduce_k<4, true><<<grid, 256, 0, st>>>(a, x, dst, B, HW, C, ppc, cxs, sc);
  else if (V == 4) tp::se_reduce_k<4, false><<<grid, 256, 0, st>>>(a, x, dst, B, HW, C, ppc, cxs, sc);
  else if (prod) tp::se_reduce_k<1, true><<<grid, 256, 0, st>>>(a, x, dst, B, HW, C, ppc, cxs, sc);
  else tp::se_reduce_k<1, false><<<grid, 256, 0, st>>>(a, x, dst, B, HW, C, ppc, cxs, sc);
  if (splits > 1) tp::se_fold_k<<<tp::ceil_div((long long)B * C, 256), 256, 0, st>>>(ws, out, splits, B * C, scale);
  return hipGetLastError();
}

// p (B, C) = mean over HW of x (B, HW, C); ws: splits * B * C floats when splits = tp_se_splits(...) > 1
extern "C" hipError_t tp_se_pool(const float* x, float* p, float* ws, int splits, int B, int HW, int C,
                                 hipStream_t st) {
  if (HW < 1) return hipErrorInvalidValue;
  return se_reduce(x, nullptr, p, ws, splits, B, HW, C, false, 1.0 / (double)HW, st);
}

// ds (B, C) = sum over HW of g * x
extern "C" hipError_t tp_se_bwd_reduce(const float* g, const float* x, float* ds, float* ws, int splits, int B, int HW,
                                       int C, hipStream_t st) {
  return se_reduce(g, x, ds, ws, splits, B, HW, C, true, 1.0, st);
}

// h (B, Cs) = relu(p . W1^T + b1), s (B, C) = gate(h . W2^T + b2); w1 (Cs, C), w2 (C, Cs) row-major,
// b1 / b2 may be null; gate 0 Hardsigmoid, 1 Sigmoid
extern "C" hipError_t tp_se_gate_fwd(const float* p, const float* w1, const float* b1, const float* w2,
                                     const float* b2, float* h, float* s, int B, int C, int Cs, int gate,
                                     hipStream_t st) {
  if (p == nullptr || w1 == nullptr || w2 == nullptr || h == nullptr || s == nullptr) return hipErrorInvalidValue;
  if ((gate != 0 && gate != 1) || !tp::se_fc_ok(B, C, Cs)) return hipErrorInvalidValue;
  if (!tp::se_aligned(1, p, w1, w2, h) || !tp::se_aligned(1, s, b1, b2)) return hipErrorInvalidValue;
  const int g1 = tp::se_pow2_at_least(C, 64), g2 = tp::se_pow2_at_least(Cs, 64);
  tp::se_gate_fwd_k<<<B, tp::SE_FC_THREADS, (size_t)(C + Cs) * sizeof(float), st>>>(p, w1, b1, w2, b2, h, s, C, Cs, g1, g2, gate);
  return hipGetLastError();
}

// dz2 (B, C) = ds * gate'(s), dz1 (B, Cs) = (dz2 . W2) * [h > 0], dp (B, C) = dz1 . W1
extern "C" hipError_t tp_se_gate_bwd(const float* ds, const float* s, const float* h, const float* w1,
                                     const float* w2, float* dz2, float* dz1, float* dp, int B, int C, int Cs,
                                     int gate, hipStream_t st) {
  if (ds == nullptr || s == nullptr || h == nullptr || w1 == nullptr || w2 == nullptr || dz2 == nullptr ||
      dz1 == nullptr || dp == nullptr)
    return hipErrorInvalidValue;
  if ((gate != 0 && gate != 1) || !tp::se_fc_ok(B, C, Cs)) return hipErrorInvalidValue;
  if (!tp::se_aligned(1, ds, s, h, w1) || !tp::se_aligned(1, w2, dz2, dz1, dp)) return hipErrorInvalidValue;
  const int tj = tp::se_pow2_at_least(Cs, tp::SE_FC_THREADS);
  tp::se_gate_bwd_k<<<B, tp::SE_FC_THREADS, (size_t)(C + Cs + tp::SE_FC_THREADS) * sizeof(float), st>>>(
      ds, s, h, w1, w2, dz2, dz1, dp, C, Cs, tj, gate);
  return hipGetLastError();
}

// shared body of the scale and the input gradient: out = a * s[b, c] (+ dp[b, c] / HW)
static hipError_t se_apply(const float* a, const float* s, const float* dp, float* out, int B, int HW, int C, bool add,
                           hipStream_t st) {
  if (a == nullptr || s == nullptr || out == nullptr || (add && dp == nullptr) || !tp::se_act_ok(B, HW, C))
    return hipErrorInvalidValue;
  if (!tp::se_aligned(C, a, s, dp, out)) return hipErrorInvalidValue;
  const int V = C % 4 == 0 ? 4 : 1, CV = C / V;
  const long long nq = (long long)HW * CV;  // below 2^29
  const dim3 grid(tp::ceil_div(nq, 256), B);
  if ((long long)grid.x * B >= tp::SE_MAX_BLOCKS) return hipErrorInvalidValue;
  const tp::FastDiv dcv((unsigned)CV);
  const float inv_hw = 1.f / (float)HW;
  if (V == 4 && add) tp::se_apply_k<4, true><<<grid, 256, 0, st>>>(a, s, dp, out, (int)nq, C, dcv, inv_hw);
  else if (V == 4) tp::se_apply_k<4, false><<<grid, 256, 0, st>>>(a, s, dp, out, (int)nq, C, dcv, inv_hw);
  else if (add) tp::se_apply_k<1, true><<<grid, 256, 0, st>>>(a, s, dp, out, (int)nq, C, dcv, inv_hw);
  else tp::se_apply_k<1, false><<<grid, 256, 0, st>>>(a, s, dp, out, (int)nq, C, dcv, inv_hw);
  return hipGetLastError();
}

// out (B, HW, C) = x * s[b, c]
extern "C" hipError_t tp_se_scale(const float* x, const float* s, float* out, int B, int HW, int C, hipStream_t st) {
  return se_apply(x, s, nullptr, out, B, HW, C, false, st);
}

// dx (B, HW, C) = g * s[b, c] + dp[b, c] / HW
extern "C" hipError_t tp_se_bwd_dx(const float* g, const float* s, const float* dp, float* dx, int B, int HW, int C,
                                   hipStream_t st) {
  return se_apply(g, s, dp, dx, B, HW, C, true, st);
}

// dW[r, k] = sum_b a[b, r] * m[b, k] at dw[r * s0 + k * s1] (strides in elements) and, with db,
// db[r] = sum_b a[b, r]: a (B, R), m (B, K). dW2 = (dz2, h), dW1 = (dz1, p).
extern "C" hipError_t tp_se_wgrad(const float* a, const float* m, float* dw, float* db, int B, int R, int K,
                                  long long s0, long long s1, hipStream_t st) {
  if (a == nullptr || m == nullptr || dw == nullptr) return hipErrorInvalidValue;
  long long na = 1, nm = 1, nw = 1;
  if (!(tp::se_grow(na, B) && tp::se_grow(na, R) && tp::se_grow(nm, B) && tp::se_grow(nm, K) && tp::se_grow(nw, R) &&
        tp::se_grow(nw, K)))
    return hipErrorInvalidValue;
  if (!tp::se_aligned(1, a, m, dw, db)) return hipErrorInvalidValue;
  if (s0 < 1 || s1 < 1 || s0 >= tp::SE_MAX_BYTES || s1 >= tp::SE_MAX_BYTES) return hipErrorInvalidValue;
  if ((s0 * (R - 1) + s1 * (K - 1) + 1) * 4 >= tp::SE_MAX_BYTES) return hipErrorInvalidValue;
  if (tp::ceil_div(nw, 256) >= tp::SE_MAX_BLOCKS) return hipErrorInvalidValue;
  tp::se_wgrad_k<<<tp::ceil_div(nw, 256), 256, 0, st>>>(a, m, dw, db, B, R, K, s0, s1, tp::FastDiv((unsigned)K));
  return hipGetLastError();
}
