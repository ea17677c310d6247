// Shared pieces of the depthwise-conv kernels (dwconv.hip, dwconv_act.hip): the channel-vector
// loads / stores, the register layout of a channel quad's taps, the column range of the gather
// form of the input gradient, and the host-side geometry checks of the launchers.
#pragma once
#include "tp_common.h"

namespace tp {

constexpr int DW_SW = 4;         // columns per thread (forward: output, dgrad: input)
constexpr int DW_SLICE = 64;     // most channels per wgrad block
constexpr int DW_FOLD_TAPS = 4;  // taps reduced through the LDS per round

template <int V>
struct DwVec;  // V channels per thread
template <>
struct DwVec<4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <>
struct DwVec<1> {
  static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float* v) { *p = v[0]; }
};

// the V * KK contiguous weights of channels [c, c + V) -> wf[v * KK + tap] (float4 loads for V = 4:
// 16 * KK bytes per quad, 16-byte aligned)
template <int V, int KK>
__device__ __forceinline__ void dw_load_w(const float* __restrict__ w, int c, float* wf) {
  const float* p = w + c * KK;
  if constexpr (V == 4) {
#pragma unroll
    for (int i = 0; i < KK; ++i) DwVec<4>::load(p + 4 * i, wf + 4 * i);
  } else {
#pragma unroll
    for (int i = 0; i < KK; ++i) wf[i] = p[i];
  }
}

// The g columns a strip of the gather-form input gradient needs (see dwconv_dgrad_k): for a strip
// whose (iw0 + pad) % S == PB they are ow = (iw0 + pad - PB) / S + d, d in [lo(), hi()].
template <int K, int S, int PB>
struct DwTaps {
  static constexpr int lo() {
    int m = 1 << 20;
    for (int j = 0; j < DW_SW; ++j)
      for (int kw = 0; kw < K; ++kw)
        if ((PB + j - kw) % S == 0 && (PB + j - kw) / S < m) m = (PB + j - kw) / S;
    return m;
  }
  static constexpr int hi() {
    int m = -(1 << 20);
    for (int j = 0; j < DW_SW; ++j)
      for (int kw = 0; kw < K; ++kw)
        if ((PB + j - kw) % S == 0 && (PB + j - kw) / S > m) m = (PB + j - kw) / S;
    return m;
  }
};

constexpr long long DW_MAX_BYTES = 1ll << 31;  // operands are indexed with 32-bit element offsets

// n * m * 4 bytes below 2^31 (n below it already): no overflow for any int arguments
static inline bool dw_grow(long long& n, int m) {
  if (m < 1) return false;
  n *= m;
  return n * 4 < DW_MAX_BYTES;
}

// geometry the kernels support; the output size and that every operand stays below 2^31 bytes
static inline bool dw_geometry(int B, int H, int W, int C, int k, int s, int pad, int* Ho, int* Wo) {
  if ((k != 3 && k != 5) || (s != 1 && s != 2) || pad < 0 || pad > k - 1) return false;
  if (B < 1 || H < 1 || W < 1 || C < 1) return false;
  long long nx = 1, ny = 1, nw = (long long)k * k;
  if (!(dw_grow(nx, B) && dw_grow(nx, H) && dw_grow(nx, W) && dw_grow(nx, C))) return false;
  if (H + 2 * pad < k || W + 2 * pad < k) return false;  // empty output
  *Ho = (H + 2 * pad - k) / s + 1, *Wo = (W + 2 * pad - k) / s + 1;
  if (!(dw_grow(ny, B) && dw_grow(ny, *Ho) && dw_grow(ny, *Wo) && dw_grow(ny, C))) return false;
  return dw_grow(nw, C);
}

static inline bool dw_aligned(int C, const void* a, const void* b, const void* c, const void* d = nullptr) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d;
  return (bits & (C % 4 == 0 ? 15 : 3)) == 0;
}

// a launch of 256-thread blocks stays below HIP's limit of 2^32 threads per grid
constexpr long long DW_MAX_BLOCKS = 1ll << 24;

// blocks of a (rows x strips x channel vectors) launch: rows * cpr, cpr blocks per image row
// (millions of rows of a few elements each, which would need more blocks than a grid takes, are
// rejected like any other unsupported shape)
static inline bool dw_row_grid(int rows, int cols, int C, int V, int* cpr, int* nq, long long* blocks) {
  const long long q = (long long)ceil_div(cols, DW_SW) * (C / V);
  if (q >= (1ll << 31)) return false;
  *nq = (int)q;
  *cpr = (int)ceil_div(q, 256);
  *blocks = (long long)rows * *cpr;
  return *blocks < DW_MAX_BLOCKS;
}

}  // namespace tp

#define TP_DW_KS(fn, ...)                      \
  do {                                         \
    if (k == 3 && s == 1) fn(3, 1, __VA_ARGS__); \
    else if (k == 3) fn(3, 2, __VA_ARGS__);    \
    else if (s == 1) fn(5, 1, __VA_ARGS__);    \
    else fn(5, 2, __VA_ARGS__);                \
  } while (0)
