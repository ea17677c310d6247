// Prefix-scan 1x1 project conv for Monte-Carlo Shapley values on inverted-residual blocks
// (engine/mobilenet_engine.py: MobileNetEngine.prefix_logits).
//
// Copy j of a block's hidden activation differs from copy j-1 by ONE channel c = perm[p0+j-1] being
// replaced by its fill value, and the project conv is linear, so the K stacked project outputs are a
// running rank-1 subtraction per pixel row:
//
//   out[0] = base
//   out[j] = out[j-1] - (a[:, c] - fill[c]) (x) wt[c, :],   c = perm[p0 + j - 1],  j = 1 .. cnt-1
//
// base (N, Co) is the project output of the copy masked up to p0, a (N, C) the unmasked hidden
// activation, wt (C, Co) the BN-scale-folded transposed weights. cnt * Co FMAs per pixel instead of
// the cnt * C * Co of a GEMM over cnt masked copies, and the 6x wider hidden copies never exist.
//
// A thread owns one float4 of one pixel row and keeps it in registers across the cnt steps; the
// block's 256 (64 on a small grid) float4s are consecutive in memory, so every store instruction
// writes whole lines. The step's channel is the same for the whole grid: the wt row and fill[c] are
// uniform. The per-pixel deltas a[n, c] - fill[c] are the only gathers: a block stages its
// (pixel rows x steps) tile of them through LDS once instead of once per float4 of the row. (Staging
// the tile's wt rows through LDS as well was measured: it shortens the tiles and ran 1.2x - 3.6x
// slower on narrow feature maps.) The order of the subtractions is the sequential one above for every
// element: no atomics, the same bits on every run.
#include "tp_common.h"
#include "tp_launchers.h"

namespace tp {

constexpr int PP_THREADS = 256;      // float4s of a block; PP_SMALL of them where the grid would not fill the chip
constexpr int PP_SMALL = 64;
constexpr int PP_SMALL_BELOW = 512;  // blocks of PP_THREADS (two per CU) below which the grid is cut four times finer
constexpr int PP_STEPS = 256;        // most steps per LDS tile (their channels are staged too)

template <int TH>
__global__ __launch_bounds__(TH) void prefix_project_k(const float4* __restrict__ base,
                                                               const float* __restrict__ a,
                                                               const float* __restrict__ fill,
                                                               const float4* __restrict__ wt,
                                                               const int* __restrict__ perm, float4* __restrict__ out,
                                                               int N, int C, int Q, int p0, int cnt) {
  constexpr int TILE = (TH + 1) * 16;  // delta floats per LDS tile: <= TH pixel rows (pitch <= TH + 1) -> >= 16 steps
  __shared__ float dl[TILE];
  __shared__ int cs[PP_STEPS];
  const int tid = threadIdx.x;
  const int items = N * Q;  // float4s of one copy (< 2^27: the launcher bounds every operand)
  const int item0 = blockIdx.x * TH;
  const int item = item0 + tid;
  const bool live = item < items;
  const int pix0 = item0 / Q;
  const int np = (min(item0 + TH, items) - 1) / Q - pix0 + 1;  // pixel rows of this block, 1 .. TH
  const int pitch = np | 1;  // odd: the staging stores of consecutive steps fall on different banks
  const int jc = min(TILE / pitch, PP_STEPS);
  const int pix = live ? item / Q : pix0;
  const int q = live ? item - pix * Q : 0;
  const int pl = pix - pix0;

  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    acc = base[item];
    out[item] = acc;
  }
  for (int s0 = 0; s0 < cnt - 1; s0 += jc) {
    const int ns = min(jc, cnt - 1 - s0);
    __syncthreads();  // the previous tile has been consumed
    for (int i = tid; i < ns; i += TH)
      cs[i] = (int)min((unsigned)perm[p0 + s0 + i], (unsigned)(C - 1));  // never index past a row
    __syncthreads();
    // lanes run over the steps of one pixel row: its gathers stay inside that row's C floats
    for (int i = tid; i < np * ns; i += TH) {
      const int p = i / ns, s = i - p * ns;
      const int c = cs[s];
      dl[s * pitch + p] = a[(pix0 + p) * C + c] - fill[c];
    }
    __syncthreads();
    if (live) {
      float4 w = wt[cs[0] * Q + q];
      for (int s = 0; s < ns; ++s) {
        const float4 wn = wt[cs[min(s + 1, ns - 1)] * Q + q];  // next step's row, in flight over this step
        const float d = dl[s * pitch + pl];
        acc.x -= d * w.x;
        acc.y -= d * w.y;
        acc.z -= d * w.z;
        acc.w -= d * w.w;
        out[(s0 + s + 1) * items + item] = acc;
        w = wn;
      }
    }
  }
}

}  // namespace tp

// base (N, Co), a (N, C), fill (C), wt (C, Co), perm (n) int32 with values in [0, C), out (cnt, N, Co).
// Rejected before any GPU work: Co % 4 != 0, empty shapes, cnt < 1, p0 < 0, p0 + cnt - 1 > n, n > C,
// null operands, float4 operands off a 16-byte boundary (scalar ones off a 4-byte boundary), any operand
// of 2^31 bytes or more.
extern "C" hipError_t tp_prefix_project(const float* base, const float* a, const float* fill, const float* wt,
                                        const int* perm, float* out, int N, int C, int Co, int n, int p0, int cnt,
                                        hipStream_t st) {
  if (N < 1 || C < 1 || Co < 4 || Co % 4 != 0) return hipErrorInvalidValue;
  if (cnt < 1 || p0 < 0 || n < 0 || n > C) return hipErrorInvalidValue;
  if ((long long)p0 + cnt - 1 > n) return hipErrorInvalidValue;
  if (base == nullptr || a == nullptr || fill == nullptr || wt == nullptr || perm == nullptr || out == nullptr)
    return hipErrorInvalidValue;
  if ((((uintptr_t)base | (uintptr_t)wt | (uintptr_t)out) & 15) != 0 ||
      (((uintptr_t)a | (uintptr_t)fill | (uintptr_t)perm) & 3) != 0)
    return hipErrorInvalidValue;
  const long long lim = 1ll << 31;
  if (N >= (1 << 29) || C >= (1 << 29) || Co >= (1 << 29)) return hipErrorInvalidValue;  // products below 2^60
  const long long copy = (long long)N * Co * 4;
  if (copy >= lim || (long long)N * C * 4 >= lim || (long long)C * Co * 4 >= lim) return hipErrorInvalidValue;
  if (copy * cnt >= lim) return hipErrorInvalidValue;  // copy < 2^31, cnt < 2^31: below 2^63
  const long long items = (long long)N * (Co / 4);
  // a grid of few blocks leaves CUs idle for all cnt steps: one wave per block then
  if (items < (long long)tp::PP_SMALL_BELOW * tp::PP_THREADS)
    tp::prefix_project_k<tp::PP_SMALL><<<tp::ceil_div(items, tp::PP_SMALL), tp::PP_SMALL, 0, st>>>(
        (const float4*)base, a, fill, (const float4*)wt, perm, (float4*)out, N, C, Co / 4, p0, cnt);
  else
    tp::prefix_project_k<tp::PP_THREADS><<<tp::ceil_div(items, tp::PP_THREADS), tp::PP_THREADS, 0, st>>>(
        (const float4*)base, a, fill, (const float4*)wt, perm, (float4*)out, N, C, Co / 4, p0, cnt);
  return hipGetLastError();
}
