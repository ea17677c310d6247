// SiLU prefix-scan 1x1 project GEMM for Monte-Carlo Shapley values at the expand SiLU of a Fused-MBConv
// block (engine/mobilenet_engine.py: EfficientNetEngine.prefix_logits). The engine keeps the 3x3 expand
// conv's PRE-activation z and never writes silu(z); copy j of the block output masks the channels whose
// rank in the permutation is below p0 + j:
//
//   out[j, n, :] = sum_c [rank[c] >= p0 + j] silu(z[n, c]) wt[c, :] + shift (+ res[n, :]),  j < cnt, n < N
//
// z (N, C), wt (C, Co) with the BN scale folded in, rank (C,) over the padded width (padding ranks after
// every real channel: never masked), perm its inverse over the real channels. Copy j + 1 differs from copy
// j by the one channel perm[p0 + j], so ONE launch does both halves and no base tensor is written and read
// back:
//
//   1. copy 0 is a GEMM over C. A block owns XP_BM = 64 pixel rows by ALL Co <= 128 columns (as
//      silu_project_fwd: four 32-column accumulators of 16 registers per wave, two waves of 32 rows). A K
//      slice is 32 channels: 8 lanes read one 128-byte line of a z row; on the way into the LDS an element
//      becomes rank[c] < p0 ? 0 : silu(z) (one exponential per staged element). The product is formed
//      transposed on v_mfma_f32_32x32x2_f32 (first operand wt[k][column], second silu(z)[row][k], K permuted
//      inside a group of 8 as in scaled_project.hip), so a lane ends with 4 x 4 consecutive columns per
//      accumulator of ONE pixel row. shift and res are added to the registers once.
//   2. the accumulators stay in registers and take the cnt - 1 rank-1 steps
//        acc -= silu(z[row, c]) * wt[c, :],  c = perm[p0 + s] (clamped below C)
//      in sequence: ONE delta per lane and step. The deltas of a tile of XP_STEPS steps are gathered from z
//      and activated once, by lanes that run over the steps of one row, and staged through the LDS as a
//      (steps x rows) tile; the step's wt row is uniform over the block and comes from L1.
//   3. every copy goes registers -> LDS tile -> global: the block's rows are one contiguous range of
//      64 * Co floats of the copy, written as consecutive float4s, whole 128-byte lines.
//
// LDS: the operand stage of the GEMM (2 x A, 2 x B, double buffered, one barrier per slice) is dead after
// it and holds the output tile (pitch columns + 4) and the delta tile (pitch XP_BM + 1) afterwards.
//
// One summation order per element: the GEMM's, then shift, res, then the steps in sequence. No atomics, no
// split-K: equal bits on every launch. Edges: rows past N, slice channels past C and columns past Co are
// zero-filled in the loads (silu(0) = 0) and not stored. sigmoid(v) = rcp(1 + exp(-v)) is 0 at v = -100
// (the exponential overflows to +inf) and 1 at +100: finite products there, as in silu_project.hip.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): profiles/mobilenet/efficientnet_shapley.txt.
#include "tp_common.h"
#include "tp_launchers.h"

namespace tp {

constexpr int XP_BM = 64;              // rows per block: two waves of 32
constexpr int XP_NT = 128;
constexpr int XP_BK = 32;              // channels per K slice: one 128-byte line of a row
constexpr int XP_LDA = XP_BK + 4;      // the 16-byte reads of 16 consecutive rows cover the 64 banks once
constexpr int XP_MAX_CO = 128;         // 4 accumulators of 16 registers per wave
constexpr int XP_A_CH = XP_BM * XP_BK / 4 / XP_NT;  // z float4s a thread stages per slice (4)
constexpr int XP_STEPS = 32;           // steps per LDS delta tile: a wave's half gathers 32 channels of one row
constexpr int XP_LDD = XP_BM + 1;      // odd: the 32 steps a half-wave stages fall on 32 banks

__device__ __forceinline__ float xp_silu(float v) { return v * __builtin_amdgcn_rcpf(1.f + __expf(-v)); }

struct XpArgs {
  const float* z;
  const float* wt;
  const float* shift;
  const float* res;
  const int* perm;
  const int* rank;
  float* out;
  int N, C, Co, p0, cnt;
  FastDiv co4;
};

template <int NCT>
__global__ __launch_bounds__(XP_NT) void silu_prefix_project_k(XpArgs p) {
  constexpr int LDB = NCT * 32 + 8, LDO = NCT * 32 + 4, B_CH = XP_BK * NCT * 8 / XP_NT;
  constexpr int STAGE = 2 * XP_BM * XP_LDA + 2 * XP_BK * LDB;
  static_assert(XP_BM * LDO + XP_STEPS * XP_LDD <= STAGE, "the output and delta tiles reuse the operand stage");
  static_assert(XP_STEPS == 32 && XP_NT == 4 * XP_STEPS, "delta staging: thread -> (step tid & 31, rows tid >> 5 + 4 i)");
  __shared__ __attribute__((aligned(16))) float smem[STAGE];
  __shared__ int cs[XP_STEPS];  // the tile's channels

  const int tid = threadIdx.x, lane = tid & 63, wr = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int C = p.C, Co = p.Co, p0 = p.p0;
  const int rb = blockIdx.x * XP_BM, rows = min(XP_BM, p.N - rb);
  const float* zb = p.z + (long long)rb * C;

  // ---------------------------------------------------------------- 1. the masked GEMM (copy 0)
  float* sA = smem;
  float* sB = smem + 2 * XP_BM * XP_LDA;
  const int a_row = tid >> 3, a_k = (tid & 7) * 4;  // + 16 i rows
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ra[XP_A_CH], rw[B_CH];
  int4 rk;
  auto load = [&](int k0) {
    const bool k_ok = k0 + a_k < C;
    rk = make_int4(0, 0, 0, 0);
    if (k_ok) rk = *reinterpret_cast<const int4*>(p.rank + k0 + a_k);
#pragma unroll
    for (int i = 0; i < XP_A_CH; ++i) {
      const int r = a_row + 16 * i;
      ra[i] = zero4;
      if (r < rows && k_ok) ra[i] = *reinterpret_cast<const float4*>(zb + (long long)r * C + k0 + a_k);
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int idx = tid + i * XP_NT;
      const int k = k0 + idx / (NCT * 8), c = (idx % (NCT * 8)) * 4;
      rw[i] = zero4;
      if (k < C && c < Co) rw[i] = *reinterpret_cast<const float4*>(p.wt + (long long)k * Co + c);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XP_A_CH; ++i) {
      const float4 v = ra[i];  // silu(0) == 0: the fill stays 0
      *reinterpret_cast<float4*>(&sA[buf * XP_BM * XP_LDA + (a_row + 16 * i) * XP_LDA + a_k]) =
          make_float4(rk.x < p0 ? 0.f : xp_silu(v.x), rk.y < p0 ? 0.f : xp_silu(v.y), rk.z < p0 ? 0.f : xp_silu(v.z),
                      rk.w < p0 ? 0.f : xp_silu(v.w));
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int idx = tid + i * XP_NT;
      *reinterpret_cast<float4*>(&sB[buf * XP_BK * LDB + (idx / (NCT * 8)) * LDB + (idx % (NCT * 8)) * 4]) = rw[i];
    }
  };

  f32x16 acc[NCT];
#pragma unroll
  for (int t = 0; t < NCT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int nsl = (C + XP_BK - 1) / XP_BK;
  load(0);
  store(0);
  __syncthreads();
  for (int sl = 0; sl < nsl; ++sl) {
    const int buf = sl & 1;
    const bool more = sl + 1 < nsl;  // block-uniform
    if (more) load((sl + 1) * XP_BK);
    const float* la = &sA[buf * XP_BM * XP_LDA + (wr * 32 + li) * XP_LDA + lh * 4];
    const float* lb = &sB[buf * XP_BK * LDB + (lh * 4) * LDB + li];
#pragma unroll
    for (int g = 0; g < XP_BK / 8; ++g) {
      const float4 av4 = *reinterpret_cast<const float4*>(la + g * 8);
      const float av[4] = {av4.x, av4.y, av4.z, av4.w};
#pragma unroll
      for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(lb[(g * 8 + s) * LDB + t * 32], av[s], acc[t], 0, 0, 0);
    }
    if (more) store(buf ^ 1);
    __syncthreads();  // also: the stage is dead after the last slice
  }

  // a lane holds columns t * 32 + q * 8 + lh * 4 .. + 3 (t < NCT, q < 4) of row wr * 32 + li
  const int row = wr * 32 + li;
  {
    const bool with_res = p.res != nullptr && row < rows;
    const long long ro = (long long)(rb + row) * Co;
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = t * 32 + q * 8 + lh * 4;
        if (col < Co) {
          const float4 sh = *reinterpret_cast<const float4*>(p.shift + col);
          acc[t][4 * q] += sh.x, acc[t][4 * q + 1] += sh.y, acc[t][4 * q + 2] += sh.z, acc[t][4 * q + 3] += sh.w;
          if (with_res) {
            const float4 r4 = *reinterpret_cast<const float4*>(p.res + ro + col);
            acc[t][4 * q] += r4.x, acc[t][4 * q + 1] += r4.y, acc[t][4 * q + 2] += r4.z, acc[t][4 * q + 3] += r4.w;
          }
        }
      }
  }

  // ---------------------------------------------------------------- 3. a copy: registers -> LDS -> whole lines
  float* so = smem;
  float* dl = smem + XP_BM * LDO;
  const int co4 = Co >> 2, total = rows * co4;  // the tile's rows are one contiguous range of a copy
  const long long copy = (long long)p.N * Co;
  float* ob = p.out + (long long)rb * Co;
  auto emit = [&](int j) {
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(&so[row * LDO + t * 32 + q * 8 + lh * 4]) =
            make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]);
    __syncthreads();
    float* oj = ob + j * copy;
    for (int f = tid; f < total; f += XP_NT) {
      const int r = p.co4.div(f), c = (f - r * co4) * 4;
      *reinterpret_cast<float4*>(oj + 4 * f) = *reinterpret_cast<const float4*>(&so[r * LDO + c]);
    }
    __syncthreads();  // the tile (and, after a step tile's last copy, cs and dl) may be rewritten
  };
  emit(0);

  // ---------------------------------------------------------------- 2. the rank-1 steps
  const int ds = tid & (XP_STEPS - 1), dr = tid >> 5;  // delta staging: one step, rows dr + 4 i
  for (int s0 = 0; s0 < p.cnt - 1; s0 += XP_STEPS) {
    const int ns = min(XP_STEPS, p.cnt - 1 - s0);  // block-uniform
    if (tid < ns) cs[tid] = (int)min((unsigned)p.perm[p0 + s0 + tid], (unsigned)(C - 1));  // never index past a row
    __syncthreads();
    if (ds < ns) {
      const int c = cs[ds];
#pragma unroll 4
      for (int i = 0; i < XP_BM / 4; ++i) {
        const int r = dr + 4 * i;
        dl[ds * XP_LDD + r] = r < rows ? xp_silu(zb[(long long)r * C + c]) : 0.f;
      }
    }
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
      const float* wrow = p.wt + (long long)__builtin_amdgcn_readfirstlane(cs[s]) * Co;
      const float d = dl[s * XP_LDD + row];
#pragma unroll
      for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = t * 32 + q * 8 + lh * 4;
          if (col < Co) {
            const float4 w = *reinterpret_cast<const float4*>(wrow + col);
            acc[t][4 * q] -= d * w.x, acc[t][4 * q + 1] -= d * w.y, acc[t][4 * q + 2] -= d * w.z,
                acc[t][4 * q + 3] -= d * w.w;
          }
        }
      emit(s0 + s + 1);
    }
  }
}

}  // namespace tp

// z (N, C), wt (C, Co), shift (Co), res (N, Co) or null, perm (n <= C) int32, rank (C) int32, out (cnt, N, Co).
// Rejected before any GPU work: null operands (res may be null), empty shapes, C % 4 or Co % 4 non-zero,
// Co > 128, cnt < 1, p0 < 0, n > C, p0 + cnt - 1 > n, float4 / int4 operands off a 16-byte boundary (perm off a
// 4-byte one), any operand of 2^31 bytes or more.
extern "C" hipError_t tp_silu_prefix_project(const float* z, const float* wt, const float* shift, const float* res,
                                             const int* perm, const int* rank, float* out, int N, int C, int Co, int n,
                                             int p0, int cnt, hipStream_t st) {
  using namespace tp;
  if (N < 1 || C < 4 || Co < 4 || C % 4 != 0 || Co % 4 != 0 || Co > XP_MAX_CO) return hipErrorInvalidValue;
  if (cnt < 1 || p0 < 0 || n < 0 || n > C || (long long)p0 + cnt - 1 > n) return hipErrorInvalidValue;
  if (z == nullptr || wt == nullptr || shift == nullptr || perm == nullptr || rank == nullptr || out == nullptr)
    return hipErrorInvalidValue;
  if ((((uintptr_t)z | (uintptr_t)wt | (uintptr_t)shift | (uintptr_t)res | (uintptr_t)rank | (uintptr_t)out) & 15) != 0 ||
      ((uintptr_t)perm & 3) != 0)
    return hipErrorInvalidValue;
  const long long lim = 1ll << 29;  // floats of 2^31 bytes
  if (N >= lim || C >= lim) return hipErrorInvalidValue;  // Co <= 128, cnt <= C + 1: every product below 2^63
  if ((long long)N * C >= lim || (long long)C * Co >= lim || (long long)N * Co * cnt >= lim) return hipErrorInvalidValue;
  XpArgs p;
  p.z = z, p.wt = wt, p.shift = shift, p.res = res, p.perm = perm, p.rank = rank, p.out = out;
  p.N = N, p.C = C, p.Co = Co, p.p0 = p0, p.cnt = cnt;
  p.co4 = FastDiv((unsigned)(Co / 4));
  const unsigned blocks = ceil_div(N, XP_BM);
  if (Co <= 32)
    silu_prefix_project_k<1><<<blocks, XP_NT, 0, st>>>(p);
  else if (Co <= 64)
    silu_prefix_project_k<2><<<blocks, XP_NT, 0, st>>>(p);
  else
    silu_prefix_project_k<4><<<blocks, XP_NT, 0, st>>>(p);
  return hipGetLastError();
}
