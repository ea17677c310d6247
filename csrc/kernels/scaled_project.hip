// Channel-scaled 1x1 project GEMM for Monte-Carlo Shapley values behind a squeeze-and-excitation gate
// (engine/mobilenet_engine.py: MobileNetV3Engine.prefix_logits).
//
//   out[j, n, :] = (a[n, :] * sc[j, n / HW, :]) @ wt + bias[j, n / HW, :] (+ res[n, :]),  j < cnt, n < N = B * HW
//
// a (N, C) is the block's hidden activation, shared by all cnt prefix copies; what a copy changes (its masked
// channels and its gate) is a (B, C) scale and a (B, Co) bias, so the cnt masked, gated copies of the hidden
// activation are never written or read.
//
// Loop nest. A block owns a tile of BM = 32 * WM pixel rows by SP_BN = 64 output columns for one group of
// SP_JC = 4 copies (further groups are further blocks over the same tile: a then comes from L2 / MALL). Its
// 2 * WM waves each own 32 rows x 32 columns and SP_JC accumulators of 16 registers. The K slices (SP_BK = 16
// channels) of a and wt go global -> registers -> LDS, double buffered, one barrier per slice. The product is
// formed transposed, out^T = wt^T (a * sc)^T, on v_mfma_f32_32x32x2_f32: its first operand is wt[k][column],
// its second a[row][k] * sc, so a lane ends up with 4 x 4 consecutive output columns of ONE pixel row and
// stores float4s. K is permuted inside an 8-channel group so that a lane's four a values are one 16-byte LDS
// read: the lanes of half lh use channels 4 lh .. 4 lh + 3 of the group in MFMA steps 0 .. 3 (both operands
// alike, so the sum is the same set of products in a fixed order). Per step the wt fragment is read once and
// feeds SP_JC MFMAs; before each the a value is multiplied by that copy's sc value, the one VALU op per MFMA.
//
// sc is read straight from L2: a lane's pixel row, hence its image, is fixed for the whole K walk, so its sc
// address is a per-lane base computed once plus wave-uniform offsets, and the slice's values are SP_JC * 2
// 16-byte loads issued one slice ahead with the a / wt staging loads. (Staging them through LDS needs a tile
// per image; with HW = 1 that is one per row, 2 * SP_JC * BM * SP_BK floats = 32 KB for the large tile.)
//
// No split-K, no atomics: one writer per output element, one summation order, equal bits on every launch.
// Edges: rows past N, channels past C and columns past Co are zero-filled in the loads and not stored.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950) are recorded in
// profiles/mobilenet_v3/shapley_engine_vs_hook.txt.
#include "tp_common.h"
#include "tp_launchers.h"

namespace tp {

constexpr int SP_JC = 4;            // copies per pass: 4 x 16 accumulator registers
constexpr int SP_BK = 16;           // channels per K slice: two groups of 8
constexpr int SP_BN = 64;           // output columns per tile
constexpr int SP_LDA = SP_BK + 4;   // 20: the 16-byte reads of 16 consecutive rows cover all 64 banks once
constexpr int SP_LDB = SP_BN + 8;   // 72: rows k and k + 4 (the two lane halves) fall 32 banks apart
constexpr int SP_FILL_BLOCKS = 512; // large-tile blocks (two per CU) below which the row tile is halved

struct SpArgs {
  const float* a;
  const float* sc;
  const float* wt;
  const float* bias;
  const float* res;
  float* out;
  int N, C, Co, B, cnt;
  int row_tiles, col_tiles;
  FastDiv hw;
};

template <int WM>
__global__ __launch_bounds__(128 * WM) void scaled_project_k(SpArgs p) {
  constexpr int BM = 32 * WM, NT = 128 * WM;
  constexpr int B_CH = (SP_BK * SP_BN / 4) / NT;  // wt float4s a thread stages per slice
  static_assert(BM * SP_BK / 4 == NT && B_CH * NT == SP_BK * SP_BN / 4, "tile/thread mapping");
  __shared__ __attribute__((aligned(16))) float sA[2][BM * SP_LDA];
  __shared__ __attribute__((aligned(16))) float sB[2][SP_BK * SP_LDB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  // column tiles fastest: the blocks that share a row tile of a run next to one another
  const int ct = blockIdx.x % p.col_tiles, t = blockIdx.x / p.col_tiles;
  const int rt = t % p.row_tiles, jg = t / p.row_tiles;
  const int rb = rt * BM, cb = ct * SP_BN, j0 = jg * SP_JC;
  const int nj = min(SP_JC, p.cnt - j0);  // 1 .. SP_JC, uniform
  const int C = p.C, Co = p.Co, N = p.N;

  // the lane's pixel row and image, fixed for the whole K walk
  const int n = rb + wr * 32 + li;
  const int img = p.hw.div(min(n, N - 1));
  const float* scp = p.sc + ((long long)j0 * p.B + img) * C + lh * 4;
  const long long sc_copy = (long long)p.B * C;

  // staging roles
  const int a_row = tid >> 2, a_k = (tid & 3) * 4;
  const bool a_ok = rb + a_row < N;
  const float* ap = p.a + (long long)min(rb + a_row, N - 1) * C + a_k;

  float4 ra, rw[B_CH];
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load = [&](int sl, float4 (&scv)[SP_JC][2]) {
    const int k0 = sl * SP_BK;
    ra = zero4;
    if (a_ok && k0 + a_k < C) ra = *reinterpret_cast<const float4*>(ap + k0);
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int idx = tid + i * NT;
      const int k = k0 + idx / (SP_BN / 4), c = cb + (idx % (SP_BN / 4)) * 4;
      rw[i] = zero4;
      if (k < C && c < Co) rw[i] = *reinterpret_cast<const float4*>(p.wt + (long long)k * Co + c);
    }
#pragma unroll
    for (int j = 0; j < SP_JC; ++j)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int k = k0 + g * 8;  // + 4 lh inside scp
        scv[j][g] = zero4;
        if (j < nj && k + lh * 4 < C) scv[j][g] = *reinterpret_cast<const float4*>(scp + j * sc_copy + k);
      }
  };
  auto store = [&](int buf) {
    *reinterpret_cast<float4*>(&sA[buf][a_row * SP_LDA + a_k]) = ra;
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int idx = tid + i * NT;
      *reinterpret_cast<float4*>(&sB[buf][(idx / (SP_BN / 4)) * SP_LDB + (idx % (SP_BN / 4)) * 4]) = rw[i];
    }
  };

  f32x16 acc[SP_JC];
#pragma unroll
  for (int j = 0; j < SP_JC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  auto compute = [&](int buf, const float4 (&scv)[SP_JC][2]) {
    const float* la = &sA[buf][(wr * 32 + li) * SP_LDA + lh * 4];
    const float* lb = &sB[buf][(lh * 4) * SP_LDB + wc * 32 + li];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const float4 av4 = *reinterpret_cast<const float4*>(la + g * 8);
      const float av[4] = {av4.x, av4.y, av4.z, av4.w};
      float w[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) w[s] = lb[(g * 8 + s) * SP_LDB];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < SP_JC; ++j)
          if (j < nj) {
            const float4 s4 = scv[j][g];
            const float sv = s == 0 ? s4.x : s == 1 ? s4.y : s == 2 ? s4.z : s4.w;
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s], av[s] * sv, acc[j], 0, 0, 0);
          }
    }
  };

  // two named sets of sc values, the slice loop unrolled by two: no register moves between slices
  float4 sc0[SP_JC][2], sc1[SP_JC][2];
  const int ns = (C + SP_BK - 1) / SP_BK;
  load(0, sc0);
  store(0);
  __syncthreads();
  for (int sl = 0; sl < ns; sl += 2) {
    const bool more1 = sl + 1 < ns;
    if (more1) load(sl + 1, sc1);
    compute(0, sc0);
    if (!more1) break;
    store(1);
    __syncthreads();
    const bool more2 = sl + 2 < ns;
    if (more2) load(sl + 2, sc0);
    compute(1, sc1);
    if (more2) store(0);
    __syncthreads();
  }

  if (n >= N) return;
#pragma unroll
  for (int j = 0; j < SP_JC; ++j) {
    if (j >= nj) continue;
    const float* bj = p.bias + ((long long)(j0 + j) * p.B + img) * Co;
    float* oj = p.out + ((long long)(j0 + j) * N + n) * Co;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = cb + wc * 32 + q * 8 + lh * 4;
      if (co < Co) {
        const float4 b4 = *reinterpret_cast<const float4*>(bj + co);
        float4 v = make_float4(acc[j][4 * q] + b4.x, acc[j][4 * q + 1] + b4.y, acc[j][4 * q + 2] + b4.z,
                               acc[j][4 * q + 3] + b4.w);
        if (p.res != nullptr) {
          const float4 r4 = *reinterpret_cast<const float4*>(p.res + (long long)n * Co + co);
          v.x += r4.x;
          v.y += r4.y;
          v.z += r4.z;
          v.w += r4.w;
        }
        *reinterpret_cast<float4*>(oj + co) = v;
      }
    }
  }
}

}  // namespace tp

// a (N, C), sc (cnt, B, C), wt (C, Co), bias (cnt, B, Co), res (N, Co) or null, out (cnt, N, Co); N = B * HW.
// Rejected before any GPU work: null operands (res may be null), empty shapes, cnt < 1, HW < 1, N != B * HW,
// C % 4 or Co % 4 non-zero, any operand off a 16-byte boundary, any operand of 2^31 bytes or more.
extern "C" hipError_t tp_scaled_project(const float* a, const float* sc, const float* wt, const float* bias,
                                        const float* res, float* out, int N, int C, int Co, int B, int HW, int cnt,
                                        hipStream_t st) {
  if (N < 1 || C < 4 || Co < 4 || C % 4 != 0 || Co % 4 != 0) return hipErrorInvalidValue;
  if (cnt < 1 || HW < 1 || B < 1 || (long long)B * HW != N) return hipErrorInvalidValue;
  if (a == nullptr || sc == nullptr || wt == nullptr || bias == nullptr || out == nullptr) return hipErrorInvalidValue;
  if ((((uintptr_t)a | (uintptr_t)sc | (uintptr_t)wt | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)out) & 15) != 0)
    return hipErrorInvalidValue;
  const long long lim = 1ll << 31;
  if (N >= (1 << 29) || C >= (1 << 29) || Co >= (1 << 29) || cnt >= (1 << 29)) return hipErrorInvalidValue;
  const long long copy = (long long)N * Co * 4;  // factors below 2^29: every product below 2^60
  if (copy >= lim || (long long)N * C * 4 >= lim || (long long)C * Co * 4 >= lim) return hipErrorInvalidValue;
  if (copy * cnt >= lim || (long long)B * C * 4 * cnt >= lim || (long long)B * Co * 4 * cnt >= lim)
    return hipErrorInvalidValue;
  tp::SpArgs p;
  p.a = a, p.sc = sc, p.wt = wt, p.bias = bias, p.res = res, p.out = out;
  p.N = N, p.C = C, p.Co = Co, p.B = B, p.cnt = cnt;
  p.hw = tp::FastDiv((unsigned)HW);
  p.col_tiles = (Co + tp::SP_BN - 1) / tp::SP_BN;
  const long long groups = (cnt + tp::SP_JC - 1) / tp::SP_JC;
  // out < 2^31 bytes: N * Co * cnt < 2^29, so the tile count stays far below the grid limit
  const long long big = (long long)((N + 63) / 64) * p.col_tiles * groups;
  if (big >= tp::SP_FILL_BLOCKS) {
    p.row_tiles = (N + 63) / 64;
    tp::scaled_project_k<2><<<(unsigned)big, 256, 0, st>>>(p);
  } else {  // a grid that would leave CUs idle: half the row tile, twice the blocks
    p.row_tiles = (N + 31) / 32;
    tp::scaled_project_k<1><<<(unsigned)((long long)p.row_tiles * p.col_tiles * groups), 128, 0, st>>>(p);
  }
  return hipGetLastError();
}
