// SiLU-on-load 1x1 project GEMM of a Fused-MBConv block (EfficientNetV2's early stages: dense 3x3 expand,
// BN, SiLU, 1x1 project, BN), fp32 MFMA, and its data gradient (engine/mobilenet_engine.py:
// EfficientNetEngine). The hidden tensor is kept as the PRE-activation z; both kernels activate it as they
// read it, so the activated tensor and the gradient of the activation never exist in memory.
//
//   forward  out[n, :] = (silu(z[n, :]) @ wt) * scale + shift (+ res[n, :])      z (N, C), wt (C, Co)
//            apoz[n / HW, c] += [silu(z[n, c]) > 0]
//   dgrad    gy = g @ wtT                                                          g (N, Co), wtT (Co, C)
//            a = silu(z), d = s (1 + z (1 - s)), s = sigmoid(z): one exponential, one reciprocal
//            dz = gy * d;  tay[slot, n / HW, c] = sum over the block's rows of -(gy * a) or |gy|
//
// Both are short in one GEMM dimension and bound by the (N, C) tensor, so a block owns SJ_BM = 64 rows:
//
//   forward  64 rows x ALL Co columns (Co <= SJ_MAX_CO = 128: four 32-column accumulators of 16 registers
//            per wave), so every z element is loaded and activated once. A K slice is SJ_BK = 32 channels:
//            8 lanes read one 128-byte line of a z row, the SiLU runs in registers on the way into the LDS.
//   dgrad    64 rows x 64 of the C columns; the narrow g tile is re-read per column chunk (from L2), z is
//            read once, in the epilogue. gy never leaves the block.
//
// Two waves, each 32 rows x all of the block's columns. The product is formed transposed on
// v_mfma_f32_32x32x2_f32 (first operand B[k][column], second A[row][k]), so a lane ends with 4 x 4
// consecutive columns of ONE row. K is permuted inside a group of 8: the lanes of half lh take channels
// 4 lh .. 4 lh + 3 in steps 0 .. 3 (both operands alike), so a lane's four A values are one 16-byte LDS
// read. LDS pitches: A rows SJ_BK + 4 = 36 floats (the 16-byte reads of 16 consecutive rows cover the 64
// banks once), B rows columns + 8 (rows k and k + 4, the two lane halves, fall 32 banks apart), the output
// tile columns + 4. Both operands go global -> registers -> LDS, double buffered, one barrier per slice;
// the last slice is zero-filled in the loads.
//
// Epilogues go through the LDS (the operand stage is dead by then). Forward: the block's output is ONE
// contiguous range of 64 * Co floats, written as consecutive float4s (+ res at the same addresses).
// Dgrad: a thread takes one channel quad of 8 consecutive rows, 16 lanes cover the 256 bytes of a row
// chunk of z and dz.
//
// Score partials: one writer per (slot, image, channel), one summation order. A thread sums runs of its
// consecutive rows (a run ends where the image does) and leaves each run's sum at the run's first row in
// the LDS tile; then one thread per (image of the tile, channel quad) adds the run heads of its image in
// row order (the image's first row, then every multiple of 8 inside it) and stores into slot
// (tile - first tile of the image). An image of HW rows meets at most (HW - g + 63) / 64 + 1 tiles,
// g = gcd(HW, 64) (HW / 64 when 64 divides HW): the slot count. A tile may hold up to 64 images (HW = 1) or
// a 64th of one.
//
// APoZ counts are integers: LDS integer atomics per (image of the tile, channel of the slice), then one
// float atomic per non-zero count (exact up to 2^24, order-independent), as dwconv_silu.hip adds its.
// No float atomics on out, dz or tay.
//
// Numerics: sigmoid(v) = rcp(1 + exp(-v)) is 0 at v = -100 (exp overflows to +inf) and 1 at +100, so a, d
// and every product are finite there. Measured: profiles/numerics/silu_project.txt.
#include "tp_common.h"
#include "tp_launchers.h"

#include <initializer_list>

namespace tp {

constexpr int SJ_BM = 64;                 // rows per block: two waves of 32
constexpr int SJ_NT = 128;
constexpr int SJ_BK = 32;                  // channels per K slice: one 128-byte line of a row
constexpr int SJ_LDA = SJ_BK + 4;
constexpr int SJ_MAX_CO = 128;             // forward: 4 accumulators of 16 registers per wave
constexpr int SJ_BN = 64;                  // dgrad: columns per block
constexpr int SJ_A_CH = SJ_BM * SJ_BK / 4 / SJ_NT;  // A float4s a thread stages per slice (4)

__device__ __forceinline__ float sj_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.f + __expf(-v)); }
__device__ __forceinline__ float sj_silu(float v) { return v * sj_sigmoid(v); }
__device__ __forceinline__ void sj_silu_both(float v, float& a, float& d) {
  const float s = sj_sigmoid(v);
  a = v * s;
  d = s * fmaf(v, 1.f - s, 1.f);
}

template <int NCT>
constexpr int sj_stage_floats() {  // operand stage (2 x A, 2 x B), which the output tile then reuses
  return 2 * SJ_BM * SJ_LDA + 2 * SJ_BK * (NCT * 32 + 8);
}

// acc (the wave's 32 rows x NCT * 32 columns from column cb) = act(A[rb .. rb + 64, :K]) @ Bm[:K, cb ..]:
// A has `rows` valid rows of pitch lda from its pointer, Bm `ncols` columns (its pitch). ``seen(k0, i, row,
// k, a4)`` is called once per activated A float4 that lies inside the operand (ACT only). Ends on a barrier.
template <int NCT, bool ACT, class Seen, class Flush>
__device__ __forceinline__ void sj_gemm(const float* __restrict__ A, int lda, int rows, const float* __restrict__ Bm,
                                        int ncols, int cb, int K, float* smem, f32x16 (&acc)[NCT], Seen seen,
                                        Flush flush) {
  constexpr int LDB = NCT * 32 + 8, B_CH = SJ_BK * NCT * 8 / SJ_NT;
  float* sA = smem;
  float* sB = smem + 2 * SJ_BM * SJ_LDA;
  const int tid = threadIdx.x, lane = tid & 63, wr = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int a_row = tid >> 3, a_k = (tid & 7) * 4;  // + 16 i rows
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ra[SJ_A_CH], rw[B_CH];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < SJ_A_CH; ++i) {
      const int r = a_row + 16 * i;
      ra[i] = zero4;
      if (r < rows && k0 + a_k < K) ra[i] = *reinterpret_cast<const float4*>(A + (long long)r * lda + k0 + a_k);
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int idx = tid + i * SJ_NT;
      const int k = k0 + idx / (NCT * 8), c = cb + (idx % (NCT * 8)) * 4;
      rw[i] = zero4;
      if (k < K && c < ncols) rw[i] = *reinterpret_cast<const float4*>(Bm + (long long)k * ncols + c);
    }
  };
  auto store = [&](int buf, int k0) {
#pragma unroll
    for (int i = 0; i < SJ_A_CH; ++i) {
      const int r = a_row + 16 * i;
      float4 v = ra[i];
      if constexpr (ACT) {
        v = make_float4(sj_silu(v.x), sj_silu(v.y), sj_silu(v.z), sj_silu(v.w));  // silu(0) == 0: the fill stays 0
        if (r < rows && k0 + a_k < K) seen(r, a_k, v);
      }
      *reinterpret_cast<float4*>(&sA[buf * SJ_BM * SJ_LDA + r * SJ_LDA + a_k]) = v;
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int idx = tid + i * SJ_NT;
      *reinterpret_cast<float4*>(&sB[buf * SJ_BK * LDB + (idx / (NCT * 8)) * LDB + (idx % (NCT * 8)) * 4]) = rw[i];
    }
  };
#pragma unroll
  for (int t = 0; t < NCT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int ns = (K + SJ_BK - 1) / SJ_BK;
  load(0);
  store(0, 0);
  __syncthreads();
  for (int sl = 0; sl < ns; ++sl) {
    const int buf = sl & 1;
    const bool more = sl + 1 < ns;  // block-uniform
    if (more) load((sl + 1) * SJ_BK);
    const float* la = &sA[buf * SJ_BM * SJ_LDA + (wr * 32 + li) * SJ_LDA + lh * 4];
    const float* lb = &sB[buf * SJ_BK * LDB + (lh * 4) * LDB + li];
#pragma unroll
    for (int g = 0; g < SJ_BK / 8; ++g) {
      const float4 av4 = *reinterpret_cast<const float4*>(la + g * 8);
      const float av[4] = {av4.x, av4.y, av4.z, av4.w};
#pragma unroll
      for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(lb[(g * 8 + s) * LDB + t * 32], av[s], acc[t], 0, 0, 0);
    }
    flush(sl * SJ_BK);  // what `seen` gathered for this slice (after the barrier that published it)
    if (more) store(buf ^ 1, (sl + 1) * SJ_BK);
    __syncthreads();
  }
}

// The wave's accumulators -> the LDS tile so[row][column] (pitch NCT * 32 + 4), each value through
// ``fin(column, v)``; a lane holds columns t * 32 + q * 8 + lh * 4 .. + 3 of row wr * 32 + li.
template <int NCT, class Fin>
__device__ __forceinline__ void sj_spill(const f32x16 (&acc)[NCT], float* so, Fin fin) {
  constexpr int LDO = NCT * 32 + 4;
  const int lane = threadIdx.x & 63, wr = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int t = 0; t < NCT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = t * 32 + q * 8 + lh * 4;
      *reinterpret_cast<float4*>(&so[(wr * 32 + li) * LDO + col]) =
          fin(col, make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]));
    }
}

struct SjFwd {
  const float* z;
  const float* wt;
  const float* scale;
  const float* shift;
  const float* res;
  float* out;
  float* apoz;
  int N, C, Co, HW;
  FastDiv hw, co4;
};

template <int NCT>
__global__ __launch_bounds__(SJ_NT) void silu_project_fwd_k(SjFwd p) {
  constexpr int LDO = NCT * 32 + 4;
  static_assert(SJ_BM * LDO <= sj_stage_floats<NCT>(), "the output tile reuses the operand stage");
  __shared__ __attribute__((aligned(16))) float smem[sj_stage_floats<NCT>()];
  __shared__ int scnt[SJ_BM * SJ_BK];  // [image of the tile][channel of the slice]
  const int tid = threadIdx.x;
  const int rb = blockIdx.x * SJ_BM, rows = min(SJ_BM, p.N - rb);
  const bool count = p.apoz != nullptr;  // block-uniform
  const int b0 = p.hw.div(rb), nimg = p.hw.div(rb + rows - 1) - b0 + 1;
  if (count) {
    for (int e = tid; e < SJ_BM * SJ_BK; e += SJ_NT) scnt[e] = 0;
    __syncthreads();
  }
  auto seen = [&](int r, int k, float4 a) {
    if (!count) return;
    int* row = &scnt[(p.hw.div(rb + r) - b0) * SJ_BK + k];
    if (a.x > 0.f) atomicAdd(row + 0, 1);
    if (a.y > 0.f) atomicAdd(row + 1, 1);
    if (a.z > 0.f) atomicAdd(row + 2, 1);
    if (a.w > 0.f) atomicAdd(row + 3, 1);
  };
  auto flush = [&](int k0) {
    if (!count) return;
    for (int e = tid; e < nimg * SJ_BK; e += SJ_NT) {
      const int v = scnt[e];
      if (v != 0) {  // counted only for channels inside C
        scnt[e] = 0;
        atomicAdd(p.apoz + (long long)(b0 + e / SJ_BK) * p.C + k0 + e % SJ_BK, (float)v);
      }
    }
    __syncthreads();  // the table is clear before the next slice counts into it
  };
  f32x16 acc[NCT];
  sj_gemm<NCT, true>(p.z + (long long)rb * p.C, p.C, rows, p.wt, p.Co, 0, p.C, smem, acc, seen, flush);

  sj_spill<NCT>(acc, smem, [&](int col, float4 v) {
    if (col < p.Co) {
      const float4 sc = *reinterpret_cast<const float4*>(p.scale + col);
      const float4 sh = *reinterpret_cast<const float4*>(p.shift + col);
      v = make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w));
    }
    return v;
  });
  __syncthreads();
  // the tile's rows are one contiguous range of the output: consecutive float4s, full lines
  const int co4 = p.Co >> 2, total = rows * co4;
  const long long base = (long long)rb * p.Co;
  for (int f = tid; f < total; f += SJ_NT) {
    const int r = p.co4.div(f), c = (f - r * co4) * 4;
    float4 v = *reinterpret_cast<const float4*>(&smem[r * LDO + c]);
    if (p.res != nullptr) {
      const float4 r4 = *reinterpret_cast<const float4*>(p.res + base + 4ll * f);
      v.x += r4.x, v.y += r4.y, v.z += r4.z, v.w += r4.w;
    }
    *reinterpret_cast<float4*>(p.out + base + 4ll * f) = v;
  }
}

struct SjBwd {
  const float* g;
  const float* wtT;
  const float* z;
  float* dz;
  float* tay;
  int N, C, Co, B, HW, tay_mode, col_chunks;
  FastDiv hw;
};

__global__ __launch_bounds__(SJ_NT) void silu_project_dgrad_k(SjBwd p) {
  constexpr int NCT = SJ_BN / 32, LDO = SJ_BN + 4;
  static_assert(SJ_BM * LDO <= sj_stage_floats<NCT>(), "the gy tile reuses the operand stage");
  __shared__ __attribute__((aligned(16))) float smem[sj_stage_floats<NCT>()];
  const int tid = threadIdx.x;
  const int cc = blockIdx.x % p.col_chunks, rt = blockIdx.x / p.col_chunks;  // chunks of a row tile run together
  const int rb = rt * SJ_BM, cb = cc * SJ_BN, rows = min(SJ_BM, p.N - rb);
  f32x16 acc[NCT];
  sj_gemm<NCT, false>(p.g + (long long)rb * p.Co, p.Co, rows, p.wtT, p.C, cb, p.Co, smem, acc,
                      [](int, int, float4) {}, [](int) {});
  sj_spill<NCT>(acc, smem, [](int, float4 v) { return v; });
  __syncthreads();

  const bool part = p.tay != nullptr;  // block-uniform
  {
    const int c4 = tid & 15, rg = tid >> 4, c = cb + c4 * 4;
    if (c < p.C) {
      int head = -1;
      float4 run = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 0; i < 8; ++i) {
        const int r = rg * 8 + i, n = rb + r;
        if (r >= rows) break;
        const float4 gy = *reinterpret_cast<const float4*>(&smem[r * LDO + c4 * 4]);
        const long long o = (long long)n * p.C + c;
        const float4 zv = *reinterpret_cast<const float4*>(p.z + o);
        float4 a, d;
        sj_silu_both(zv.x, a.x, d.x), sj_silu_both(zv.y, a.y, d.y);
        sj_silu_both(zv.z, a.z, d.z), sj_silu_both(zv.w, a.w, d.w);
        *reinterpret_cast<float4*>(p.dz + o) = make_float4(gy.x * d.x, gy.y * d.y, gy.z * d.z, gy.w * d.w);
        if (part) {
          const float4 t = make_float4(tay_term(p.tay_mode, gy.x, a.x), tay_term(p.tay_mode, gy.y, a.y),
                                       tay_term(p.tay_mode, gy.z, a.z), tay_term(p.tay_mode, gy.w, a.w));
          if (i == 0 || p.hw.div(n) * p.HW == n) {  // a run starts at the thread's first row and with an image
            if (head >= 0) *reinterpret_cast<float4*>(&smem[head * LDO + c4 * 4]) = run;  // (a row already read)
            head = r, run = t;
          } else {
            run.x += t.x, run.y += t.y, run.z += t.z, run.w += t.w;
          }
        }
      }
      if (head >= 0) *reinterpret_cast<float4*>(&smem[head * LDO + c4 * 4]) = run;
    }
  }
  if (!part) return;
  __syncthreads();
  const int b0 = p.hw.div(rb), nimg = p.hw.div(rb + rows - 1) - b0 + 1;
  for (int q = tid; q < nimg * 16; q += SJ_NT) {
    const int b = b0 + (q >> 4), c4 = q & 15, c = cb + c4 * 4;
    if (c >= p.C) continue;
    const int s = max(b * p.HW, rb) - rb, e = min((b + 1) * p.HW, rb + rows) - rb;  // the image's rows of the tile
    float4 tot = *reinterpret_cast<const float4*>(&smem[s * LDO + c4 * 4]);
    for (int r = (s / 8 + 1) * 8; r < e; r += 8) {
      const float4 h = *reinterpret_cast<const float4*>(&smem[r * LDO + c4 * 4]);
      tot.x += h.x, tot.y += h.y, tot.z += h.z, tot.w += h.w;
    }
    const int slot = rt - (b * p.HW) / SJ_BM;
    *reinterpret_cast<float4*>(p.tay + ((long long)slot * p.B + b) * p.C + c) = tot;
  }
}

// shapes both launchers take: N = B * HW rows, C and Co multiples of 4, every operand below 2^31 bytes
static bool sj_shape_ok(int N, int C, int Co, int B, int HW) {
  if (N < 1 || C < 4 || Co < 4 || C % 4 != 0 || Co % 4 != 0 || B < 1 || HW < 1 || (long long)B * HW != N) return false;
  const long long lim = 1ll << 29;  // floats of 2^31 bytes
  return (long long)N * C < lim && (long long)N * Co < lim && (long long)C * Co < lim;
}

static bool sj_aligned(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* q : ps) bits |= (uintptr_t)q;
  return (bits & 15) == 0;
}

}  // namespace tp

// Slots R of the dgrad's (R, B, C) score-partial slab for images of HW rows; 0 for a rejected shape. An image
// starts at a multiple of g = gcd(HW, 64) inside its first tile, at 64 - g at the latest.
extern "C" int tp_silu_project_tay_slots(int HW, int C) {
  if (HW < 1 || C < 4 || C % 4 != 0) return 0;
  const int g = (HW & -HW) < tp::SJ_BM ? (HW & -HW) : tp::SJ_BM;
  return (int)(((long long)HW - g + tp::SJ_BM - 1) / tp::SJ_BM) + 1;
}

// out (N, Co) = (silu(z) @ wt) * scale + shift (+ res): z (N, C), wt (C, Co), scale / shift (Co), res (N, Co)
// or null; apoz (B, C) or null += counts of silu(z) > 0 per image of HW rows (N = B * HW; B = 1, HW = N
// without apoz). Rejected before any GPU work: null operands, C % 4 or Co % 4 non-zero, Co > 128, operands
// off a 16-byte boundary or of 2^31 bytes or more.
extern "C" hipError_t tp_silu_project_fwd(const float* z, const float* wt, const float* scale, const float* shift,
                                          const float* res, float* out, float* apoz, int N, int C, int Co, int B,
                                          int HW, hipStream_t st) {
  using namespace tp;
  if (!sj_shape_ok(N, C, Co, B, HW) || Co > SJ_MAX_CO) return hipErrorInvalidValue;
  if (z == nullptr || wt == nullptr || scale == nullptr || shift == nullptr || out == nullptr ||
      !sj_aligned({z, wt, scale, shift, res, out, apoz}))
    return hipErrorInvalidValue;
  SjFwd p;
  p.z = z, p.wt = wt, p.scale = scale, p.shift = shift, p.res = res, p.out = out, p.apoz = apoz;
  p.N = N, p.C = C, p.Co = Co, p.HW = HW;
  p.hw = FastDiv((unsigned)HW), p.co4 = FastDiv((unsigned)(Co / 4));
  const unsigned blocks = ceil_div(N, SJ_BM);
  if (Co <= 32)
    silu_project_fwd_k<1><<<blocks, SJ_NT, 0, st>>>(p);
  else if (Co <= 64)
    silu_project_fwd_k<2><<<blocks, SJ_NT, 0, st>>>(p);
  else
    silu_project_fwd_k<4><<<blocks, SJ_NT, 0, st>>>(p);
  return hipGetLastError();
}

// dz (N, C) = (g @ wtT) * silu'(z): g (N, Co), wtT (Co, C), z (N, C); tay (optional): a zeroed (R, B, C)
// slab, R = tp_silu_project_tay_slots(HW, C), of partial sums over rows of -(gy * silu(z)) (tay_mode 0)
// or |gy| (1) per image of HW rows (N = B * HW; B = 1, HW = N without tay). Rejections as the forward's
// (no limit on Co), plus a wrong R and a tay_mode outside 0 .. 1.
extern "C" hipError_t tp_silu_project_dgrad(const float* g, const float* wtT, const float* z, float* dz, float* tay,
                                            int R, int tay_mode, int N, int C, int Co, int B, int HW,
                                            hipStream_t st) {
  using namespace tp;
  if (!sj_shape_ok(N, C, Co, B, HW)) return hipErrorInvalidValue;
  if (g == nullptr || wtT == nullptr || z == nullptr || dz == nullptr || !sj_aligned({g, wtT, z, dz, tay}))
    return hipErrorInvalidValue;
  if (tay != nullptr && (tay_mode < 0 || tay_mode > 1 || R != tp_silu_project_tay_slots(HW, C) ||
                         (long long)R * B * C >= (1ll << 29)))
    return hipErrorInvalidValue;
  SjBwd p;
  p.g = g, p.wtT = wtT, p.z = z, p.dz = dz, p.tay = tay;
  p.N = N, p.C = C, p.Co = Co, p.B = B, p.HW = HW, p.tay_mode = tay_mode;
  p.col_chunks = (int)ceil_div(C, SJ_BN);
  p.hw = FastDiv((unsigned)HW);
  const long long blocks = (long long)ceil_div(N, SJ_BM) * p.col_chunks;  // N * C < 2^29: far below the grid limit
  silu_project_dgrad_k<<<(unsigned)blocks, SJ_NT, 0, st>>>(p);
  return hipGetLastError();
}
