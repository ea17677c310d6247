// Fused Winograd F(2x2, 3x3) convolution on fp32 MFMA (v_mfma_f32_16x16x4_f32), the
// 2.25x-fewer-multiplies algorithm MIOpen uses for fp32 3x3 convs, re-designed so that
// NOTHING but the input, the pre-transformed weights and the final output touch memory:
//
//   * a wave owns 16 output tiles (2x2 pixels each) x 32 output channels x all 16 transform
//     points xi; its 16*2 accumulator tiles (16x16, 4 regs) live in registers;
//   * per 8-channel chunk each lane fetches the 4x4 input patch of "its" tile (MFMA A-row =
//     lane&15) for 2 channels (A-k = lane>>4), forms V = B^T d B in registers (packed fp32
//     adds, both channels at once) and feeds the 16 V values straight into the MFMAs as the
//     A operand;
//   * the transformed weights U = G g G^T are pre-arranged on the host into the exact 16-KB
//     LDS image of one (8-channel chunk, 32-output-channel block) and DMA'd into LDS with
//     `buffer_load_dwordx4 ... lds` (no staging VGPRs); the image is XOR-arranged so every
//     B-operand ds_read_b64 is bank-conflict free;
//   * input path (XMODE):
//       X_DIRECT  each lane loads its 16 patch pixels straight from HBM/L2 (prefetched one
//                 chunk ahead). Simple, any shape, but 4x overlapping patches make the
//                 texture-address path the bottleneck (TA busy ~60%, PMC);
//       X_UNPOOL  the same, rebuilding the full-resolution dgrad input from the pooled
//                 gradient + argmax bytes (a 4x4 patch spans 3x3 pooled cells);
//       X_STAGED  the block's input REGION (its 64 tiles' union, halos shared) is DMA'd once
//                 per chunk into a double-buffered, source-swizzled LDS image, and lanes read
//                 their patches with conflict-free ds_read_b64: ~3x fewer bytes through the
//                 TA and 1/5 of the load instructions;
//       X_STAGED_UNPOOL  the same for the dgrad of a pooled layer: the POOLED gradient region
//                 (16-B DMA) and its argmax bytes (4-B DMA) are staged, and each lane rebuilds
//                 its full-resolution 4x4 patch from the 3x3 pooled cells it spans;
//   * the epilogue applies Y = A^T m A in registers. A 2x2 Winograd output tile IS a 2x2
//     max-pool window, so pooling is 3 max ops on values the lane already holds; BN affine,
//     ReLU, Taylor partials and the masked gradient are fused exactly as in conv_mfma.hip.
#include "tp_common.h"
#include "tp_launchers.h"

#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

namespace tp {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two fp32 -> two bf16 (round to nearest even, v_cvt_pk_bf16_f32) in one dword, .x in the low half
__device__ __forceinline__ unsigned bf16x2_of(const f32x2 v) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ f32x2 buf_load_f32x2(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2f32");
__device__ unsigned short buf_load_u16(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.i16");

enum WEpi : int { W_FWD = 0, W_FWD_POOL = 1, W_BWD = 2, W_PARTIAL = 3 };

// X_SPAN: X_STAGED for any W/2 (ResNet's 56/28/14): the block's 64 consecutive tiles span a few
// tile rows of up to MAX_SEG images; each image segment's input rows (halos included) are
// stacked in the staged LDS image, so every shape gets the halo-sharing LDS input path.
enum XMode : int { X_DIRECT = 0, X_UNPOOL = 1, X_STAGED = 2, X_STAGED_UNPOOL = 3, X_SPAN = 4 };
constexpr int MAX_SEG = 4;

constexpr int W_TK = 32;             // output channels per block
constexpr int W_CH = 8;              // input channels per chunk
constexpr int W_UIMG = 4096;         // floats of one U image (16 xi x 8 c x 32 k)
constexpr int W_XS = 6144;           // floats of one staged input image (24 KiB)

struct WinoArgs {
  const float* x;           // NHWC (B,H,W,C), or pooled grad (B,H/2,W/2,C) for X_UNPOOL
  const uint8_t* x_argmax;  // X_UNPOOL: argmax bytes of the pooled grad
  const float* u;           // U images [C/8][K/32][4096]
  int B, H, W, C, K;
  int P;                    // output tiles = B*(H/2)*(W/2)
  int c_per_split;
  long long x_elems;
  const float* scale;
  const float* shift;
  int relu;
  float* out;
  uint8_t* out_argmax;
  const float* act;
  float* taylor;
  int pooled_m;             // W_PARTIAL: write the slab in pooled M order (b, th, tw, q)
  // X_STAGED region geometry: a block's 64 tiles = n_img images x R tile rows each
  int n_img, R, RW, IP;     // RW: row pitch (pixels), IP: image pitch (pixels); X_SPAN uses RW only
  int rounds;               // 256-slot DMA rounds per staged image
  // X_STAGED_UNPOOL: pooled region pitches; argmax image rounds and its byte offset
  int arounds, aoff;
  int tay_slots;            // W_BWD: partial slots R of the (R, B, K) taylor slab
  FastDiv fd_timg, fd_w2, fd_ip, fd_rw;  // T_img = (H/2)(W/2), W/2, IP, RW
  float* apoz;              // W_FWD: [B][K] counts of positive outputs (exact integers), nullable
  int dbg;                  // experiment switches (TP_WINO_DBG): 1 no epilogue, 2 no restaging, 4 no transform
  int tay_mode;             // W_BWD partials: 0 Taylor -(g*a), 1 Sensitivity |g|, 2 |g| where a > 0
};

// Phase-attribution switches for profiling experiments only: they skip barriers / stores and
// give wrong results, so they exist only in a -DTP_WINO_DEBUG build (compiled out otherwise).
#ifdef TP_WINO_DEBUG
#define WDBG(p, bit) ((p).dbg & (bit))
#else
#define WDBG(p, bit) (0)
#endif

__device__ __forceinline__ int xcd_remap_w(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = bid % 8, idx = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// staged-image slot swizzle (an involution; keeps 4-slot groups): linear slot L = 2*pixel + half
__host__ __device__ __forceinline__ int xswz(int L) { return L ^ ((L >> 4) & 3); }

// V = B^T d B on two channels at once, B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]
__device__ __forceinline__ void input_transform2(const f32x2 d[16], f32x2 v[16]) {
  f32x2 t[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t[0 * 4 + j] = d[0 * 4 + j] - d[2 * 4 + j];
    t[1 * 4 + j] = d[1 * 4 + j] + d[2 * 4 + j];
    t[2 * 4 + j] = d[2 * 4 + j] - d[1 * 4 + j];
    t[3 * 4 + j] = d[1 * 4 + j] - d[3 * 4 + j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i * 4 + 0] = t[i * 4 + 0] - t[i * 4 + 2];
    v[i * 4 + 1] = t[i * 4 + 1] + t[i * 4 + 2];
    v[i * 4 + 2] = t[i * 4 + 2] - t[i * 4 + 1];
    v[i * 4 + 3] = t[i * 4 + 1] - t[i * 4 + 3];
  }
}

// Y = A^T m A, A^T = [[1,1,1,0],[0,1,-1,-1]]  ->  y[a*2+b]
__device__ __forceinline__ void output_transform(const float m[16], float y[4]) {
  float t[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t[0 * 4 + j] = m[0 * 4 + j] + m[1 * 4 + j] + m[2 * 4 + j];
    t[1 * 4 + j] = m[1 * 4 + j] - m[2 * 4 + j] - m[3 * 4 + j];
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    y[a * 2 + 0] = t[a * 4 + 0] + t[a * 4 + 1] + t[a * 4 + 2];
    y[a * 2 + 1] = t[a * 4 + 1] - t[a * 4 + 2] - t[a * 4 + 3];
  }
}

// output_transform on two accumulator rows at once (v_pk_add_f32): rows r, r+1 of an f32x4
// accumulator are an aligned register pair; same operations and order as output_transform
__device__ __forceinline__ void output_transform2(const f32x2 m[16], f32x2 y[4]) {
  f32x2 t[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t[0 * 4 + j] = m[0 * 4 + j] + m[1 * 4 + j] + m[2 * 4 + j];
    t[1 * 4 + j] = m[1 * 4 + j] - m[2 * 4 + j] - m[3 * 4 + j];
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    y[a * 2 + 0] = t[a * 4 + 0] + t[a * 4 + 1] + t[a * 4 + 2];
    y[a * 2 + 1] = t[a * 4 + 1] - t[a * 4 + 2] - t[a * 4 + 3];
  }
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// one 16-B-per-lane LDS-DMA: lane l's 16 bytes land at lds_base + 16*l
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, float* lds_base, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)lds_base, 16, voff, soff, 0, 0);
}

// ---- epilogue: output tiles pw0 + 4g + r, channels k0 + j + 16n ------------------------
// Taylor partials (W_BWD) without atomics: the block reduces its (tile, channel) partials in a
// fixed order and writes each image's block sum into slot (block index within the image) of
// the (R, B, K) taylor slab — a single-writer +=; score_fold sums the R slots in slot order.
// The result is bit-reproducible run to run (no float atomics on the engine's Taylor path).
__host__ __device__ inline int wino_taylor_slots(int H, int W) {
  const int T_img = ((H + 1) / 2) * ((W + 1) / 2);  // odd sizes: the last tile row / column is partial
  if (T_img <= 0) return 1;
  if (T_img % 64 == 0) return T_img / 64;
  if (64 % T_img == 0) return 1;
  return (T_img + 63) / 64 + 1;
}

// LDS slot of pixel q of block-local tile t in the transpose buffer (rotated by t>>2 so the
// phase-1 writes of lanes g and g+1, whose tiles differ by 4, land on different banks)
__device__ __forceinline__ int ybuf_row(int t, int q) { return t * 4 + ((q + (t >> 2)) & 3); }
__device__ __forceinline__ int pbuf_row(int t) { return t ^ ((t >> 2) & 1); }

// Epilogue in two phases so that every global access is a full 128-B line:
//   1. each lane applies Y = A^T m A to its (tile, channel) accumulators and parks the 2x2
//      outputs (or the pooled value + argmax) in LDS (yb0: channels k0..k0+15, yb1: +16..31);
//   2. threads own (pixel, 4-channel) items: act loads, out / pooled / argmax / slab stores
//      are float4 (uint32 for argmax) and 8 consecutive lanes cover a pixel's 32 channels.
// yb0, yb1: 4096 floats each, free for reuse (the main loop ended with a barrier);
// al0, al1 (W_BWD, staged kernels): the act tile prefetched into LDS, else nullptr.
template <int EPI>
__device__ __forceinline__ void wino_epilogue(const WinoArgs& p, f32x4 (&acc)[16][2], int pw0, int k0, int g, int j,
                                              int blk_p, float* yb0, float* yb1, const float* al0, const float* al1) {
  const int H2 = (p.H + 1) >> 1, W2 = (p.W + 1) >> 1, T_img = H2 * W2;
  const int t0 = blk_p * 64;
  const int tid = threadIdx.x;
  const int tl_base = (pw0 - t0) + 4 * g;  // block-local index of this lane's first output tile
  unsigned char* ab = reinterpret_cast<unsigned char*>(yb0 + 2048);  // FWD_POOL argmax bytes [64][32]

  // ---- phase 1: transform, park in LDS --------------------------------------------------
  if WDBG(p, 16) goto phase2;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    float* yb = n == 0 ? yb0 : yb1;
    const int k = k0 + j + 16 * n;
    float sc = 1.f, sh = 0.f;
    if constexpr (EPI == W_FWD_POOL) {
      if (k < p.K) {
        sc = p.scale ? p.scale[k] : 1.f;
        sh = p.shift ? p.shift[k] : 0.f;
      }
    }
#pragma unroll
    for (int r2 = 0; r2 < 4; r2 += 2) {  // tiles r2, r2 + 1: one packed output transform
      f32x2 m2[16], y2[4];
#pragma unroll
      for (int x = 0; x < 16; ++x) m2[x] = f32x2{acc[x][n][r2], acc[x][n][r2 + 1]};
      output_transform2(m2, y2);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
      const int tl = tl_base + r2 + h;
      float y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = h ? y2[q].y : y2[q].x;
      if constexpr (EPI == W_FWD_POOL) {
        float best = 0.f;
        int arg = 0, cnt = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = y[q] * sc + sh;
          if (p.relu) v = nan_relu(v);
          cnt += v > 0.f ? 1 : 0;
          if (q == 0 || v > best || (v != v && best == best)) {
            best = v;
            arg = q;
          }
        }
        yb[pbuf_row(tl) * 16 + j] = best;
        // argmax in bits 0-1; the window's count of positive pre-pool outputs (APoZ) in bits 2-4
        ab[pbuf_row(tl) * 32 + j + 16 * n] = (unsigned char)(arg | (cnt << 2));
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) yb[ybuf_row(tl, q) * 16 + j] = y[q];
      }
      }
    }
  }
  __syncthreads();
phase2:
  // ---- phase 2: coalesced global traffic ------------------------------------------------
  if WDBG(p, 8) return;
  const int c4 = tid & 7;  // 4-channel group: channels k0 + 4*c4 .. +3
  const int k = k0 + 4 * c4;
  const float* ybr = (c4 < 4 ? yb0 : yb1) + (c4 & 3) * 4;
  if constexpr (EPI == W_FWD_POOL) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int tl = (tid >> 3) + 32 * i;
      const int pt = t0 + tl;
      if (pt >= p.P || k >= p.K) continue;
      const float4 v = *reinterpret_cast<const float4*>(ybr + pbuf_row(tl) * 16);
      const unsigned a4 = *reinterpret_cast<const unsigned*>(ab + pbuf_row(tl) * 32 + 4 * c4);
      const long long o = (long long)pt * p.K + k;
      *reinterpret_cast<float4*>(p.out + o) = v;
      *reinterpret_cast<unsigned*>(p.out_argmax + o) = a4 & 0x03030303u;
    }
    if (p.apoz) {  // per-(image, channel) counts of positive pre-pool outputs (exact integers)
      const int b_first = p.fd_timg.div(t0);
      const int t_last = min(t0 + 64, p.P) - 1;
      const int n_img = p.fd_timg.div(t_last) - b_first + 1;
      for (int t = tid; t < n_img * W_TK; t += blockDim.x) {
        const int bb = b_first + t / W_TK, kk = t % W_TK, kc = k0 + kk;
        if (bb >= p.B || kc >= p.K) continue;
        const int lo = max(bb * T_img, t0) - t0, hi = min((bb + 1) * T_img - 1, t_last) - t0;
        int sum = 0;
        for (int tl = lo; tl <= hi; ++tl) sum += ab[pbuf_row(tl) * 32 + kk] >> 2;
        if (sum > 0) atomicAdd(p.apoz + (long long)bb * p.K + kc, (float)sum);
      }
    }
    return;
  } else {
    const int q = (tid >> 3) & 3;
    float4 sc4 = make_float4(1.f, 1.f, 1.f, 1.f), sh4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EPI != W_PARTIAL) {
      if (k < p.K) {
        if (p.scale) sc4 = *reinterpret_cast<const float4*>(p.scale + k);
        if (EPI == W_FWD && p.shift) sh4 = *reinterpret_cast<const float4*>(p.shift + k);
      }
    }
    float4 tq[8];  // W_BWD: per-tile Taylor partial of this (q, 4 channels)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int tl = (tid >> 5) + 8 * i;
      const int pt = t0 + tl;
      tq[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pt >= p.P || k >= p.K) continue;
      const float4 y = *reinterpret_cast<const float4*>(ybr + ybuf_row(tl, q) * 16);
      const int bb = p.fd_timg.div(pt), rr = pt - bb * T_img;
      const int oh2 = p.fd_w2.div(rr), ow2 = rr - oh2 * W2;
      const int oh = 2 * oh2 + (q >> 1), ow = 2 * ow2 + (q & 1);
      if (oh >= p.H || ow >= p.W) continue;  // outside an odd-sized image: nothing to store or sum
      const long long pix = ((long long)bb * p.H + oh) * p.W + ow;
      if constexpr (EPI == W_FWD) {
        float4 v;
        v.x = y.x * sc4.x + sh4.x;
        v.y = y.y * sc4.y + sh4.y;
        v.z = y.z * sc4.z + sh4.z;
        v.w = y.w * sc4.w + sh4.w;
        if (p.relu) {
          v.x = nan_relu(v.x);
          v.y = nan_relu(v.y);
          v.z = nan_relu(v.z);
          v.w = nan_relu(v.w);
        }
        *reinterpret_cast<float4*>(p.out + pix * p.K + k) = v;
        if (p.apoz)
          tq[i] = make_float4(v.x > 0.f ? 1.f : 0.f, v.y > 0.f ? 1.f : 0.f, v.z > 0.f ? 1.f : 0.f,
                              v.w > 0.f ? 1.f : 0.f);
      } else if constexpr (EPI == W_PARTIAL) {
        const long long mrow = p.pooled_m ? (long long)pt * 4 + q : pix;
        *reinterpret_cast<float4*>(p.out + ((long long)blockIdx.y * p.B * p.H * p.W + mrow) * p.K + k) = y;
      } else {  // W_BWD
        // act: prefetched into LDS by the last chunk's DMA (slot tid + 256 i), else global
        const float4 a = al0 ? *reinterpret_cast<const float4*>((i < 4 ? al0 : al1) + ((i & 3) * 256 + tid) * 4)
                             : *reinterpret_cast<const float4*>(p.act + pix * p.K + k);
        tq[i] = make_float4(tay_term(p.tay_mode, y.x, a.x), tay_term(p.tay_mode, y.y, a.y),
                            tay_term(p.tay_mode, y.z, a.z), tay_term(p.tay_mode, y.w, a.w));
        if (p.out) {
          float4 v;
          v.x = a.x > 0.f ? y.x * sc4.x : 0.f;
          v.y = a.y > 0.f ? y.y * sc4.y : 0.f;
          v.z = a.z > 0.f ? y.z * sc4.z : 0.f;
          v.w = a.w > 0.f ? y.w * sc4.w : 0.f;
          *reinterpret_cast<float4*>(p.out + pix * p.K + k) = v;
        }
      }
    }
    if constexpr (EPI == W_BWD || EPI == W_FWD) {
      // per-(image, channel) sums of the per-item partials: W_BWD Taylor (fixed order, slot
      // write), W_FWD APoZ counts (exact integers: atomics are order-free)
      if (EPI == W_BWD ? !p.taylor : !p.apoz) return;
      // sum the 4 pixels of each tile: lanes tid ^ 8, ^ 16 hold q ^ 1, q ^ 2 (fixed order)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float4 t = tq[i];
        t.x = xsum16(xsum8(t.x));
        t.y = xsum16(xsum8(t.y));
        t.z = xsum16(xsum8(t.z));
        t.w = xsum16(xsum8(t.w));
        tq[i] = t;
      }
      __syncthreads();  // everyone is done reading yb0/yb1
      if (q == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int tl = (tid >> 5) + 8 * i;
          *reinterpret_cast<float4*>(yb0 + tl * W_TK + 4 * c4) = tq[i];
        }
      }
      __syncthreads();
      const int b_first = p.fd_timg.div(t0);
      const int t_last = min(t0 + 64, p.P) - 1;
      const int n_img = p.fd_timg.div(t_last) - b_first + 1;
      for (int t = tid; t < n_img * W_TK; t += blockDim.x) {
        const int bb = b_first + t / W_TK, kk = t % W_TK, kc = k0 + kk;
        if (bb >= p.B || kc >= p.K) continue;
        const int lo = max(bb * T_img, t0) - t0, hi = min((bb + 1) * T_img - 1, t_last) - t0;
        float sum = 0.f;
        for (int tl = lo; tl <= hi; ++tl) sum += yb0[tl * W_TK + kk];
        if constexpr (EPI == W_FWD) {
          if (sum > 0.f) atomicAdd(p.apoz + (long long)bb * p.K + kc, sum);
        } else {
          const int slot = blk_p - (bb * T_img) / 64;
          if (slot < p.tay_slots) p.taylor[((long long)slot * p.B + bb) * p.K + kc] += sum;
        }
      }
    }
  }
}

// BF (opt-in, compute_dtype=bfloat16; staged input modes): U images in bf16 (half the bytes of
// DMA) and the products on v_mfma_f32_16x16x16_bf16 with fp32 accumulation. A lane's V pair
// (channels 2g, 2g+1, transformed in fp32) is rounded to bf16 and zero-padded to the MFMA's 4
// k-values, so one bf16 MFMA replaces the two fp32 MFMAs of (e = 0, 1) per output half;
// staging, transforms and epilogues are the fp32 kernel's. BF = 2 (TP_WINO_BF_SPLIT=1, measured
// option): V carried as a bf16 hi + lo pair in the padding k-slots (~16 mantissa bits of V, only
// U rounded); 18% slower, and on the trained headline teacher the scores rank the same.
// BF = 3 (measured option TP_WINO_BF_K16=1; X_STAGED regions of <= 3 DMA rounds, C % 16 == 0):
// 16-channel chunks — two 8-channel X images and two U images per stage — so a lane's MFMA
// operand holds its two channel pairs (k = image 0 pair, image 1 pair) and every k-slot is used:
// half the bf16 MFMAs (v_mfma_f32_16x16x16_bf16 costs as much as 16x16x32, ~16 cycles) and half
// the barriers. Measured on the VGG16 layers: forward 0.5-19% faster on the 32/16-pixel maps,
// the 32-pixel data gradient 28% slower, the engine unchanged (profiles/bf16/).
// Measured and dropped: a 3-deep LDS-DMA ring for these kernels (DMA latency is not what bounds
// them: fwd 1.0x, dgrad 0.94x without the act prefetch it displaced).
template <int EPI, int XMODE, int BF = 0>
__global__ __launch_bounds__(256, 2) void wino_f2x3(WinoArgs p) {
  constexpr bool STAGED = XMODE == X_STAGED || XMODE == X_STAGED_UNPOOL || XMODE == X_SPAN;
  constexpr bool UNPOOL = XMODE == X_UNPOOL;
  static_assert(BF != 3 || XMODE == X_STAGED, "16-channel bf16 chunks: staged regions only");
  constexpr int CHK = BF == 3 ? 2 * W_CH : W_CH;  // input channels per stage
  // separate objects per buffer so the compiler's LDS-DMA alias tracking can tell them apart.
  // The staged modes use exactly 80 KB: two blocks per CU (160 KB). ANY extra __shared__ byte
  // halves the occupancy (tests/test_conv_gpu.py::test_wino_lds_budget guards this).
  __shared__ __attribute__((aligned(16))) float us0[W_UIMG];
  __shared__ __attribute__((aligned(16))) float us1[W_UIMG];
  __shared__ __attribute__((aligned(16))) float xs0[STAGED ? W_XS : 4];
  __shared__ __attribute__((aligned(16))) float xs1[STAGED ? W_XS : 4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int n_k = p.K / W_TK;
  const int tile = xcd_remap_w(blockIdx.x, gridDim.x);
  const int kb = tile % n_k, k0 = kb * W_TK;
  const int blk_p = tile / n_k;
  const int pw0 = blk_p * 64 + wave * 16;  // first tile of this wave
  // tile grid: odd H / W (X_DIRECT only) get a partial last tile row / column
  const int H2 = (p.H + 1) >> 1, W2 = (p.W + 1) >> 1, T_img = H2 * W2;
  const int c_begin = blockIdx.y * p.c_per_split;
  const int c_end = min(p.C, c_begin + p.c_per_split);
  constexpr unsigned OOB = 0x80000000u;

  const __amdgpu_buffer_rsrc_t urs =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.u, (short)0, (int)(16u * p.C * p.K * (BF ? 2u : 4u)), 0x00020000);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, (short)0,
                                                                        (int)(p.x_elems * 4), 0x00020000);
  const i32x4 xr = make_rsrc(p.x, (unsigned)(p.x_elems * 4));
  const i32x4 ar = make_rsrc(p.x_argmax, UNPOOL ? (unsigned)p.x_elems : 0u);
  const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x_argmax, (short)0, XMODE == X_STAGED_UNPOOL ? (int)p.x_elems : 0, 0x00020000);

  // ---- this lane's input tile (A row j) ------------------------------------------------
  const int pin = pw0 + j;
  int b = 0, th = 0, tw = 0;
  const bool tok = pin < p.P;
  if (tok) {
    b = p.fd_timg.div(pin);
    const int r = pin - b * T_img;
    th = p.fd_w2.div(r);
    tw = r - th * W2;
  }

  // X_DIRECT / X_UNPOOL: per-lane pixel offsets; X_STAGED: per-lane LDS byte offsets
  int poff[16];
  int aoffs[XMODE == X_STAGED_UNPOOL ? 9 : 1];
  unsigned pmask = 0;
  // X_STAGED: this thread's DMA source offsets (bytes, channel 0) for each 256-slot round
  constexpr int MAX_ROUNDS = W_XS * 4 / 16 / 256;  // 6
  unsigned xsrc[STAGED ? MAX_ROUNDS : 1];
  if constexpr (XMODE == X_DIRECT) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ih = 2 * th - 1 + r, iw = 2 * tw - 1 + q;
        const bool ok = tok && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        poff[r * 4 + q] = ((b * p.H + ih) * p.W + iw) * p.C;
        pmask |= (ok ? 1u : 0u) << (r * 4 + q);
      }
  } else if constexpr (XMODE == X_UNPOOL) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int ph = th - 1 + r, pq = tw - 1 + q;
        const bool ok = tok && ph >= 0 && ph < H2 && pq >= 0 && pq < W2;
        poff[r * 3 + q] = ((b * H2 + ph) * W2 + pq) * p.C;
        pmask |= (ok ? 1u : 0u) << (r * 3 + q);
      }
  } else if constexpr (XMODE == X_SPAN) {
    // segments: images b0 .. bL of the block's tiles; segment sg holds input rows
    // 2*th_lo[sg]-1 .. 2*th_hi[sg]+2 of image b0+sg at region rows base[sg] ..
    const int t0 = blk_p * 64, tl = min(t0 + 63, p.P - 1);
    const int b0 = p.fd_timg.div(t0), bL = p.fd_timg.div(tl);
    int th_lo[MAX_SEG], base[MAX_SEG + 1];
    base[0] = 0;
#pragma unroll
    for (int sg = 0; sg < MAX_SEG; ++sg) {
      const int bb = b0 + sg;
      const bool live = bb <= bL;
      const int lo = sg == 0 ? p.fd_w2.div(t0 - b0 * T_img) : 0;
      const int hi = bb == bL ? p.fd_w2.div(tl - bL * T_img) : H2 - 1;
      th_lo[sg] = lo;
      base[sg + 1] = base[sg] + (live ? 2 * (hi - lo + 1) + 2 : 0);
    }
    const int sg_l = tok ? b - b0 : 0;
    int bsel = 0, lsel = 0;
#pragma unroll
    for (int sg = 0; sg < MAX_SEG; ++sg)
      if (sg == sg_l) {
        bsel = base[sg];
        lsel = th_lo[sg];
      }
    const int pix0 = tok ? (bsel + 2 * (th - lsel)) * p.RW + 2 * tw : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int L = 2 * (pix0 + r * p.RW + q) + (g >> 1);
        poff[r * 4 + q] = xswz(L) * 16 + (g & 1) * 8;
      }
#pragma unroll
    for (int i = 0; i < MAX_ROUNDS; ++i) {
      const int s_ = i * 256 + tid;
      const int L = xswz(s_);
      const int pix = L >> 1, h = L & 1;
      const int row = p.fd_rw.div(pix), col = pix - row * p.RW;
      int sg = 0;
#pragma unroll
      for (int k = 1; k < MAX_SEG; ++k) sg += row >= base[k] ? 1 : 0;
      int rb = 0, lo = 0;
#pragma unroll
      for (int k = 0; k < MAX_SEG; ++k)
        if (k == sg) {
          rb = base[k];
          lo = th_lo[k];
        }
      const int bb = b0 + sg, ih = 2 * lo - 1 + (row - rb), iw = col - 1;
      const bool ok = i < p.rounds && row < base[MAX_SEG] && col < p.W + 2 && bb <= bL && bb < p.B && ih >= 0 &&
                      ih < p.H && iw >= 0 && iw < p.W;
      xsrc[i] = ok ? (unsigned)((((bb * p.H + ih) * p.W + iw) * p.C) * 4 + h * 16) : OOB;
    }
  } else if constexpr (XMODE == X_STAGED) {
    // block region: images b0 .. b0+n_img-1, input rows 2*th0-1 .. 2*th0+2R, cols -1 .. W
    const int t0 = blk_p * 64;
    const int b0 = p.fd_timg.div(t0);
    const int th0 = p.fd_w2.div(t0 - b0 * T_img);
    const int RH = 2 * p.R + 2, RWc = p.W + 2;
    // lane's patch in region coordinates (clamped for tail lanes: results are discarded)
    const int im = tok ? b - b0 : 0, rr0 = tok ? 2 * (th - th0) : 0, cc0 = tok ? 2 * tw : 0;
    const int pix0 = im * p.IP + rr0 * p.RW + cc0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int L = 2 * (pix0 + r * p.RW + q) + (g >> 1);
        poff[r * 4 + q] = xswz(L) * 16 + (g & 1) * 8;
      }
#pragma unroll
    for (int i = 0; i < MAX_ROUNDS; ++i) {
      const int s = i * 256 + tid;
      const int L = xswz(s);
      const int pix = L >> 1, h = L & 1;
      const int imr = p.fd_ip.div(pix), rem = pix - imr * p.IP;
      const int rr = p.fd_rw.div(rem), cc = rem - rr * p.RW;
      const int bb = b0 + imr, ih = 2 * th0 - 1 + rr, iw = cc - 1;
      const bool ok = i < p.rounds && imr < p.n_img && rr < RH && cc < RWc && bb < p.B && ih >= 0 &&
                      ih < p.H && iw >= 0 && iw < p.W;
      xsrc[i] = ok ? (unsigned)((((bb * p.H + ih) * p.W + iw) * p.C) * 4 + h * 16) : OOB;
    }
  } else {  // X_STAGED_UNPOOL: pooled rows th0-1 .. th0+R, pooled cols -1 .. W2
    const int t0 = blk_p * 64;
    const int b0 = p.fd_timg.div(t0);
    const int th0 = p.fd_w2.div(t0 - b0 * T_img);
    const int PRH = p.R + 2, PRWc = W2 + 2;
    const int im = tok ? b - b0 : 0, pr0 = tok ? th - th0 : 0, pc0 = tok ? tw : 0;
    const int cell0 = im * p.IP + pr0 * p.RW + pc0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int cell = cell0 + r * p.RW + q;
        poff[r * 3 + q] = xswz(2 * cell + (g >> 1)) * 16 + (g & 1) * 8;  // value (2 floats)
        aoffs[r * 3 + q] = p.aoff + cell * 8 + 2 * g;                   // argmax (2 bytes)
      }
#pragma unroll
    for (int i = 0; i < MAX_ROUNDS; ++i) {
      // rounds [0, rounds): value slots (16 B), [rounds, rounds + arounds): argmax units (4 B)
      const bool val = i < p.rounds;
      const int s = val ? i * 256 + tid : (i - p.rounds) * 256 + tid;
      const int L = val ? xswz(s) : s;
      const int cell = L >> 1, h = L & 1;
      const int imr = p.fd_ip.div(cell), rem = cell - imr * p.IP;
      const int pr = p.fd_rw.div(rem), pc = rem - pr * p.RW;
      const int bb = b0 + imr, ph = th0 - 1 + pr, pw = pc - 1;
      const bool ok = i < p.rounds + p.arounds && imr < p.n_img && pr < PRH && pc < PRWc && bb < p.B &&
                      ph >= 0 && ph < H2 && pw >= 0 && pw < W2;
      const unsigned e0 = (unsigned)(((bb * H2 + ph) * W2 + pw) * p.C);
      xsrc[i] = ok ? (val ? e0 * 4 + h * 16 : e0 + h * 4) : OOB;
    }
  }

  // ---- staging (LDS-DMA): U image of chunk c0 (+ the input region when STAGED) ---------
  auto stage = [&](int c0, float* ud, float* xd) {
    const unsigned ubase = (unsigned)(((c0 / W_CH) * n_k + kb) * W_UIMG) * (BF ? 2u : 4u);
#pragma unroll
    for (int i = 0; i < (BF ? 2 : 4); ++i)
      dma16(urs, ud + (i * 256 + wave * 64) * 4, (unsigned)(i * 256 + tid) * 16u, ubase);
    if constexpr (BF == 3) {  // second 8-channel half: U image of chunk c0/8 + 1, X image at + rounds
      const unsigned ubase1 = (unsigned)((((c0 / W_CH) + 1) * n_k + kb) * W_UIMG) * 2u;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        dma16(urs, ud + W_UIMG / 2 + (i * 256 + wave * 64) * 4, (unsigned)(i * 256 + tid) * 16u, ubase1);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < p.rounds) dma16(xrs, xd + (i * 256 + wave * 64) * 4, xsrc[i], (unsigned)c0 * 4u);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < p.rounds)
          dma16(xrs, xd + p.rounds * 1024 + (i * 256 + wave * 64) * 4, xsrc[i], (unsigned)(c0 + W_CH) * 4u);
    } else if constexpr (XMODE == X_STAGED || XMODE == X_SPAN) {
#pragma unroll
      for (int i = 0; i < MAX_ROUNDS; ++i)
        if (i < p.rounds) dma16(xrs, xd + (i * 256 + wave * 64) * 4, xsrc[i], (unsigned)c0 * 4u);
    } else if constexpr (XMODE == X_STAGED_UNPOOL) {
#pragma unroll
      for (int i = 0; i < MAX_ROUNDS; ++i) {
        if (i < p.rounds) {
          dma16(xrs, xd + (i * 256 + wave * 64) * 4, xsrc[i], (unsigned)c0 * 4u);
        } else if (i < p.rounds + p.arounds) {
          float* ab = reinterpret_cast<float*>(reinterpret_cast<char*>(xd) + p.aoff) + (i - p.rounds) * 256 +
                      wave * 64;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(ars, (lds_ptr_t)ab, 4, xsrc[i], (unsigned)c0, 0, 0);
        }
      }
    }
  };

  // X_DIRECT/X_UNPOOL raw operands, prefetched one chunk ahead
  f32x2 xin[STAGED ? 1 : (UNPOOL ? 9 : 16)];
  unsigned amr[UNPOOL ? 9 : 1];
  auto issue_x = [&](int c0) {
    const int cc = c0 + 2 * g;
    if constexpr (XMODE == X_DIRECT) {
#pragma unroll
      for (int t = 0; t < 16; ++t)
        xin[t] = buf_load_f32x2(xr, (int)(((pmask >> t) & 1u) ? (unsigned)(poff[t] + cc) * 4u : OOB), 0, 0);
    } else if constexpr (XMODE == X_UNPOOL) {
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const bool ok = (pmask >> t) & 1u;
        xin[t] = buf_load_f32x2(xr, (int)(ok ? (unsigned)(poff[t] + cc) * 4u : OOB), 0, 0);
        amr[t] = buf_load_u16(ar, (int)(ok ? (unsigned)(poff[t] + cc) : OOB), 0, 0);
      }
    }
  };

  f32x4 acc[16][2];
#pragma unroll
  for (int x = 0; x < 16; ++x)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[x][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // B-operand read offset of this lane inside a U image: k = j + 16n at 2 adjacent floats,
  // channel c = 2g + e; the g-slot is XORed with j>>3 so lanes j and j+8 use other banks
  const int uoff = j * 8 + 2 * (g ^ ((j >> 3) << 1));

  // W_BWD + STAGED: epilogue act tile prefetch (DMA source offset of this thread per round)
  float* epi_y0 = us0;
  float* epi_y1 = us1;
  float* epi_a0 = nullptr;
  float* epi_a1 = nullptr;
  const __amdgpu_buffer_rsrc_t acts = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.act, (short)0, (STAGED && EPI == W_BWD) ? (int)((long long)p.B * p.H * p.W * p.K * 4) : 0, 0x00020000);
  // DMA source offset of this thread's act slot in round i (slot = 8*pixel + c4: phase 2's order)
  auto act_off = [&](int i) -> unsigned {
    const int slot = i * 256 + tid;
    const int pl = slot >> 3, c4 = slot & 7;
    const int tl = pl >> 2, q = pl & 3;
    const int pt = blk_p * 64 + tl;
    unsigned off = 0x80000000u;
    if (pt < p.P && k0 + 4 * c4 < p.K) {
      const int bb = p.fd_timg.div(pt), rr = pt - bb * T_img;
      const int r2 = p.fd_w2.div(rr);
      const int oh = 2 * r2 + (q >> 1), ow = 2 * (rr - r2 * W2) + (q & 1);
      off = (unsigned)(((((long long)bb * p.H + oh) * p.W + ow) * p.K + k0 + 4 * c4) * 4);
    }
    return off;
  };
  unsigned act_src[STAGED && EPI == W_BWD && BF != 3 ? 8 : 1];
  if constexpr (STAGED && EPI == W_BWD && BF != 3) {
#pragma unroll
    for (int i = 0; i < 8; ++i) act_src[i] = act_off(i);
  }

  // bf16 products of one chunk: U image ub (bf16), this lane's transformed pair v[16]
  auto mfma_bf = [&](const float* ub, const f32x2 (&v)[16]) {
    // bf16 image: dword (x*16 + j)*8 + 2*(g ^ 2*(j >> 3)) + n = channels (2g, 2g+1) of output j + 16n
    const unsigned* ulb = reinterpret_cast<const unsigned*>(ub) + uoff;
    constexpr int AHEAD = 4;
    u32x2 wq[AHEAD];
#pragma unroll
    for (int s = 0; s < AHEAD; ++s) wq[s] = *reinterpret_cast<const u32x2*>(ulb + s * 128);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int x = 0; x < 16; ++x) {
      const u32x2 w2 = wq[x % AHEAD];
      if (x + AHEAD < 16) wq[x % AHEAD] = *reinterpret_cast<const u32x2*>(ulb + (x + AHEAD) * 128);
      u32x2 av;
      if constexpr (BF == 2) {
        // V = hi + lo: hi = V truncated to bf16 (exact), lo = bf16(V - hi) in the MFMA's padding
        // k-slots against the same U pair: ~16 mantissa bits of V at no extra MFMA
        // (whole-vector bit casts: the per-element form `bit_cast(unsigned, v.x)` / `.y` compiled
        // to perm(x, x) and x's mask for both halves on this toolchain — wrong lo and hi for .y)
        const u32x2 uv = __builtin_bit_cast(u32x2, v[x]);
        const f32x2 hf = __builtin_bit_cast(f32x2, uv & 0xffff0000u);
        av = u32x2{__builtin_amdgcn_perm(uv.y, uv.x, 0x07060302u), bf16x2_of(v[x] - hf)};
      } else {
        av = u32x2{bf16x2_of(v[x]), 0u};
      }
      const s16x4 a = __builtin_bit_cast(s16x4, av);
      acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(s16x4, u32x2{w2.x, w2.x}),
                                                           acc[x][0], 0, 0, 0);
      acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(s16x4, u32x2{w2.y, w2.y}),
                                                           acc[x][1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // BF == 3: one 16-channel stage. Each half's patch is read and transformed in turn and rounded
  // to bf16 right away (16 dwords per half), then every point's two halves feed one MFMA per
  // output half against U images 0 / 1
  auto compute16 = [&](int c0, const float* ub, const float* xb, float* ud_next, float* xd_next, bool more) {
    unsigned ah[2][16];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x2 d[16], v[16];
      const char* xh = reinterpret_cast<const char*>(xb) + h * p.rounds * 4096;
#pragma unroll
      for (int t = 0; t < 16; ++t) d[t] = *reinterpret_cast<const f32x2*>(xh + poff[t]);
      input_transform2(d, v);
#pragma unroll
      for (int x = 0; x < 16; ++x) ah[h][x] = bf16x2_of(v[x]);
      __builtin_amdgcn_sched_barrier(0);  // half 1's patch loads after half 0 is packed: 32 fewer live VGPRs
    }
    if (more) stage(c0 + CHK, ud_next, xd_next);
    if constexpr (EPI == W_BWD) {
      if (!more) {  // as compute(): the act tile lands under the last stage's MFMAs
        epi_y0 = const_cast<float*>(ub);
        epi_y1 = const_cast<float*>(xb);
        epi_a0 = ud_next;
        epi_a1 = xd_next;
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // offsets computed here, once: no registers held over the loop
          float* dst = (i < 4 ? ud_next : xd_next) + ((i & 3) * 256 + wave * 64) * 4;
          dma16(acts, dst, act_off(i), 0u);
        }
      }
    }
    const unsigned* ul0 = reinterpret_cast<const unsigned*>(ub) + uoff;
    const unsigned* ul1 = ul0 + W_UIMG / 2;
    constexpr int AHEAD = 2;
    u32x2 w0[AHEAD], w1[AHEAD];
#pragma unroll
    for (int s_ = 0; s_ < AHEAD; ++s_) {
      w0[s_] = *reinterpret_cast<const u32x2*>(ul0 + s_ * 128);
      w1[s_] = *reinterpret_cast<const u32x2*>(ul1 + s_ * 128);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int x = 0; x < 16; ++x) {
      const u32x2 a0 = w0[x % AHEAD], a1 = w1[x % AHEAD];
      if (x + AHEAD < 16) {
        w0[x % AHEAD] = *reinterpret_cast<const u32x2*>(ul0 + (x + AHEAD) * 128);
        w1[x % AHEAD] = *reinterpret_cast<const u32x2*>(ul1 + (x + AHEAD) * 128);
      }
      const s16x4 a = __builtin_bit_cast(s16x4, u32x2{ah[0][x], ah[1][x]});
      acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(s16x4, u32x2{a0.x, a1.x}),
                                                           acc[x][0], 0, 0, 0);
      acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(s16x4, u32x2{a0.y, a1.y}),
                                                           acc[x][1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  };

  auto compute = [&](int c0, const float* ub, const float* xb, float* ud_next, float* xd_next, bool more) {
    f32x2 v[16];
    {
      f32x2 d[16];
      if constexpr (XMODE == X_STAGED || XMODE == X_SPAN) {
#pragma unroll
        for (int t = 0; t < 16; ++t)
          d[t] = WDBG(p, 64) ? f32x2{(float)t, 1.f}
                              : *reinterpret_cast<const f32x2*>(reinterpret_cast<const char*>(xb) + poff[t]);
      } else if constexpr (XMODE == X_STAGED_UNPOOL) {
        f32x2 cv[9];
        unsigned ca[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          cv[t] = *reinterpret_cast<const f32x2*>(reinterpret_cast<const char*>(xb) + poff[t]);
          ca[t] = *reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(xb) + aoffs[t]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int cell = ((r + 1) >> 1) * 3 + ((q + 1) >> 1);
            const unsigned want = (unsigned)((((r + 1) & 1) << 1) | ((q + 1) & 1));
            d[r * 4 + q][0] = (ca[cell] & 0xffu) == want ? cv[cell][0] : 0.f;
            d[r * 4 + q][1] = ((ca[cell] >> 8) & 0xffu) == want ? cv[cell][1] : 0.f;
          }
      } else if constexpr (XMODE == X_DIRECT) {
#pragma unroll
        for (int t = 0; t < 16; ++t) d[t] = xin[t];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int cell = ((r + 1) >> 1) * 3 + ((q + 1) >> 1);
            const unsigned want = (unsigned)((((r + 1) & 1) << 1) | ((q + 1) & 1));
            d[r * 4 + q][0] = (amr[cell] & 0xffu) == want ? xin[cell][0] : 0.f;
            d[r * 4 + q][1] = ((amr[cell] >> 8) & 0xffu) == want ? xin[cell][1] : 0.f;
          }
      }
      if WDBG(p, 4) {
#pragma unroll
        for (int t = 0; t < 16; ++t) v[t] = d[t];
      } else {
        input_transform2(d, v);
      }
    }
    if (more && !WDBG(p, 2)) {
      stage(c0 + W_CH, ud_next, xd_next);
      if constexpr (!STAGED) issue_x(c0 + W_CH);
    }
    if constexpr (STAGED && EPI == W_BWD) {
      if (!more) {
        // last chunk: the next-stage buffers are free -> DMA the epilogue's act tile (256 pixels
        // x 32 channels, slot = 8*pixel + c4, i.e. exactly phase 2's thread order) so it lands
        // under this chunk's MFMAs; the current buffers become the phase-1 transpose space
        epi_y0 = const_cast<float*>(ub);
        epi_y1 = const_cast<float*>(xb);
        epi_a0 = ud_next;
        epi_a1 = xd_next;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float* dst = (i < 4 ? ud_next : xd_next) + ((i & 3) * 256 + wave * 64) * 4;
          dma16(acts, dst, act_src[i], 0u);
        }
      }
    }
    if constexpr (BF) {
      mfma_bf(ub, v);
      __syncthreads();
      return;
    }
    const float* ul = ub + uoff;
    constexpr int AHEAD = 4;
    float2 wq[AHEAD];
#pragma unroll
    for (int s = 0; s < AHEAD; ++s)
      wq[s] = *reinterpret_cast<const float2*>(ul + ((s & 15) * 2 + (s >> 4)) * 128);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      const int x = s & 15, e = s >> 4;
      const float2 w2 = wq[s % AHEAD];
      if (s + AHEAD < 32) {
        const int s2 = s + AHEAD;
        wq[s % AHEAD] = *reinterpret_cast<const float2*>(ul + ((s2 & 15) * 2 + (s2 >> 4)) * 128);
      }
      acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[x][e], w2.x, acc[x][0], 0, 0, 0);
      acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[x][e], w2.y, acc[x][1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);
    if WDBG(p, 32) __builtin_amdgcn_s_waitcnt(0);
    else __syncthreads();  // drains this chunk's DMA for the next one and orders buffer reuse
  };

  if (c_begin < c_end) {
    if constexpr (!STAGED) issue_x(c_begin);
    stage(c_begin, us0, xs0);
    __syncthreads();
    if constexpr (BF == 3) {
      for (int c0 = c_begin; c0 < c_end; c0 += 2 * CHK) {
        compute16(c0, us0, xs0, us1, xs1, c0 + CHK < c_end);
        if (c0 + CHK < c_end) compute16(c0 + CHK, us1, xs1, us0, xs0, c0 + 2 * CHK < c_end);
      }
    } else {
    for (int c0 = c_begin; c0 < c_end; c0 += 2 * W_CH) {
      compute(c0, us0, xs0, us1, xs1, c0 + W_CH < c_end);
      if (c0 + W_CH < c_end) compute(c0 + W_CH, us1, xs1, us0, xs0, c0 + 2 * W_CH < c_end);
    }
    }
  }
  if WDBG(p, 1) {
    float t = 0.f;
#pragma unroll
    for (int x = 0; x < 16; ++x) t += acc[x][0][0] + acc[x][1][3];
    if (t == 1234.5f) p.out[0] = t;  // keeps the main loop alive
    return;
  }
  wino_epilogue<EPI>(p, acc, pw0, k0, g, j, blk_p, epi_y0, epi_y1, epi_a0, epi_a1);
}

// ---------------------------------------------------------------------------------------
// Weight transform U = G g G^T written straight into the LDS images the kernels DMA (the
// layout of fused_chain.winograd_weights): word ((xi*2 + e)*16 + j)*8 + 2*(g ^ 2*(j >> 3)) + n of
// image (cb, kb) holds U[xi][c = 8cb + 2g + e][k = 32kb + j + 16n]. Computed in fp64, rounded once.
// ``flip_t``: the data-gradient operand — w'[k][c] = w[c][k] with the taps rotated 180 degrees —
// read from the forward weight directly (no flipped / transposed copy).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wino_weight_transform(const float* __restrict__ w, float* __restrict__ u,
                                                             int K, int C, int flip_t, int S0, int S1) {
  const long long total = (long long)(C / 8) * (K / 32) * W_UIMG;
  const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const int word = (int)(t % W_UIMG);
    const long long img = t / W_UIMG;
    const int kb = (int)(img % (K / 32)), cb = (int)(img / (K / 32));
    const int n = word & 1, gs = (word >> 1) & 3, j = (word >> 3) & 15, e = (word >> 7) & 1, xi = word >> 8;
    const int g = gs ^ ((j >> 3) << 1);
    const int c = 8 * cb + 2 * g + e, k = 32 * kb + j + 16 * n;
    const int i = xi >> 2, jj = xi & 3;
    // source (S0, S1, 3, 3), unpadded: forward w[k][c]; flip_t: the forward weight w[c][k] rotated.
    // (k, c) outside the source are the zero padding of the kernels' channel granules.
    const int r0 = flip_t ? c : k, r1 = flip_t ? k : c;
    double acc = 0.0;
    if (r0 < S0 && r1 < S1) {
      const float* src = w + ((long long)r0 * S1 + r1) * 9;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const int tap = flip_t ? (2 - a) * 3 + (2 - b) : a * 3 + b;
          acc += G[i][a] * (double)src[tap] * G[jj][b];
        }
    }
    u[t] = (float)acc;
  }
}

// bf16 U images (the BF kernels): dword (xi*16 + j)*8 + 2*(g ^ 2*(j >> 3)) + n of image (cb, kb)
// holds bf16(U[xi][c][k]) for c = 8cb + 2g (low half) and c + 1 (high half), k = 32kb + j + 16n.
__global__ __launch_bounds__(256) void wino_weight_transform_bf16(const float* __restrict__ w, unsigned* __restrict__ u,
                                                                  int K, int C, int flip_t, int S0, int S1) {
  constexpr int DW = W_UIMG / 2;
  const long long total = (long long)(C / 8) * (K / 32) * DW;
  const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const int word = (int)(t % DW);
    const long long img = t / DW;
    const int kb = (int)(img % (K / 32)), cb = (int)(img / (K / 32));
    const int n = word & 1, gs = (word >> 1) & 3, j = (word >> 3) & 15, xi = word >> 7;
    const int g = gs ^ ((j >> 3) << 1);
    const int k = 32 * kb + j + 16 * n;
    const int i = xi >> 2, jj = xi & 3;
    f32x2 pair;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = 8 * cb + 2 * g + e;
      const int r0 = flip_t ? c : k, r1 = flip_t ? k : c;
      double acc = 0.0;
      if (r0 < S0 && r1 < S1) {
        const float* src = w + ((long long)r0 * S1 + r1) * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) {
            const int tap = flip_t ? (2 - a) * 3 + (2 - b) : a * 3 + b;
            acc += G[i][a] * (double)src[tap] * G[jj][b];
          }
      }
      pair[e] = (float)acc;
    }
    u[t] = bf16x2_of(pair);
  }
}

// ---------------------------------------------------------------------------------------
// host: staged-region geometry (bank-conflict-minimising pitches) per (B, H, W)
// ---------------------------------------------------------------------------------------
struct XGeom {
  bool ok = false;
  int n_img = 0, R = 0, RW = 0, IP = 0, rounds = 0, arounds = 0, aoff = 0;
};

// extra LDS cycles of the patch ds_read_b64s of one block (2 x 32-lane groups, banks mod 64);
// pooled: 3x3 pooled cells per lane (staged unpool) instead of 4x4 pixels
static int staged_conflicts(int W2, int T_img, int RW, int IP, bool pooled) {
  const int span = pooled ? 3 : 4, step = pooled ? 1 : 2;
  int total = 0;
  for (int wave = 0; wave < 4; ++wave)
    for (int r = 0; r < span; ++r)
      for (int q = 0; q < span; ++q)
        for (int half = 0; half < 2; ++half) {
          int words[64];
          int n = 0;
          for (int jj = 0; jj < 16; ++jj)
            for (int gg = 2 * half; gg < 2 * half + 2; ++gg) {
              const int t = wave * 16 + jj;
              const int im = T_img >= 64 ? 0 : t / T_img;
              const int rem = T_img >= 64 ? t : t % T_img;
              const int th = rem / W2, tw = rem % W2;
              const int pix = im * IP + (step * th + r) * RW + step * tw + q;
              const int w0 = xswz(2 * pix + (gg >> 1)) * 4 + (gg & 1) * 2;
              words[n++] = w0;
              words[n++] = w0 + 1;
            }
          for (int bank = 0; bank < 64; ++bank) {
            int distinct[64];
            int nd = 0;
            for (int a = 0; a < n; ++a) {
              if ((words[a] & 63) != bank) continue;
              bool seen = false;
              for (int z = 0; z < nd; ++z) seen |= distinct[z] == words[a];
              if (!seen) distinct[nd++] = words[a];
            }
            if (nd > 1) total += nd - 1;
          }
        }
  return total;
}

static XGeom staged_geometry(int H, int W, bool pooled) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, bool>, XGeom> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({H, W, pooled});
  if (it != cache.end()) return it->second;
  XGeom gm;
  const int H2 = H / 2, W2 = W / 2, T_img = H2 * W2;
  int n_img = 0, R = 0;
  if (T_img >= 64 && T_img % 64 == 0 && 64 % W2 == 0) {
    n_img = 1;
    R = 64 / W2;
  } else if (T_img >= 4 && 64 % T_img == 0) {
    n_img = 64 / T_img;
    R = H2;
  }
  if (n_img) {
    // region rows x cols: full resolution (2R+2) x (W+2); pooled (R+2) x (W/2+2)
    const int RH = pooled ? R + 2 : 2 * R + 2, RWc = pooled ? W2 + 2 : W + 2;
    int best = -1;
    for (int RW = RWc; RW < RWc + 16; ++RW)
      for (int IP = RH * RW; IP < RH * RW + (n_img > 1 ? 32 : 1); ++IP) {
        const int items = 2 * ((n_img - 1) * IP + RH * RW);  // 16-B value slots (= 4-B argmax units)
        const int rounds = (items + 255) / 256;
        const int arounds = pooled ? rounds : 0;
        const int bytes = rounds * 256 * 16 + arounds * 256 * 4;
        if (bytes > W_XS * 4 || rounds + arounds > W_XS * 4 / 16 / 256) continue;
        const int c = staged_conflicts(W2, T_img, RW, IP, pooled);
        const int cost = c * 4 + rounds;  // conflicts first, then DMA volume
        if (best < 0 || cost < best) {
          best = cost;
          gm.ok = true;
          gm.n_img = n_img;
          gm.R = R;
          gm.RW = RW;
          gm.IP = IP;
          gm.rounds = rounds;
          gm.arounds = arounds;
          gm.aoff = rounds * 256 * 16;
        }
      }
  }
  cache[{H, W, pooled}] = gm;
  return gm;
}

// X_SPAN geometry: the worst-case stacked row count over all block start phases, a row pitch
// chosen by the same bank simulation (block starting at tile 0), and the DMA rounds.
struct SpanGeom {
  bool ok = false;
  int RW = 0, rounds = 0, rows = 0;
};

static void span_rows(int t0, int P, int T_img, int W2, int H2, int* base /* MAX_SEG+1 */, int* th_lo) {
  const int tl = std::min(t0 + 63, P - 1);
  const int b0 = t0 / T_img, bL = tl / T_img;
  base[0] = 0;
  for (int sg = 0; sg < MAX_SEG; ++sg) {
    const int bb = b0 + sg;
    const int lo = sg == 0 ? (t0 - b0 * T_img) / W2 : 0;
    const int hi = bb == bL ? (tl - bL * T_img) / W2 : H2 - 1;
    th_lo[sg] = lo;
    base[sg + 1] = base[sg] + (bb <= bL ? 2 * (hi - lo + 1) + 2 : 0);
  }
}

static int span_conflicts(int W2, int H2, int RW) {
  const int T_img = W2 * H2, P = 64 * 4;
  int base[MAX_SEG + 1], th_lo[MAX_SEG];
  span_rows(0, P, T_img, W2, H2, base, th_lo);
  int total = 0;
  for (int wave = 0; wave < 4; ++wave)
    for (int r = 0; r < 4; ++r)
      for (int q = 0; q < 4; ++q)
        for (int half = 0; half < 2; ++half) {
          int words[64];
          int n = 0;
          for (int jj = 0; jj < 16; ++jj)
            for (int gg = 2 * half; gg < 2 * half + 2; ++gg) {
              const int t = wave * 16 + jj;
              const int bb = t / T_img, rem = t % T_img, th = rem / W2, tw = rem % W2;
              const int pix = (base[bb] + 2 * (th - th_lo[bb]) + r) * RW + 2 * tw + q;
              const int w0 = xswz(2 * pix + (gg >> 1)) * 4 + (gg & 1) * 2;
              words[n++] = w0;
              words[n++] = w0 + 1;
            }
          for (int bank = 0; bank < 64; ++bank) {
            int distinct[64];
            int nd = 0;
            for (int a = 0; a < n; ++a) {
              if ((words[a] & 63) != bank) continue;
              bool seen = false;
              for (int z = 0; z < nd; ++z) seen |= distinct[z] == words[a];
              if (!seen) distinct[nd++] = words[a];
            }
            if (nd > 1) total += nd - 1;
          }
        }
  return total;
}

static SpanGeom span_geometry(int H, int W) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, SpanGeom> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({H, W});
  if (it != cache.end()) return it->second;
  SpanGeom gm;
  const int H2 = H / 2, W2 = W / 2, T_img = H2 * W2;
  if (T_img > 0) {
    // worst case over the block start phases t0 mod T_img (P large enough that no block is cut)
    int rows = 0, segs = 0;
    bool fits = true;
    for (int ph = 0; ph < T_img && fits; ++ph) {
      int base[MAX_SEG + 1], th_lo[MAX_SEG];
      const int t0 = ph;  // a block starting at phase ph of an image
      const int span_imgs = (ph + 63) / T_img + 1;
      if (span_imgs > MAX_SEG) fits = false;
      span_rows(t0, t0 + 64 + 4 * T_img, T_img, W2, H2, base, th_lo);
      rows = std::max(rows, base[MAX_SEG]);
      segs = std::max(segs, span_imgs);
    }
    int best = -1;
    for (int RW = W + 2; fits && RW < W + 18; ++RW) {
      const int items = 2 * rows * RW;
      const int rounds = (items + 255) / 256;
      if (rounds * 256 * 16 > W_XS * 4) continue;
      const int cost = span_conflicts(W2, H2, RW) * 4 + rounds;
      if (best < 0 || cost < best) {
        best = cost;
        gm.ok = true;
        gm.RW = RW;
        gm.rounds = rounds;
        gm.rows = rows;
      }
    }
    (void)segs;
  }
  cache[{H, W}] = gm;
  return gm;
}

}  // namespace tp

extern "C" int tp_wino_taylor_slots(int H, int W) { return tp::wino_taylor_slots(H, W); }

// w: (S0, S1, 3, 3) = the forward weight (Cout, Cin, 3, 3), possibly narrower than the padded
// GEMM: flip_t = 0 -> U of (K = Cout_p, C = Cin_p); flip_t = 1 -> the dgrad operand, (K = Cin_p,
// C = Cout_p) with rotated taps. u: (C/8, K/32, 4096) images. K % 32 == 0, C % 8 == 0.
extern "C" hipError_t tp_wino_weights(const float* w, float* u, int K, int C, int flip_t, int S0, int S1,
                                      hipStream_t st) {
  if (K % 32 || C % 8 || K <= 0 || C <= 0 || S0 <= 0 || S1 <= 0) return hipErrorInvalidValue;
  if (flip_t ? (S0 > C || S1 > K) : (S0 > K || S1 > C)) return hipErrorInvalidValue;
  const long long total = (long long)(C / 8) * (K / 32) * tp::W_UIMG;
  const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 16384);
  tp::wino_weight_transform<<<grid, 256, 0, st>>>(w, u, K, C, flip_t, S0, S1);
  return hipGetLastError();
}

// the bf16 images of the BF kernels: u = (C/8, K/32, 4096) bf16 (2048 dwords per image)
extern "C" hipError_t tp_wino_weights_bf16(const float* w, void* u, int K, int C, int flip_t, int S0, int S1,
                                           hipStream_t st) {
  if (K % 32 || C % 8 || K <= 0 || C <= 0 || S0 <= 0 || S1 <= 0) return hipErrorInvalidValue;
  if (flip_t ? (S0 > C || S1 > K) : (S0 > K || S1 > C)) return hipErrorInvalidValue;
  const long long total = (long long)(C / 8) * (K / 32) * (tp::W_UIMG / 2);
  const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 16384);
  tp::wino_weight_transform_bf16<<<grid, 256, 0, st>>>(w, static_cast<unsigned*>(u), K, C, flip_t, S0, S1);
  return hipGetLastError();
}

// static LDS bytes of the largest Winograd kernel instantiations (occupancy guard)
extern "C" int tp_wino_lds_bytes() {
  using namespace tp;
  const void* fns[] = {(const void*)wino_f2x3<W_FWD, X_STAGED>, (const void*)wino_f2x3<W_FWD_POOL, X_STAGED>,
                       (const void*)wino_f2x3<W_BWD, X_STAGED_UNPOOL>, (const void*)wino_f2x3<W_BWD, X_SPAN>,
                       (const void*)wino_f2x3<W_PARTIAL, X_STAGED>, (const void*)wino_f2x3<W_BWD, X_STAGED, 1>,
                       (const void*)wino_f2x3<W_FWD_POOL, X_STAGED, 1>, (const void*)wino_f2x3<W_BWD, X_STAGED_UNPOOL, 1>};
  int worst = 0;
  for (const void* f : fns) {
    hipFuncAttributes a{};
    if (hipFuncGetAttributes(&a, f) != hipSuccess) return -1;
    worst = std::max(worst, (int)a.sharedSizeBytes);
  }
  return worst;
}

extern "C" int tp_wino_staged_ok(int H, int W, int unpool) {
  return tp::staged_geometry(H, W, unpool != 0).ok ? 1 : 0;
}

// host-side introspection (tests, tuning): {ok, n_img, R, RW, IP, rounds, arounds, aoff, conflicts}
extern "C" void tp_wino_geometry(int H, int W, int unpool, int* out9) {
  const tp::XGeom g = tp::staged_geometry(H, W, unpool != 0);
  const int vals[9] = {g.ok, g.n_img, g.R, g.RW, g.IP, g.rounds, g.arounds, g.aoff,
                       g.ok ? tp::staged_conflicts(W / 2, (H / 2) * (W / 2), g.RW, g.IP, unpool != 0) : -1};
  for (int i = 0; i < 9; ++i) out9[i] = vals[i];
}

// Winograd conv: same operand/epilogue contract as tp_conv_igemm (3x3, stride 1, pad 1),
// ``u`` = U images from winograd_weights(). epi: 0 fwd, 1 fwd+pool, 2 bwd (dgrad epilogue).
// H, W even, C % 8 == 0, K % 32 == 0. splits > 1 -> partial slabs in ``ws`` + combine.
// staged: bit 0 = LDS-staged input region when the shape allows it (else direct loads); bit 1 =
// ``u`` holds bf16 images (tp_wino_weights_bf16) for the BF kernels — staged input modes only.
extern "C" hipError_t tp_conv_wino(const float* x, const uint8_t* x_argmax, const float* u, int B, int H, int W,
                                   int C, int K, int unpool, int epi, int splits, int staged, const float* scale,
                                   const float* shift, int relu, float* out, uint8_t* out_argmax, const float* act,
                                   float* taylor, float* apoz, float* ws, int tay_mode, hipStream_t st) {
  using namespace tp;
  // odd H / W: a partial last tile row / column, direct loads only (no pooling / unpooling)
  const bool odd = (H & 1) || (W & 1);
  if ((odd && (unpool || epi == W_FWD_POOL)) || C % 8 != 0 || K % 32 != 0) return hipErrorInvalidValue;
  const bool bf = (staged & 2) != 0;
  staged &= 1;
  if (odd) staged = 0;
  WinoArgs a{};
  a.x = x;
  a.x_argmax = x_argmax;
  a.u = u;
  a.B = B;
  a.H = H;
  a.W = W;
  a.C = C;
  a.K = K;
  a.P = B * ((H + 1) / 2) * ((W + 1) / 2);
  a.x_elems = unpool ? (long long)B * (H / 2) * (W / 2) * C : (long long)B * H * W * C;
  if (a.x_elems * 4 >= (1ll << 31) || 16ll * C * K * 4 >= (1ll << 31)) return hipErrorInvalidValue;
  if (epi == W_BWD && (long long)B * H * W * K * 4 >= (1ll << 31)) return hipErrorInvalidValue;  // act rsrc
  const int chunks = C / 8;
  splits = std::max(1, std::min(splits, chunks));
  a.c_per_split = ((chunks + splits - 1) / splits) * 8;
  splits = (C + a.c_per_split - 1) / a.c_per_split;
  a.scale = scale;
  a.shift = shift;
  a.relu = relu;
  a.out = out;
  a.out_argmax = out_argmax;
  a.act = act;
  a.taylor = taylor;
  a.tay_mode = tay_mode;
  a.apoz = (epi == W_FWD || epi == W_FWD_POOL) ? apoz : nullptr;
  if (apoz && epi != W_FWD && epi != W_FWD_POOL) return hipErrorInvalidValue;
  a.tay_slots = wino_taylor_slots(H, W);
  a.fd_timg = FastDiv((unsigned)std::max(1, ((H + 1) / 2) * ((W + 1) / 2)));
  a.fd_w2 = FastDiv((unsigned)std::max(1, (W + 1) / 2));
#ifdef TP_WINO_DEBUG
  static const int dbg_bits = [] {
    const char* d = getenv("TP_WINO_DBG");
    const int v = d ? atoi(d) : 0;
    if (v) fprintf(stderr, "[tpamd] WARNING: TP_WINO_DBG=%d: Winograd results are WRONG (phase-cost experiment)\n", v);
    return v;
  }();
  a.dbg = dbg_bits;
#endif
  int xmode = unpool ? X_UNPOOL : X_DIRECT;
  static const bool span_ok = getenv("TP_WINO_NOSPAN") == nullptr;  // experiments only; read once at load
  if (staged && !unpool && !staged_geometry(H, W, false).ok && span_ok) {
    const SpanGeom sg = span_geometry(H, W);
    if (sg.ok) {
      xmode = X_SPAN;
      a.RW = sg.RW;
      a.rounds = sg.rounds;
      a.fd_rw = FastDiv((unsigned)sg.RW);
    }
  }
  if (staged && xmode != X_SPAN) {
    const XGeom gm = staged_geometry(H, W, unpool != 0);
    if (gm.ok) {
      xmode = unpool ? X_STAGED_UNPOOL : X_STAGED;
      a.n_img = gm.n_img;
      a.R = gm.R;
      a.RW = gm.RW;
      a.IP = gm.IP;
      a.rounds = gm.rounds;
      a.arounds = gm.arounds;
      a.aoff = gm.aoff;
      a.fd_ip = FastDiv((unsigned)gm.IP);
      a.fd_rw = FastDiv((unsigned)gm.RW);
    }
  }
  const int n_p = (a.P + 63) / 64, n_k = K / 32;
  dim3 grid(n_p * n_k, splits);
  int e_launch = epi;
  if (splits > 1) {
    if (!ws) return hipErrorInvalidValue;
    a.out = ws;
    a.pooled_m = epi == W_FWD_POOL ? 1 : 0;
    e_launch = W_PARTIAL;
  }
  if (bf && xmode != X_STAGED && xmode != X_SPAN && xmode != X_STAGED_UNPOOL) return hipErrorInvalidValue;
  static const bool bf_split = getenv("TP_WINO_BF_SPLIT") != nullptr;  // measured option: V as bf16 hi + lo
  static const bool k16_ok = getenv("TP_WINO_BF_K16") != nullptr;  // measured option: 16-channel bf16 chunks
  const bool k16 = bf && !bf_split && k16_ok && xmode == X_STAGED && a.rounds <= 3 && C % 16 == 0;
  if (k16) {  // 16-channel stages: the channel split granule is 16
    const int c16 = C / 16;
    int sp16 = std::max(1, std::min(splits, c16));
    a.c_per_split = ((c16 + sp16 - 1) / sp16) * 16;
    splits = (C + a.c_per_split - 1) / a.c_per_split;
    grid.y = splits;
    if (splits == 1 && e_launch == W_PARTIAL) {  // the 16-channel granule left one split: no slabs
      a.out = out;
      e_launch = epi;
    }
  }
#define TP_W(E)                                                                                 \
  do {                                                                                          \
    if (k16) {                                                                                  \
      wino_f2x3<E, X_STAGED, 3><<<grid, 256, 0, st>>>(a);                                       \
    } else if (bf && bf_split) {                                                                \
      if (xmode == X_STAGED) wino_f2x3<E, X_STAGED, 2><<<grid, 256, 0, st>>>(a);               \
      else if (xmode == X_SPAN) wino_f2x3<E, X_SPAN, 2><<<grid, 256, 0, st>>>(a);              \
      else wino_f2x3<E, X_STAGED_UNPOOL, 2><<<grid, 256, 0, st>>>(a);                          \
    } else if (bf) {                                                                            \
      if (xmode == X_STAGED) wino_f2x3<E, X_STAGED, 1><<<grid, 256, 0, st>>>(a);               \
      else if (xmode == X_SPAN) wino_f2x3<E, X_SPAN, 1><<<grid, 256, 0, st>>>(a);              \
      else wino_f2x3<E, X_STAGED_UNPOOL, 1><<<grid, 256, 0, st>>>(a);                          \
    } else if (xmode == X_STAGED) wino_f2x3<E, X_STAGED><<<grid, 256, 0, st>>>(a);             \
    else if (xmode == X_SPAN) wino_f2x3<E, X_SPAN><<<grid, 256, 0, st>>>(a);                   \
    else if (xmode == X_STAGED_UNPOOL) wino_f2x3<E, X_STAGED_UNPOOL><<<grid, 256, 0, st>>>(a);  \
    else if (xmode == X_UNPOOL) wino_f2x3<E, X_UNPOOL><<<grid, 256, 0, st>>>(a);               \
    else wino_f2x3<E, X_DIRECT><<<grid, 256, 0, st>>>(a);                                      \
  } while (0)
  if (e_launch == W_FWD) TP_W(W_FWD);
  else if (e_launch == W_FWD_POOL) {
    if (unpool) return hipErrorInvalidValue;
    TP_W(W_FWD_POOL);
  } else if (e_launch == W_BWD) TP_W(W_BWD);
  else TP_W(W_PARTIAL);
#undef TP_W
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || splits == 1) return e;
  return tp_conv_epilogue_slabs(ws, splits, B, H, W, K, epi, scale, shift, relu, out, out_argmax, act, taylor,
                                a.apoz, tay_mode, st);
}
