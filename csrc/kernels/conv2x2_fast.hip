// 3x3 / pad-1 convolution on 2x2 maps with 9 channel products per image instead of the dense
// GEMM's 16 (fused_chain.py DENSE). On a 2-pixel row the conv is a 2x2 Toeplitz product,
//   y0 = W1 x0 + W2 x1,  y1 = W0 x0 + W1 x1,
// which takes 3 multiplications: m_s = W1 (x0 + x1), m_1 = (W2 - W1) x1, m_0 = (W0 - W1) x0,
// y0 = m_s + m_1, y1 = m_s + m_0. Nested in both dimensions:
//   V = Bt x Bt^T,  U = G w G^T,  M[i][j] = sum_c V[i][j][c] U[i][j][c][k],  Y = At M At^T
//   Bt = [[1,1],[0,1],[1,0]],  G = [[0,1,0],[0,-1,1],[1,-1,0]],  At = [[1,1,0],[1,0,1]].
// Three launches per conv: the input transform x (B,2,2,C) -> V (9,B,C) (optionally unpooling a
// pooled gradient through its argmax bytes first), nine independent (B x C).(C x K) GEMMs in one
// conv_igemm launch (tp_conv_igemm_batched: raw slabs, optional split-K), and one combine that
// adds the 9 x splits slabs in a fixed order and applies the dense path's epilogue contracts
// (forward: BN affine, NaN-propagating ReLU, optional 2x2 max-pool + argmax byte in
// maxpool2_nhwc's convention; data gradient: ReLU-mask x BN-scale output and Taylor / Sensitivity
// partials, one slot per pixel). Deterministic: no atomics. The data gradient is the same
// algorithm on the flipped, transposed weight. The coefficients are 0 and +-1 only: the fp32
// error stays at the 1e-6 level (V sums at most 4 pixels, Y at most 4 products).
#include "tp_common.h"
#include "tp_launchers.h"

namespace tp {

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// V[i*3+j] = sum_{a,b} Bt[i][a] Bt[j][b] x[a][b]; one thread per (image, 4 channels).
// UNPOOL: x is the pooled gradient (B, C) and ``am`` its argmax bytes: pixel q holds the value
// where am == q and zero elsewhere (unpool2_nhwc).
template <bool UNPOOL>
__global__ __launch_bounds__(256) void fast2x2_transform(const float4* __restrict__ x, const uint32_t* __restrict__ am,
                                                         float4* __restrict__ V, int C4, long long total) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    float4 p[4];
    if constexpr (UNPOOL) {
      const float4 v = x[t];
      const uint32_t a = am[t];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        p[q].x = ((a >> 0) & 0xffu) == (uint32_t)q ? v.x : 0.f;
        p[q].y = ((a >> 8) & 0xffu) == (uint32_t)q ? v.y : 0.f;
        p[q].z = ((a >> 16) & 0xffu) == (uint32_t)q ? v.z : 0.f;
        p[q].w = ((a >> 24) & 0xffu) == (uint32_t)q ? v.w : 0.f;
      }
    } else {
      const long long b = t / C4;
      const long long o = b * 4 * C4 + (t - b * C4);
#pragma unroll
      for (int q = 0; q < 4; ++q) p[q] = x[o + (long long)q * C4];
    }
    const float4 r0 = add4(p[0], p[1]), r1 = add4(p[2], p[3]);  // row sums
    const float4 c0 = add4(p[0], p[2]), c1 = add4(p[1], p[3]);  // column sums
    V[0 * total + t] = add4(r0, r1);
    V[1 * total + t] = c1;
    V[2 * total + t] = c0;
    V[3 * total + t] = r1;
    V[4 * total + t] = p[3];
    V[5 * total + t] = p[2];
    V[6 * total + t] = r0;
    V[7 * total + t] = p[1];
    V[8 * total + t] = p[0];
  }
}

// M[i*3+j] = the product's slabs summed over the splits in order, then Y = At M At^T in a fixed
// order: y[q = 2a + b] = sum_{i in {0, 1+a}} sum_{j in {0, 1+b}} M[i][j].
__device__ __forceinline__ void fast2x2_output(const float4* __restrict__ S, int splits, long long total, long long t,
                                               float4 y[4]) {
  float4 m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    float4 v = S[(long long)i * splits * total + t];
    for (int s = 1; s < splits; ++s) v = add4(v, S[((long long)i * splits + s) * total + t]);
    m[i] = v;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = 1 + (q >> 1), j = 1 + (q & 1);
    y[q] = add4(add4(add4(m[0], m[j]), m[3 * i]), m[3 * i + j]);
  }
}

// forward combine: y = relu?(Y * scale + shift) stored (B,2,2,N), or POOL: the 2x2 max (first
// max wins, NaN wins over numbers: maxpool2_nhwc) stored (B,N) with its argmax byte
template <bool POOL>
__global__ __launch_bounds__(256) void fast2x2_combine_fwd(const float4* __restrict__ S, int splits,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, int relu,
                                                           float4* __restrict__ out, uint32_t* __restrict__ out_am,
                                                           int N4, long long total) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const long long b = t / N4;
    const int n4 = (int)(t - b * N4);
    float4 y[4];
    fast2x2_output(S, splits, total, t, y);
    const float4 sc = scale ? *reinterpret_cast<const float4*>(scale + 4 * n4) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 sh = shift ? *reinterpret_cast<const float4*>(shift + 4 * n4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      y[q].x = y[q].x * sc.x + sh.x;
      y[q].y = y[q].y * sc.y + sh.y;
      y[q].z = y[q].z * sc.z + sh.z;
      y[q].w = y[q].w * sc.w + sh.w;
      if (relu) {
        y[q].x = nan_relu(y[q].x);
        y[q].y = nan_relu(y[q].y);
        y[q].z = nan_relu(y[q].z);
        y[q].w = nan_relu(y[q].w);
      }
    }
    if constexpr (POOL) {
      float4 best = y[0];
      uint32_t arg = 0;
#pragma unroll
      for (int q = 1; q < 4; ++q) {
#define TP_F2_MAX(f, sh_)                                           \
  if (y[q].f > best.f || (y[q].f != y[q].f && best.f == best.f)) { \
    best.f = y[q].f;                                                \
    arg = (arg & ~(0xffu << sh_)) | ((uint32_t)q << sh_);           \
  }
        TP_F2_MAX(x, 0)
        TP_F2_MAX(y, 8)
        TP_F2_MAX(z, 16)
        TP_F2_MAX(w, 24)
#undef TP_F2_MAX
      }
      out[t] = best;
      out_am[t] = arg;
    } else {
      const long long o = b * 4 * N4 + n4;
#pragma unroll
      for (int q = 0; q < 4; ++q) out[o + (long long)q * N4] = y[q];
    }
  }
}

// data-gradient combine (the EPI_BWD contract of conv_mfma.hip with tay_group = C): g = Y is
// dL/d(act); out (B,2,2,C) = act > 0 ? g * bn_scale : 0 (nullable); taylor (4,B,C), slot = pixel,
// += -(g * act) (tay_mode 1: |g|, 2: |g| where act > 0), nullable
__global__ __launch_bounds__(256) void fast2x2_combine_bwd(const float4* __restrict__ S, int splits,
                                                           const float4* __restrict__ act,
                                                           const float* __restrict__ scale, float4* __restrict__ out,
                                                           float4* __restrict__ taylor, int tay_mode, int N4,
                                                           long long total) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const long long b = t / N4;
    const int n4 = (int)(t - b * N4);
    float4 y[4];
    fast2x2_output(S, splits, total, t, y);
    const float4 sc = scale ? *reinterpret_cast<const float4*>(scale + 4 * n4) : make_float4(1.f, 1.f, 1.f, 1.f);
    const long long o = b * 4 * N4 + n4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 a = act[o + (long long)q * N4];
      const float4 g = y[q];
      if (taylor) {
        float4 tv = taylor[(long long)q * total + t];
        tv.x += tay_term(tay_mode, g.x, a.x);
        tv.y += tay_term(tay_mode, g.y, a.y);
        tv.z += tay_term(tay_mode, g.z, a.z);
        tv.w += tay_term(tay_mode, g.w, a.w);
        taylor[(long long)q * total + t] = tv;
      }
      if (out) {
        out[o + (long long)q * N4] = make_float4(act_grad(a.x, g.x * sc.x, 0.f), act_grad(a.y, g.y * sc.y, 0.f),
                                                 act_grad(a.z, g.z * sc.z, 0.f), act_grad(a.w, g.w * sc.w, 0.f));
      }
    }
  }
}

}  // namespace tp

namespace {

inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// shapes both directions share: B images, Cin -> Cout channels (the GEMMs are (B x Cin).(Cin x Cout))
bool bad_shape(int B, int Cin, int Cout, int cfg, int splits) {
  if (B < 1 || Cin < 32 || Cin % 32 != 0 || Cout < 4 || Cout % 4 != 0 || cfg < 0 || cfg > 6 || splits < 1) return true;
  if (splits != tp_conv_norm_splits(splits, Cin) || 9ll * splits > 65535) return true;
  // per-batch operands below 2^31 bytes (buffer descriptors), 32-bit tile indices
  const long long lim = 1ll << 29;
  return (long long)B * Cin >= lim || (long long)B * Cout >= lim || (long long)Cin * Cout >= lim;
}

unsigned grid_for(long long total) { return (unsigned)std::min<long long>(tp::ceil_div(total, 256), 16384); }

}  // namespace

// Forward. x (B,2,2,C) NHWC; u9 (9,K,C) = G w G^T per (output, input) channel pair; V (9,B,C) and
// slabs (9*splits,B,K) workspaces; out (B,2,2,K), or pool: (B,K) + argmax bytes (B,K).
extern "C" hipError_t tp_conv2x2_fast_fwd(const float* x, const float* u9, int B, int C, int K, int cfg, int splits,
                                          const float* scale, const float* shift, int relu, int pool, float* out,
                                          uint8_t* out_argmax, float* V, float* slabs, hipStream_t st) {
  if (bad_shape(B, C, K, cfg, splits)) return hipErrorInvalidValue;
  if (!x || !u9 || !out || !V || !slabs || (pool && !out_argmax)) return hipErrorInvalidValue;
  if (misaligned16(x) || misaligned16(u9) || misaligned16(out) || misaligned16(V) || misaligned16(slabs) ||
      misaligned16(scale) || misaligned16(shift) || (reinterpret_cast<uintptr_t>(out_argmax) & 3))
    return hipErrorInvalidValue;
  const long long tin = (long long)B * (C / 4), tout = (long long)B * (K / 4);
  tp::fast2x2_transform<false><<<grid_for(tin), 256, 0, st>>>(reinterpret_cast<const float4*>(x), nullptr,
                                                              reinterpret_cast<float4*>(V), C / 4, tin);
  TP_HIP_CHECK(hipGetLastError());
  TP_HIP_CHECK(tp_conv_igemm_batched(V, u9, 9, B, C, K, cfg, splits, slabs, st));
  if (pool)
    tp::fast2x2_combine_fwd<true><<<grid_for(tout), 256, 0, st>>>(
        reinterpret_cast<const float4*>(slabs), splits, scale, shift, relu, reinterpret_cast<float4*>(out),
        reinterpret_cast<uint32_t*>(out_argmax), K / 4, tout);
  else
    tp::fast2x2_combine_fwd<false><<<grid_for(tout), 256, 0, st>>>(reinterpret_cast<const float4*>(slabs), splits,
                                                                   scale, shift, relu, reinterpret_cast<float4*>(out),
                                                                   nullptr, K / 4, tout);
  return hipGetLastError();
}

// Data gradient. g (B,2,2,Cg), or with g_argmax the pooled gradient (B,Cg) + argmax bytes; u9t
// (9,Cin,Cg) = G w' G^T of the flipped, transposed weight; act (B,2,2,Cin); out (B,2,2,Cin)
// nullable; taylor (4,B,Cin) nullable (accumulated); V (9,B,Cg), slabs (9*splits,B,Cin).
extern "C" hipError_t tp_conv2x2_fast_dgrad(const float* g, const uint8_t* g_argmax, const float* u9t, int B, int Cg,
                                            int Cin, int cfg, int splits, const float* act, const float* bn_scale,
                                            float* taylor, int tay_mode, float* out, float* V, float* slabs,
                                            hipStream_t st) {
  if (bad_shape(B, Cg, Cin, cfg, splits) || tay_mode < 0 || tay_mode > 2) return hipErrorInvalidValue;
  if (!g || !u9t || !act || !V || !slabs || (!out && !taylor)) return hipErrorInvalidValue;
  if (misaligned16(g) || misaligned16(u9t) || misaligned16(act) || misaligned16(V) || misaligned16(slabs) ||
      misaligned16(bn_scale) || misaligned16(taylor) || misaligned16(out) ||
      (reinterpret_cast<uintptr_t>(g_argmax) & 3))
    return hipErrorInvalidValue;
  const long long tin = (long long)B * (Cg / 4), tout = (long long)B * (Cin / 4);
  if (g_argmax)
    tp::fast2x2_transform<true><<<grid_for(tin), 256, 0, st>>>(reinterpret_cast<const float4*>(g),
                                                               reinterpret_cast<const uint32_t*>(g_argmax),
                                                               reinterpret_cast<float4*>(V), Cg / 4, tin);
  else
    tp::fast2x2_transform<false><<<grid_for(tin), 256, 0, st>>>(reinterpret_cast<const float4*>(g), nullptr,
                                                                reinterpret_cast<float4*>(V), Cg / 4, tin);
  TP_HIP_CHECK(hipGetLastError());
  TP_HIP_CHECK(tp_conv_igemm_batched(V, u9t, 9, B, Cg, Cin, cfg, splits, slabs, st));
  tp::fast2x2_combine_bwd<<<grid_for(tout), 256, 0, st>>>(reinterpret_cast<const float4*>(slabs), splits,
                                                          reinterpret_cast<const float4*>(act), bn_scale,
                                                          reinterpret_cast<float4*>(out),
                                                          reinterpret_cast<float4*>(taylor), tay_mode, Cin / 4, tout);
  return hipGetLastError();
}
