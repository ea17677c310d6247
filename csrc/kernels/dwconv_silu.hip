// Depthwise convolutions of the attribution path with SiLU on either side (the hidden layer of an
// eval-mode EfficientNet MBConv block), fp32 NHWC, BN affine fused:
//
//   forward  v  = scale[c] * dwconv(in_act(x))[c] + shift[c],  y = v * sigmoid(v)
//            (+ v into `pre`, + APoZ counts of y > 0, + per-block sums of y: the gate's pool partials)
//   dgrad    dA = gather(g * scale[c] * silu'(v)),  silu'(v) = s * (1 + v * (1 - s)),  s = sigmoid(v)
//            tay[slot, b, c] = sum over the block's pixels of -(dA * a) or |dA|,  a = in_act(z)
//            dz = dA * in_act'(z)
//
// Activation codes: 0 none, 4 SiLU (codes 1..3 stay on dwconv_act.hip); the output's is always 4.
//
// These are not instantiations of dwconv_act.hip's templates. There a thread activates every tap it
// loads, once per kernel row: K evaluations per element, a clamp each. A SiLU is an exponential and
// a reciprocal (quarter-rate), so here the activated operand is STAGED in the LDS and every staged
// element is evaluated once:
//
//   block    256 threads = QB channel quads x TW columns (QB * TW = 256; TW in {8, 16, 32} is the
//            smallest that holds the column band, so a 7-pixel map takes 32 quads = 128 channels per
//            block and a 112-pixel one four bands of 28 columns x 8 quads). Lanes run over
//            consecutive quads of a pixel first: 8 lanes read or write one full 128-byte line, and an
//            LDS row is [column][quad] float4, so a wave's ds_read_b128 of one tap is contiguous
//            (stride 1) or 128-byte pieces (stride 2).
//   march    a block owns (image, row band, column band, channel slice) and walks down the output
//            rows of its band. The forward keeps a ring of input rows in the LDS (K + 1 rows, one
//            barrier per output row, for stride 1; K rows and two barriers for stride 2, which keeps
//            the 5x5 stride-2 tile at 48.6 KB); the S rows of the next step are loaded into registers
//            before the current row is computed and activated + written to the ring after it. A
//            thread computes one output pixel of its quad per row: K * K LDS reads, weights in
//            registers. The dgrad marches down the INPUT rows over a ring of g' = g * scale * silu'(v)
//            rows ((K - 1) / S + 2 of them); stride-2 parity: a thread whose (iw + pad) is odd takes
//            the odd taps, selected from registers with v_cndmask (no dynamic register index).
//   bands    rows are split into bands only while the grid is short of ~4 blocks per CU, into at most
//            (rows + 2) / 4 bands of equal height (rounded up): 4 rows where the map allows it, 3 for
//            a 6-row map, and the last band takes what is left (2 rows of a 14-row map).
//
// Halo factor (activations per input element). A band of r output rows and c output columns stages
// (r - 1) S + K rows of (c - 1) S + K columns, clipped to the image: only the columns its own taps
// read, not the tile's width; zero padding is not an input element and is not counted.
// EfficientNet-B0's forward layers at 224 px
// (input map, row bands x column bands in brackets), at the finest row split (B = 1) and at B = 32:
//   k3 s1 112 (C   32)   1.56 (28 x 4)   1.19 ( 8 x 4)      k5 s2  56 (C  160)   1.32 (7 x 1)   1.32
//   k3 s2 112 (C   96)   1.13 (14 x 2)   1.05 ( 6 x 2)      k5 s1  28 (C  256)   1.86 (7 x 1)   1.43 (4 x 1)
//   k3 s1  56 (C  160)   1.52 (14 x 2)   1.15 ( 4 x 2)      k5 s1  14 (C  480)   1.86 (4 x 1)   1.86
//   k3 s2  28 (C  256)   1.11 ( 4 x 1)   1.11               k5 s1  14 (C  672)   1.86 (4 x 1)   1.57 (3 x 1)
//   k3 s1  14 (C  480)   1.43 ( 4 x 1)   1.43               k5 s2  14 (C  672)   1.21 (2 x 1)   1.21
//   k3 s1   7 (C 1152)   1.29 ( 2 x 1)   1.29               k5 s1   7 (C 1152)   1.57 (2 x 1)   1.57
// so at most 1.56 for k = 3 (limit 1.6) and 1.86 for k = 5 (limit 2.3); 1.0 where a map is one block.
// LDS: at most 48,640 B of ring (5x5 stride 2, TW = 8) + 4,096 B of reduction buffer = 52,736 B per
// block, three blocks per CU of 160 KB. No scratch (profiles/silu/dwconv_silu_kernel_stats.txt).
//
// Partials: a thread sums its pixels in row order, the TW threads of a quad are summed in column
// order through the LDS, and the block stores into its own slot (row band x column band) of the
// (R, B, C) slab: one writer per element, no float atomics, bit-identical from run to run. The slot
// count is a function of the map alone (the finest split); a coarser split leaves slots of the zeroed
// slab untouched. APoZ counts are integers added with float atomics (exact up to 2^24).
//
// Numerics (the bn_silu contract): sigmoid(v) = 1 / (1 + exp(-v)) is 0 at v = -100 (exp overflows to
// +inf) and 1 at +100, so y and the slopes are finite there; NaN passes through; a padded channel
// (zero weights and affine, any finite z) has v = 0, y = 0, g' = g * 0 * 0.5 = 0, dA = 0 and
// dz = 0 * slope(z) = 0, every partial 0.
#include "tp_dwconv.h"
#include "tp_launchers.h"

#include <initializer_list>

namespace tp {

constexpr int DWS_T = 256;
constexpr int DWS_MIN_ROWS = 4;       // output rows per row band at the finest split: (rows + 2) / 4 bands
constexpr int DWS_WANT_BLOCKS = 1024;  // rows are split while the grid is below this

// one hardware exponential (v_exp_f32) and one reciprocal (v_rcp_f32) per value
__device__ __forceinline__ float dws_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.f + __expf(-v)); }

__device__ __forceinline__ float4 dws_silu4(float4 v) {
  return make_float4(v.x * dws_sigmoid(v.x), v.y * dws_sigmoid(v.y), v.z * dws_sigmoid(v.z), v.w * dws_sigmoid(v.w));
}
// silu and its derivative from one sigmoid
__device__ __forceinline__ void dws_silu_both(float v, float& a, float& d) {
  const float s = dws_sigmoid(v);
  a = v * s;
  d = s * fmaf(v, 1.f - s, 1.f);
}
__device__ __forceinline__ float dws_silu_slope(float v) {
  const float s = dws_sigmoid(v);
  return s * fmaf(v, 1.f - s, 1.f);
}

// How a (rows x cols x C) output map is cut into blocks; depends on B only through the row split
struct DwsTile {
  int tw, lq;    // columns per block (8 | 16 | 32), log2 of the quads per block (256 / tw)
  int ncb, bw;   // column bands, columns per band (<= tw)
  int nsl;       // channel slices of QB quads
  int nrb, rbh;  // row bands, rows per band
  int slots;     // (finest row split) x column bands: the partial slab's slot count
};

static bool dws_tile(int B, int rows, int cols, int C, DwsTile* t) {
  if (B < 1 || rows < 1 || cols < 1 || C < 4 || C % 4 != 0) return false;
  t->ncb = (int)ceil_div(cols, 32);
  t->bw = (int)ceil_div(cols, t->ncb);
  t->tw = t->bw <= 8 ? 8 : t->bw <= 16 ? 16 : 32;
  t->lq = t->tw == 8 ? 5 : t->tw == 16 ? 4 : 3;
  t->nsl = (int)ceil_div(C / 4, DWS_T / t->tw);
  const long long finest = std::max(1ll, ((long long)rows + DWS_MIN_ROWS / 2) / DWS_MIN_ROWS);  // rows up to INT_MAX
  const long long slots = finest * t->ncb;
  if (slots >= (1ll << 24)) return false;
  t->slots = (int)slots;
  const long long base = (long long)B * t->ncb * t->nsl;
  const long long want = std::min(finest, (DWS_WANT_BLOCKS + base - 1) / base);
  t->rbh = (int)ceil_div(rows, want);
  t->nrb = (int)ceil_div(rows, t->rbh);
  return base * t->nrb < DW_MAX_BLOCKS;
}

// Sum of the float4 values of the threads that share a channel quad (threads qi, qi + QB, ...: column
// order) -> the thread of column 0. Every thread of the block calls this.
__device__ __forceinline__ bool dws_block_fold(float4* red, float4 mine, int QB, float4* out) {
  __syncthreads();  // the buffer's last readers
  red[threadIdx.x] = mine;
  __syncthreads();
  if ((int)threadIdx.x >= QB) return false;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = threadIdx.x; t < DWS_T; t += QB) {
    const float4 r = red[t];
    a.x += r.x, a.y += r.y, a.z += r.z, a.w += r.w;
  }
  *out = a;
  return true;
}

struct DwsGeo {
  int B, H, W, C, pad, Ho, Wo;  // H x W: the conv's input map, Ho x Wo: its output map
  int tw, lq, ncb, bw, nsl, nrb, rbh;
};

// block -> (image, row band, column band, channel slice)
__device__ __forceinline__ void dws_decode(const DwsGeo& G, int& b, int& rb, int& cb, int& sl) {
  int i = blockIdx.x;
  sl = i % G.nsl, i /= G.nsl;
  cb = i % G.ncb, i /= G.ncb;
  rb = i % G.nrb, b = i / G.nrb;
}

template <int K, int S>
__global__ __launch_bounds__(DWS_T, 2) void dwconv_silu_fwd_k(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift, float* __restrict__ y,
                                                              float* __restrict__ pre, float* __restrict__ apoz,
                                                              float* __restrict__ pool, DwsGeo G, int in_silu) {
  constexpr int KK = K * K, RING = S == 1 ? K + 1 : K, NLD = S + 1;
  extern __shared__ float4 dws_lds[];
  const int QB = 1 << G.lq, ncin = (G.tw - 1) * S + K;  // staged columns of a row
  float4* red = dws_lds + RING * ncin * QB;
  const int qi = threadIdx.x & (QB - 1), cs = threadIdx.x >> G.lq;
  int b, rb, cb, sl;
  dws_decode(G, b, rb, cb, sl);
  const int c = (sl * QB + qi) * 4;
  const bool qok = c < G.C;
  const int oc0 = cb * G.bw, ocn = min(G.bw, G.Wo - oc0);
  const int r0 = rb * G.rbh, r1 = min(r0 + G.rbh, G.Ho);
  const int ic0 = oc0 * S - G.pad;
  const int nst = (ocn - 1) * S + K;  // columns the band's taps read (<= ncin): no other is staged
  const bool active = qok && cs < ocn;
  float wf[4 * KK];
  float4 sc = make_float4(0.f, 0.f, 0.f, 0.f), sh = sc;
#pragma unroll
  for (int i = 0; i < 4 * KK; ++i) wf[i] = 0.f;
  if (qok) {
    dw_load_w<4, KK>(w, c, wf);
    sc = *reinterpret_cast<const float4*>(scale + c);
    sh = *reinterpret_cast<const float4*>(shift + c);
  }
  const float* xb = x + b * G.H * G.W * G.C + c;

  // rows of the input are staged whole (the band's columns + halo): thread -> columns cs, cs + TW, ...
  float4 pf[S][NLD];
  auto fetch = [&](int ih, float4* p) {  // raw loads, zeros outside the image
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int iw = ic0 + cs + i * G.tw;
      p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (qok && cs + i * G.tw < nst && ih >= 0 && ih < G.H && iw >= 0 && iw < G.W)
        p[i] = *reinterpret_cast<const float4*>(xb + (ih * G.W + iw) * G.C);
    }
  };
  auto commit = [&](int ih, const float4* p) {  // activate once, write to the row's ring slot
    if (ih < 0 || ih >= G.H) return;            // rows outside the image are skipped by the taps
    float4* row = dws_lds + ((ih + G.pad) % RING) * ncin * QB + qi;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int col = cs + i * G.tw;
      if (col < nst) row[col * QB] = in_silu ? dws_silu4(p[i]) : p[i];  // silu(0) == 0: padding stays 0
    }
  };

  for (int ih = r0 * S - G.pad; ih < r0 * S - G.pad + K; ++ih) {  // the first window
    fetch(ih, pf[0]);
    commit(ih, pf[0]);
  }
  __syncthreads();
  float4 cnt = make_float4(0.f, 0.f, 0.f, 0.f), psum = cnt;
  for (int oh = r0; oh < r1; ++oh) {
    const int ih0 = oh * S - G.pad;
    const bool more = oh + 1 < r1;  // block-uniform
    if (more) {
#pragma unroll
      for (int r = 0; r < S; ++r) fetch(ih0 + K + r, pf[r]);
    }
    if (active) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        const int ih = ih0 + kh;
        if (ih < 0 || ih >= G.H) continue;  // block-uniform
        const float4* row = dws_lds + (((ih + G.pad) % RING) * ncin + cs * S) * QB + qi;
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const float4 v = row[kw * QB];
          acc[0] = fmaf(v.x, wf[0 * KK + kh * K + kw], acc[0]);
          acc[1] = fmaf(v.y, wf[1 * KK + kh * K + kw], acc[1]);
          acc[2] = fmaf(v.z, wf[2 * KK + kh * K + kw], acc[2]);
          acc[3] = fmaf(v.w, wf[3 * KK + kh * K + kw], acc[3]);
        }
      }
      const float4 v = make_float4(fmaf(sc.x, acc[0], sh.x), fmaf(sc.y, acc[1], sh.y), fmaf(sc.z, acc[2], sh.z),
                                   fmaf(sc.w, acc[3], sh.w));
      const int o = ((b * G.Ho + oh) * G.Wo + oc0 + cs) * G.C + c;
      if (pre != nullptr) *reinterpret_cast<float4*>(pre + o) = v;
      const float4 a = dws_silu4(v);
      *reinterpret_cast<float4*>(y + o) = a;
      cnt.x += a.x > 0.f ? 1.f : 0.f, cnt.y += a.y > 0.f ? 1.f : 0.f;
      cnt.z += a.z > 0.f ? 1.f : 0.f, cnt.w += a.w > 0.f ? 1.f : 0.f;
      psum.x += a.x, psum.y += a.y, psum.z += a.z, psum.w += a.w;
    }
    if (more) {
      if constexpr (RING < K + S) __syncthreads();  // the slots written next are still being read
#pragma unroll
      for (int r = 0; r < S; ++r) commit(ih0 + K + r, pf[r]);
      __syncthreads();
    }
  }
  float4 tot;
  if (apoz != nullptr && dws_block_fold(red, cnt, QB, &tot) && qok) {  // the pointer tests are block-uniform
    float* ap = apoz + b * G.C + c;
    if (tot.x != 0.f) atomicAdd(ap + 0, tot.x);
    if (tot.y != 0.f) atomicAdd(ap + 1, tot.y);
    if (tot.z != 0.f) atomicAdd(ap + 2, tot.z);
    if (tot.w != 0.f) atomicAdd(ap + 3, tot.w);
  }
  if (pool != nullptr && dws_block_fold(red, psum, QB, &tot) && qok)
    *reinterpret_cast<float4*>(pool + ((rb * G.ncb + cb) * G.B + b) * G.C + c) = tot;
}

// The gather form of the input gradient: the block marches down the rows ih of its band of dA (the
// conv's INPUT map) and stages rows oh of g' = g * scale * silu'(v) (the conv's OUTPUT map): a tap
// (kh, kw) of dA[ih, iw] reads g'[(ih + pad - kh) / S, (iw + pad - kw) / S] where both divide.
template <int K, int S>
__global__ __launch_bounds__(DWS_T, 2) void dwconv_silu_dgrad_k(const float* __restrict__ g, const float* __restrict__ v,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ z, float* __restrict__ dz,
                                                                float* __restrict__ tay, DwsGeo G, int in_silu,
                                                                int tay_mode) {
  constexpr int KK = K * K, KR = (K - 1) / S + 1, RING = KR + 1, NLD = S == 1 ? 2 : 1, NT = (K + S - 1) / S;
  extern __shared__ float4 dws_lds[];
  const int QB = 1 << G.lq, ncg = (G.tw + K - 2) / S + 2;  // staged columns of a g' row
  float4* red = dws_lds + RING * ncg * QB;
  const int qi = threadIdx.x & (QB - 1), cs = threadIdx.x >> G.lq;
  int b, rb, cb, sl;
  dws_decode(G, b, rb, cb, sl);
  const int c = (sl * QB + qi) * 4;
  const bool qok = c < G.C;
  const int c0 = cb * G.bw, cn = min(G.bw, G.W - c0);
  const int r0 = rb * G.rbh, r1 = min(r0 + G.rbh, G.H);
  const int ow_lo = (c0 + G.pad - K + 1 + 8 + S - 1) / S - 8 / S;  // ceil((c0 + pad - K + 1) / S)
  const int nst = (c0 + cn - 1 + G.pad) / S - ow_lo + 1;  // columns the band's taps read (<= ncg)
  const bool active = qok && cs < cn;
  float wf[4 * KK];
  float4 sc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < 4 * KK; ++i) wf[i] = 0.f;
  if (qok) {
    dw_load_w<4, KK>(w, c, wf);
    sc = *reinterpret_cast<const float4*>(scale + c);
  }
  const int ob = b * G.Ho * G.Wo * G.C + c;

  float4 pg[NLD], pv[NLD];
  auto fetch = [&](int oh) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int ow = ow_lo + cs + i * G.tw;
      pg[i] = pv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (qok && cs + i * G.tw < nst && oh >= 0 && oh < G.Ho && ow >= 0 && ow < G.Wo) {
        const int o = ob + (oh * G.Wo + ow) * G.C;
        pg[i] = *reinterpret_cast<const float4*>(g + o);
        pv[i] = *reinterpret_cast<const float4*>(v + o);
      }
    }
  };
  auto commit = [&](int oh) {  // the slope once per staged element; g = 0 outside the map stays 0
    if (oh < 0 || oh >= G.Ho) return;
    float4* row = dws_lds + (oh % RING) * ncg * QB + qi;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int col = cs + i * G.tw;
      if (col < nst)
        row[col * QB] = make_float4(pg[i].x * sc.x * dws_silu_slope(pv[i].x), pg[i].y * sc.y * dws_silu_slope(pv[i].y),
                                    pg[i].z * sc.z * dws_silu_slope(pv[i].z), pg[i].w * sc.w * dws_silu_slope(pv[i].w));
    }
  };

  // rows of g' the taps of input row ih read: floor((ih + pad - K + 1 + S - 1) / S) .. (ih + pad) / S
  for (int oh = (r0 + G.pad - K + 1 + 8 + S - 1) / S - 8 / S; oh <= (r0 + G.pad) / S; ++oh) {
    fetch(oh);
    commit(oh);
  }
  __syncthreads();
  float4 part = make_float4(0.f, 0.f, 0.f, 0.f);
  const int iw = c0 + cs;
  const int par = S == 2 ? ((iw + G.pad) & 1) : 0;     // this thread's taps: kw = par, par + S, ...
  const int colb = (iw + G.pad - par) / S - ow_lo;     // staged column of tap kw = par; tap j reads colb - j
  for (int ih = r0; ih < r1; ++ih) {
    const int nxt = ih + 1 + G.pad;  // the row that enters the window at the next step
    const bool more = ih + 1 < r1 && nxt % S == 0 && nxt / S < G.Ho;  // block-uniform
    if (more) fetch(nxt / S);
    if (active) {
      const int zo = ((b * G.H + ih) * G.W + iw) * G.C + c;
      const float4 zv = *reinterpret_cast<const float4*>(z + zo);
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        const int n = ih + G.pad - kh;  // block-uniform row tests
        if (n < 0 || (S == 2 && (n & 1)) || n / S >= G.Ho) continue;
        const float4* row = dws_lds + ((n / S) % RING) * ncg * QB + qi;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          // stride 2: the even taps 2j for par 0, the odd ones 2j + 1 for par 1 (none past K - 1)
          const bool dead = S == 2 && 2 * j + 1 >= K && par;
          const float4 t = row[(dead ? colb : colb - j) * QB];
          float wv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float we = wf[u * KK + kh * K + S * j];
            const float wo = (S == 2 && 2 * j + 1 < K) ? wf[u * KK + kh * K + (2 * j + 1 < K ? 2 * j + 1 : 0)] : 0.f;
            wv[u] = par ? wo : we;
          }
          acc[0] = dead ? acc[0] : fmaf(t.x, wv[0], acc[0]);
          acc[1] = dead ? acc[1] : fmaf(t.y, wv[1], acc[1]);
          acc[2] = dead ? acc[2] : fmaf(t.z, wv[2], acc[2]);
          acc[3] = dead ? acc[3] : fmaf(t.w, wv[3], acc[3]);
        }
      }
      float a[4] = {zv.x, zv.y, zv.z, zv.w}, d[4] = {1.f, 1.f, 1.f, 1.f};
      if (in_silu) {  // block-uniform
#pragma unroll
        for (int u = 0; u < 4; ++u) dws_silu_both(a[u], a[u], d[u]);
      }
      if (tay != nullptr) {
        part.x += tay_term(tay_mode, acc[0], a[0]), part.y += tay_term(tay_mode, acc[1], a[1]);
        part.z += tay_term(tay_mode, acc[2], a[2]), part.w += tay_term(tay_mode, acc[3], a[3]);
      }
      *reinterpret_cast<float4*>(dz + zo) = make_float4(acc[0] * d[0], acc[1] * d[1], acc[2] * d[2], acc[3] * d[3]);
    }
    if (more) {  // RING = rows in use + 1: the slot written is not among those being read
      commit(nxt / S);
    }
    __syncthreads();
  }
  float4 tot;
  if (tay != nullptr && dws_block_fold(red, part, QB, &tot) && qok)
    *reinterpret_cast<float4*>(tay + ((rb * G.ncb + cb) * G.B + b) * G.C + c) = tot;
}

static bool dws_all_aligned(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

static DwsGeo dws_geo(const DwsTile& t, int B, int H, int W, int C, int pad, int Ho, int Wo) {
  return DwsGeo{B, H, W, C, pad, Ho, Wo, t.tw, t.lq, t.ncb, t.bw, t.nsl, t.nrb, t.rbh};
}

// the slab of `slots` x (B, C) partials stays below 2^31 bytes
static bool dws_slab_ok(int R, int slots, int B, int C) {
  long long n = 1;
  return R >= 1 && R == slots && dw_grow(n, R) && dw_grow(n, B) && dw_grow(n, C);
}

}  // namespace tp

// Slots Rp of the forward's (Rp, B, C) pool-partial slab for an (Ho, Wo, C) OUTPUT map, and R of the
// dgrad's (R, B, C) score-partial slab for an (H, W, C) INPUT map; 0 for shapes the kernels reject
extern "C" int tp_dwconv_silu_pool_slots(int Ho, int Wo, int C) {
  tp::DwsTile t;
  return tp::dws_tile(1, Ho, Wo, C, &t) ? t.slots : 0;
}

extern "C" int tp_dwconv_silu_tay_slots(int H, int W, int C) { return tp_dwconv_silu_pool_slots(H, W, C); }

// How the launchers cut a batch of B (rows x cols x C) maps (the forward's OUTPUT map, the dgrad's INPUT
// map): out8 = {tw, lq, ncb, bw, nsl, nrb, rbh, slots} of DwsTile. Host only, for the tests, which must
// know which band a block owns; returns 1, or 0 (out8 untouched) for a shape the kernels reject.
extern "C" int tp_dwconv_silu_tile(int B, int rows, int cols, int C, int* out8) {
  tp::DwsTile t;
  if (out8 == nullptr || !tp::dws_tile(B, rows, cols, C, &t)) return 0;
  const int v[8] = {t.tw, t.lq, t.ncb, t.bw, t.nsl, t.nrb, t.rbh, t.slots};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return 1;
}

// y = silu(v), v = scale * dwconv(in_act(x)) + shift: x (B, H, W, C), w (C, 1, k, k), scale / shift (C),
// y (B, Ho, Wo, C). Optional: pre (the shape of y) <- v; apoz (B, C) += count(y > 0); pool: a zeroed
// (Rp, B, C) slab, Rp = tp_dwconv_silu_pool_slots(Ho, Wo, C), whose slots sum to the sum of y over
// the map. in_act 0 | 4, out_act 4.
extern "C" hipError_t tp_dwconv_silu_fwd(const float* x, const float* w, const float* scale, const float* shift,
                                         float* y, float* pre, float* apoz, float* pool, int Rp, int B, int H, int W,
                                         int C, int k, int s, int pad, int in_act, int out_act, hipStream_t st) {
  using namespace tp;
  int Ho, Wo;
  DwsTile t;
  if (C < 4 || C % 4 != 0 || (in_act != 0 && in_act != 4) || out_act != 4 ||
      !dw_geometry(B, H, W, C, k, s, pad, &Ho, &Wo))
    return hipErrorInvalidValue;
  if (x == nullptr || w == nullptr || scale == nullptr || shift == nullptr || y == nullptr ||
      !dws_all_aligned({x, w, scale, shift, y, pre, apoz, pool}))
    return hipErrorInvalidValue;
  if (!dws_tile(B, Ho, Wo, C, &t) || (pool != nullptr && !dws_slab_ok(Rp, t.slots, B, C))) return hipErrorInvalidValue;
  const DwsGeo G = dws_geo(t, B, H, W, C, pad, Ho, Wo);
  const unsigned blocks = (unsigned)((long long)B * t.nrb * t.ncb * t.nsl);
  const int ring = s == 1 ? k + 1 : k, ncin = (t.tw - 1) * s + k;
  const size_t lds = ((size_t)ring * ncin * (DWS_T / t.tw) + DWS_T) * sizeof(float4);
#define TP_DWS_FWD(K_, S_, ...) \
  dwconv_silu_fwd_k<K_, S_><<<blocks, DWS_T, lds, st>>>(x, w, scale, shift, y, pre, apoz, pool, G, in_act == 4)
  TP_DW_KS(TP_DWS_FWD, 0);
#undef TP_DWS_FWD
  return hipGetLastError();
}

// dz (B, H, W, C) from g (unfactored dL/dy) and v (the forward's `pre`), both (B, Ho, Wo, C), w, scale
// and the forward input z; tay (optional): a zeroed (R, B, C) slab, R = tp_dwconv_silu_tay_slots(H, W, C),
// tay_mode 0 Taylor -(dA * in_act(z)), 1 Sensitivity |dA|
extern "C" hipError_t tp_dwconv_silu_dgrad(const float* g, const float* v, const float* w, const float* scale,
                                           const float* z, float* dz, float* tay, int R, int tay_mode, int B, int H,
                                           int W, int C, int k, int s, int pad, int in_act, int out_act,
                                           hipStream_t st) {
  using namespace tp;
  int Ho, Wo;
  DwsTile t;
  if (C < 4 || C % 4 != 0 || (in_act != 0 && in_act != 4) || out_act != 4 ||
      !dw_geometry(B, H, W, C, k, s, pad, &Ho, &Wo))
    return hipErrorInvalidValue;
  if (g == nullptr || v == nullptr || w == nullptr || scale == nullptr || z == nullptr || dz == nullptr ||
      !dws_all_aligned({g, v, w, scale, z, dz, tay}))
    return hipErrorInvalidValue;
  if (!dws_tile(B, H, W, C, &t)) return hipErrorInvalidValue;
  if (tay != nullptr && (tay_mode < 0 || tay_mode > 1 || !dws_slab_ok(R, t.slots, B, C))) return hipErrorInvalidValue;
  const DwsGeo G = dws_geo(t, B, H, W, C, pad, Ho, Wo);
  const unsigned blocks = (unsigned)((long long)B * t.nrb * t.ncb * t.nsl);
  const int ring = (k - 1) / s + 2, ncg = (t.tw + k - 2) / s + 2;
  const size_t lds = ((size_t)ring * ncg * (DWS_T / t.tw) + DWS_T) * sizeof(float4);
#define TP_DWS_DG(K_, S_, ...) \
  dwconv_silu_dgrad_k<K_, S_><<<blocks, DWS_T, lds, st>>>(g, v, w, scale, z, dz, tay, G, in_act == 4, tay_mode)
  TP_DW_KS(TP_DWS_DG, 0);
#undef TP_DWS_DG
  return hipGetLastError();
}
