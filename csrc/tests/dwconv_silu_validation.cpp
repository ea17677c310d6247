// Host-side validation of the LDS-staged SiLU depthwise-conv launchers (tp_dwconv_silu_* of
// csrc/kernels/dwconv_silu.hip), built with AddressSanitizer + UBSan on the host code like
// dwconv_hs_validation.cpp. Both launchers must reject, BEFORE touching the GPU, an unsupported kernel
// size / stride / padding, activation codes other than 0 | 4 on the input and 4 on the output, a
// channel count that is no multiple of 4, an empty output, missing or misaligned operands (`pre`,
// `apoz`, `pool` and `tay` included), operands of 2^31 bytes or more, a partial slab whose slot count
// is not the helper's and a tay_mode outside 0..1. tp_dwconv_silu_tile is swept over every map of up
// to 130 x 130: the bands cover the map with no empty band, they fit the slab, the slot count is the
// formula of ops.dwconv_silu_tay_slots and the LDS of every kernel stays within the figure of the
// kernel file's header. Runs on a CPU-only machine: no kernel is launched.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned, never dereferenced
static float* const A4 = reinterpret_cast<float*>(68);

// the slab's slot count for a geometry that has an output map, 1 otherwise (any slab is rejected then)
static int out_slots(int H, int W, int C, int k, int s, int pad) {
  if (s < 1 || H + 2ll * pad < k || W + 2ll * pad < k) return 1;
  const int r = tp_dwconv_silu_pool_slots((int)((H + 2ll * pad - k) / s + 1), (int)((W + 2ll * pad - k) / s + 1), C);
  return r > 0 ? r : 1;
}

static bool fwd_rejects(int B, int H, int W, int C, int k, int s, int pad, int ia = 4, int oa = 4) {
  const int Rp = out_slots(H, W, C, k, s, pad);
  return tp_dwconv_silu_fwd(A16, A16, A16, A16, A16, nullptr, nullptr, nullptr, 0, B, H, W, C, k, s, pad, ia, oa,
                            nullptr) == hipErrorInvalidValue &&
         tp_dwconv_silu_fwd(A16, A16, A16, A16, A16, A16, A16, A16, Rp, B, H, W, C, k, s, pad, ia, oa, nullptr) ==
             hipErrorInvalidValue;
}
static bool dgrad_rejects(int B, int H, int W, int C, int k, int s, int pad, int ia = 4, int oa = 4) {
  const int r = tp_dwconv_silu_tay_slots(H, W, C), R = r > 0 ? r : 1;
  return tp_dwconv_silu_dgrad(A16, A16, A16, A16, A16, A16, nullptr, 0, 0, B, H, W, C, k, s, pad, ia, oa, nullptr) ==
             hipErrorInvalidValue &&
         tp_dwconv_silu_dgrad(A16, A16, A16, A16, A16, A16, A16, R, 1, B, H, W, C, k, s, pad, ia, oa, nullptr) ==
             hipErrorInvalidValue;
}
static bool both_reject(int B, int H, int W, int C, int k, int s, int pad, int ia = 4, int oa = 4) {
  return fwd_rejects(B, H, W, C, k, s, pad, ia, oa) && dgrad_rejects(B, H, W, C, k, s, pad, ia, oa);
}

static long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// The dynamic LDS bytes of the launchers (the `lds` of tp_dwconv_silu_fwd / _dgrad): the ring of staged
// rows of 256 / tw quads + the 256-float4 reduction buffer
static long long fwd_lds(int tw, int k, int s) {
  const int ring = s == 1 ? k + 1 : k, ncin = (tw - 1) * s + k;
  return ((long long)ring * ncin * (256 / tw) + 256) * 16;
}
static long long dgrad_lds(int tw, int k, int s) {
  const int ring = (k - 1) / s + 2, ncg = (tw + k - 2) / s + 2;
  return ((long long)ring * ncg * (256 / tw) + 256) * 16;
}

static void sweep_tiles() {
  const int Cs[4] = {4, 8, 132, 2048}, Bs[4] = {1, 2, 32, 300};
  long long worst_lds = 0;
  for (int rows = 1; rows <= 130; ++rows)
    for (int cols = 1; cols <= 130; ++cols)
      for (int C : Cs) {
        const long long finest = (rows + 2) / 4 > 1 ? (rows + 2) / 4 : 1, formula = finest * cdiv(cols, 32);
        int first[8] = {0};
        for (int B : Bs) {
          int t[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
          const bool accepted = tp_dwconv_silu_tile(B, rows, cols, C, t) == 1;
          EXPECT(accepted);
          if (!accepted) continue;
          const int tw = t[0], lq = t[1], ncb = t[2], bw = t[3], nsl = t[4], nrb = t[5], rbh = t[6], slots = t[7];
          bool ok = (tw == 8 || tw == 16 || tw == 32) && (1 << lq) * tw == 256 && bw >= 1 && bw <= tw;
          ok = ok && (tw == 8 || bw > tw / 2);  // the smallest tile that holds the band
          ok = ok && ncb >= 1 && (long long)(ncb - 1) * bw < cols && cols <= (long long)ncb * bw;
          ok = ok && rbh >= 1 && nrb >= 1 && (long long)(nrb - 1) * rbh < rows && rows <= (long long)nrb * rbh;
          ok = ok && (long long)nrb * ncb <= slots && slots == formula;
          ok = ok && slots == tp_dwconv_silu_tay_slots(rows, cols, C) && slots == tp_dwconv_silu_pool_slots(rows, cols, C);
          ok = ok && nsl == cdiv(C / 4, 256 / tw) && (long long)B * nrb * ncb * nsl < (1ll << 24);
          // only the row split depends on B, and a larger batch never splits finer
          if (B == Bs[0]) {
            for (int i = 0; i < 8; ++i) first[i] = t[i];
          } else {
            ok = ok && t[0] == first[0] && t[1] == first[1] && t[2] == first[2] && t[3] == first[3] &&
                 t[4] == first[4] && t[7] == first[7] && nrb <= first[5];
          }
          for (int k : {3, 5})
            for (int s : {1, 2}) {
              const long long f = fwd_lds(tw, k, s), d = dgrad_lds(tw, k, s);
              worst_lds = f > worst_lds ? f : worst_lds;
              worst_lds = d > worst_lds ? d : worst_lds;
              ok = ok && f <= 52736 && d <= 52736;
            }
          if (!ok) {
            std::fprintf(stderr, "tile B %d rows %d cols %d C %d: tw %d lq %d ncb %d bw %d nsl %d nrb %d rbh %d slots %d\n",
                         B, rows, cols, C, tw, lq, ncb, bw, nsl, nrb, rbh, slots);
            EXPECT(ok);
          }
        }
      }
  EXPECT(worst_lds == 52736);  // the header's figure is reached (5x5 stride 2 forward, TW = 8), not exceeded
}

int main() {
  // unsupported kernel size, stride, padding
  EXPECT(both_reject(2, 8, 8, 16, 1, 1, 0));
  EXPECT(both_reject(2, 8, 8, 16, 4, 1, 1));
  EXPECT(both_reject(2, 8, 8, 16, 7, 1, 3));
  EXPECT(both_reject(2, 8, 8, 16, 3, 0, 1));
  EXPECT(both_reject(2, 8, 8, 16, 3, 3, 1));
  EXPECT(both_reject(2, 8, 8, 16, 5, 4, 2));
  EXPECT(both_reject(2, 8, 8, 16, 3, -1, 1));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, -1));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, 3));  // pad > k - 1
  EXPECT(both_reject(2, 8, 8, 16, 5, 2, 5));
  // activation codes: 0 | 4 on the input, 4 on the output
  for (int ia : {-1, 1, 2, 3, 5, 2147483647, -2147483647 - 1}) EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, ia, 4));
  for (int oa : {-1, 0, 1, 2, 3, 5, 2147483647, -2147483647 - 1}) {
    EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, 4, oa));
    EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, 0, oa));
  }
  // channel counts that are no multiple of 4 (the engine pads)
  EXPECT(both_reject(2, 8, 8, 67, 3, 1, 1));
  EXPECT(both_reject(2, 8, 8, 18, 5, 2, 2));
  EXPECT(both_reject(2, 8, 8, 2, 3, 1, 1));
  EXPECT(both_reject(2, 8, 8, 0, 3, 1, 1));
  EXPECT(both_reject(2, 8, 8, -4, 3, 1, 1));
  // empty tensors / empty output
  EXPECT(both_reject(0, 8, 8, 16, 3, 1, 1));
  EXPECT(both_reject(-1, 8, 8, 16, 3, 1, 1));
  EXPECT(both_reject(2, 0, 8, 16, 3, 1, 1));
  EXPECT(both_reject(2, 8, -3, 16, 3, 1, 1));
  EXPECT(both_reject(2, 2, 8, 16, 3, 1, 0));  // H + 2 pad < k
  EXPECT(both_reject(2, 8, 2, 16, 5, 2, 1));  // W + 2 pad < k
  // operands of 2^31 bytes or more (and arguments whose products overflow 32 / 64 bits)
  EXPECT(both_reject(128, 256, 256, 64, 3, 1, 1));  // x: exactly 2^31 bytes
  EXPECT(both_reject(4096, 256, 256, 68, 3, 2, 1));
  EXPECT(both_reject(4096, 1, 1, 8192, 5, 1, 4));    // x 2^27 bytes, y (5 x 5 per pixel) 25 times that
  EXPECT(both_reject(1, 1, 1, 21474840, 5, 1, 2));   // x 86 MB, w (C, 1, 5, 5) 2^31 bytes and more
  EXPECT(both_reject(2147483647, 2147483647, 2147483647, 2147483644, 3, 1, 1));
  EXPECT(both_reject(1, 2147483647, 1, 4, 3, 1, 1));
  EXPECT(both_reject(1, 1, 1, 2147483644, 3, 1, 1));
  // shapes below 2^31 bytes that need 2^24 blocks or slots
  EXPECT(both_reject(1 << 24, 1, 1, 4, 3, 1, 1));
  EXPECT(both_reject(1, 1 << 26, 1, 4, 3, 1, 1));
  // missing and misaligned operands, one at a time
  float* n = nullptr;
  const int Rp = tp_dwconv_silu_pool_slots(8, 8, 16), R = tp_dwconv_silu_tay_slots(8, 8, 16);
  EXPECT(Rp == 2 && R == 2);
#define FWD(x, w, sc, sh, y, pre, ap, pool, rp) \
  tp_dwconv_silu_fwd(x, w, sc, sh, y, pre, ap, pool, rp, 2, 8, 8, 16, 3, 1, 1, 4, 4, nullptr)
  EXPECT(FWD(n, A16, A16, A16, A16, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, n, A16, A16, A16, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, n, A16, A16, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, n, A16, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, n, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, n, A16, A16, A16, Rp) == hipErrorInvalidValue);
  EXPECT(FWD(A4, A16, A16, A16, A16, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A4, A16, A16, A16, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A4, A16, A16, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A4, A16, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A4, n, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, A4, n, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, n, A4, n, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, n, n, A4, Rp) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, A16, A16, A4, Rp) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, A4, A16, A16, Rp) == hipErrorInvalidValue);
  // the pool slab: a slot count that is not the helper's
  EXPECT(FWD(A16, A16, A16, A16, A16, n, n, A16, Rp + 1) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, n, n, A16, Rp - 1) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, A16, A16, A16, 0) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, A16, A16, A16, -Rp) == hipErrorInvalidValue);
#undef FWD
  // ... of the OUTPUT map: 8 x 8 -> 4 x 4 at stride 2 has one slot, not the input map's two
  EXPECT(tp_dwconv_silu_pool_slots(4, 4, 16) == 1);
  EXPECT(tp_dwconv_silu_fwd(A16, A16, A16, A16, A16, n, n, A16, Rp, 2, 8, 8, 16, 3, 2, 1, 4, 4, nullptr) ==
         hipErrorInvalidValue);
#define DG(g, v, w, sc, z, dz, tay, r, mode) \
  tp_dwconv_silu_dgrad(g, v, w, sc, z, dz, tay, r, mode, 2, 8, 8, 16, 5, 2, 2, 4, 4, nullptr)
  EXPECT(DG(n, A16, A16, A16, A16, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, n, A16, A16, A16, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, n, A16, A16, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, n, A16, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, n, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, n, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, n, A16, R, 0) == hipErrorInvalidValue);
  EXPECT(DG(A4, A16, A16, A16, A16, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A4, A16, A16, A16, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A4, A16, A16, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A4, A16, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A4, A16, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A4, n, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A4, R, 0) == hipErrorInvalidValue);
  // the score slab: a slot count that is not the helper's, a bad mode
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R + 1, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R - 1, 1) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, 0, 0) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R, 2) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R, -1) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R, 2147483647) == hipErrorInvalidValue);
#undef DG

  // the slot helpers and the tile on rejected shapes
  int t[8] = {7, 7, 7, 7, 7, 7, 7, 7};
  EXPECT(tp_dwconv_silu_tay_slots(0, 16, 16) == 0 && tp_dwconv_silu_pool_slots(16, -4, 16) == 0);
  EXPECT(tp_dwconv_silu_tay_slots(16, 16, -8) == 0 && tp_dwconv_silu_pool_slots(16, 16, 2) == 0);
  EXPECT(tp_dwconv_silu_tay_slots(2147483647, 2147483647, 2147483644) == 0);  // no overflow, out of range
  EXPECT(tp_dwconv_silu_tay_slots(1 << 20, 4, 4) == (1 << 18));
  EXPECT(tp_dwconv_silu_tay_slots(1 << 26, 1, 4) == 0 && tp_dwconv_silu_tay_slots((1 << 26) - 3, 1, 4) == (1 << 24) - 1);
  EXPECT(tp_dwconv_silu_tile(0, 8, 8, 16, t) == 0 && tp_dwconv_silu_tile(1, 0, 8, 16, t) == 0);
  EXPECT(tp_dwconv_silu_tile(1, 8, -1, 16, t) == 0 && tp_dwconv_silu_tile(1, 8, 8, 6, t) == 0);
  EXPECT(tp_dwconv_silu_tile(1, 8, 8, 0, t) == 0 && tp_dwconv_silu_tile(1, 1 << 26, 1, 4, t) == 0);
  EXPECT(tp_dwconv_silu_tile(1 << 24, 1, 1, 4, t) == 0);
  EXPECT(tp_dwconv_silu_tile(2147483647, 2147483647, 2147483647, 2147483644, t) == 0);
  for (int i = 0; i < 8; ++i) EXPECT(t[i] == 7);  // a rejected shape writes nothing
  EXPECT(tp_dwconv_silu_tile(1, 8, 8, 16, nullptr) == 0);
  // EfficientNet-B0's first layer as the kernel file's header has it: 28 x 4 bands at B = 1, 8 x 4 at 32
  EXPECT(tp_dwconv_silu_tile(1, 112, 112, 32, t) == 1 && t[0] == 32 && t[2] == 4 && t[3] == 28 && t[5] == 28 &&
         t[6] == 4 && t[7] == 112);
  EXPECT(tp_dwconv_silu_tile(32, 112, 112, 32, t) == 1 && t[2] == 4 && t[5] == 8 && t[6] == 14 && t[7] == 112);
  sweep_tiles();

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("dwconv_silu validation ok\n");
  return 0;
}
