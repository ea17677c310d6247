// Host-side validation of the Hardswish-aware depthwise-conv launchers (tp_dwconv_hs_* of
// csrc/kernels/dwconv_act.hip), built with AddressSanitizer + UBSan on the host code like
// dwconv_act_validation.cpp. Both launchers must reject, BEFORE touching the GPU, an unsupported
// kernel size / stride / padding, an activation code outside 0..3, a channel count that is no
// multiple of 4, an empty output, missing or misaligned operands (`pre` included), a missing y when
// out_act != 0, operands of 2^31 bytes or more and a partial slab whose slot count is not the
// helper's; the tp_dwconv_act_* entry points must keep rejecting code 3; the slot helper must agree
// with tp_dwconv_act_tay_slots. Runs on a CPU-only machine: no kernel is launched.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned, never dereferenced
static float* const A4 = reinterpret_cast<float*>(68);

static bool fwd_rejects(int B, int H, int W, int C, int k, int s, int pad, int ia = 3, int oa = 3) {
  return tp_dwconv_hs_fwd(A16, A16, A16, A16, A16, A16, A16, B, H, W, C, k, s, pad, ia, oa, nullptr) ==
             hipErrorInvalidValue &&
         tp_dwconv_hs_fwd(A16, A16, A16, A16, A16, nullptr, nullptr, B, H, W, C, k, s, pad, ia, oa, nullptr) ==
             hipErrorInvalidValue;
}
static bool dgrad_rejects(int B, int H, int W, int C, int k, int s, int pad, int ia = 3, int oa = 3) {
  const int R = tp_dwconv_hs_tay_slots(H, W, C);
  return tp_dwconv_hs_dgrad(A16, A16, A16, A16, A16, A16, nullptr, 0, 0, B, H, W, C, k, s, pad, ia, oa, nullptr) ==
             hipErrorInvalidValue &&
         tp_dwconv_hs_dgrad(A16, A16, A16, A16, A16, A16, A16, R, 0, B, H, W, C, k, s, pad, ia, oa, nullptr) ==
             hipErrorInvalidValue;
}
static bool both_reject(int B, int H, int W, int C, int k, int s, int pad, int ia = 3, int oa = 3) {
  return fwd_rejects(B, H, W, C, k, s, pad, ia, oa) && dgrad_rejects(B, H, W, C, k, s, pad, ia, oa);
}

int main() {
  // unsupported kernel size, stride, padding
  EXPECT(both_reject(2, 8, 8, 16, 1, 1, 0));
  EXPECT(both_reject(2, 8, 8, 16, 4, 1, 1));
  EXPECT(both_reject(2, 8, 8, 16, 7, 1, 3));
  EXPECT(both_reject(2, 8, 8, 16, 3, 0, 1));
  EXPECT(both_reject(2, 8, 8, 16, 3, 3, 1));
  EXPECT(both_reject(2, 8, 8, 16, 5, 4, 2));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, -1));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, 3));  // pad > k - 1
  EXPECT(both_reject(2, 8, 8, 16, 5, 2, 5));
  // activation codes outside 0..3
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, 4, 3));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, 3, 4));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, 3, -1));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, -1, 1));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, 2147483647, 0));
  EXPECT(both_reject(2, 8, 8, 16, 3, 1, 1, 0, -2147483647 - 1));
  // ... and the ReLU6-only entry points keep rejecting code 3
  EXPECT(tp_dwconv_act_fwd(A16, A16, A16, A16, A16, A16, 2, 8, 8, 16, 3, 1, 1, 3, 2, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_act_fwd(A16, A16, A16, A16, A16, A16, 2, 8, 8, 16, 3, 1, 1, 0, 3, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_act_dgrad(A16, A16, A16, A16, A16, A16, nullptr, 0, 0, 2, 8, 8, 16, 3, 1, 1, 3, 3, nullptr) ==
         hipErrorInvalidValue);
  // channel counts that are no multiple of 4 (the engine pads)
  EXPECT(both_reject(2, 8, 8, 67, 3, 1, 1));
  EXPECT(both_reject(2, 8, 8, 2, 3, 1, 1));
  EXPECT(both_reject(2, 8, 8, 0, 3, 1, 1));
  EXPECT(both_reject(2, 8, 8, -4, 3, 1, 1));
  // empty tensors / empty output
  EXPECT(both_reject(0, 8, 8, 16, 3, 1, 1));
  EXPECT(both_reject(2, 0, 8, 16, 3, 1, 1));
  EXPECT(both_reject(2, 8, -3, 16, 3, 1, 1));
  EXPECT(both_reject(2, 2, 8, 16, 3, 1, 0));  // H + 2 pad < k
  EXPECT(both_reject(2, 8, 2, 16, 5, 2, 1));  // W + 2 pad < k
  // operands of 2^31 bytes or more (and arguments whose products overflow 32 / 64 bits)
  EXPECT(both_reject(128, 256, 256, 64, 3, 1, 1));  // exactly 2^31 bytes
  EXPECT(both_reject(4096, 256, 256, 68, 3, 2, 1));
  EXPECT(both_reject(2147483647, 2147483647, 2147483647, 2147483644, 3, 1, 1));
  EXPECT(both_reject(1, 2147483647, 1, 4, 3, 1, 1));
  EXPECT(both_reject(1, 1, 1, 2147483644, 3, 1, 1));
  // shapes below 2^31 bytes that would need more 256-thread blocks than a grid takes
  EXPECT(both_reject(1 << 12, 1 << 13, 1, 4, 3, 1, 1));
  // missing and misaligned operands, one at a time
  float* n = nullptr;
#define FWD(x, w, sc, sh, y, ap, pre) tp_dwconv_hs_fwd(x, w, sc, sh, y, ap, pre, 2, 8, 8, 16, 3, 1, 1, 3, 3, nullptr)
  EXPECT(FWD(n, A16, A16, A16, A16, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, n, A16, A16, A16, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, n, A16, A16, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, n, A16, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, n, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, n, A16, A16) == hipErrorInvalidValue);
  EXPECT(FWD(A4, A16, A16, A16, A16, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A4, A16, A16, A16, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A4, A16, A16, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A4, A16, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A4, n, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, A4, n) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, n, A4) == hipErrorInvalidValue);
  EXPECT(FWD(A16, A16, A16, A16, A16, A16, A4) == hipErrorInvalidValue);
#undef FWD
  const int R = tp_dwconv_hs_tay_slots(8, 8, 16);
  EXPECT(R == 8);
#define DG(g, y, w, sc, z, dz, tay, r, mode, oa) \
  tp_dwconv_hs_dgrad(g, y, w, sc, z, dz, tay, r, mode, 2, 8, 8, 16, 5, 2, 2, 3, oa, nullptr)
  EXPECT(DG(n, A16, A16, A16, A16, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, n, A16, A16, A16, A16, n, 0, 0, 3) == hipErrorInvalidValue);  // y (pre) is read when out_act != 0
  EXPECT(DG(A16, n, A16, A16, A16, A16, n, 0, 0, 2) == hipErrorInvalidValue);
  EXPECT(DG(A16, n, A16, A16, A16, A16, n, 0, 0, 1) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, n, A16, A16, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, n, A16, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, n, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, n, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A4, A16, A16, A16, A16, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A4, A16, A16, A16, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A4, A16, A16, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A4, A16, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A4, A16, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A4, n, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A4, R, 0, 3) == hipErrorInvalidValue);
  // the partial slab: a slot count that is not the helper's, a bad mode
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R + 1, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R - 1, 1, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, 0, 0, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R, 2, 3) == hipErrorInvalidValue);
  EXPECT(DG(A16, A16, A16, A16, A16, A16, A16, R, -1, 3) == hipErrorInvalidValue);
#undef DG
  // a slab of 2^31 bytes or more although z is below it (the case of dwconv_act_validation.cpp)
  {
    const int H = 8192, W = 4, C = 16380, B = 1;
    const int r = tp_dwconv_hs_tay_slots(H, W, C);
    EXPECT(r == H * 16);
    EXPECT((long long)B * H * W * C * 4 < (1ll << 31) && (long long)r * B * C * 4 >= (1ll << 31));
    EXPECT(tp_dwconv_hs_dgrad(A16, A16, A16, A16, A16, A16, A16, r, 0, B, H, W, C, 3, 1, 1, 3, 3, nullptr) ==
           hipErrorInvalidValue);
  }

  // the slot helper is the ReLU6 one's: same slabs, same arena
  for (int h = 1; h <= 300; h = h < 20 ? h + 1 : h + h / 5)
    for (int w = 1; w <= 300; w = w < 40 ? w + 1 : w + w / 6)
      for (int c = 1; c <= 4096; c = c < 70 ? c + 1 : c + c / 9 + 1)
        EXPECT(tp_dwconv_hs_tay_slots(h, w, c) == tp_dwconv_act_tay_slots(h, w, c));
  EXPECT(tp_dwconv_hs_tay_slots(0, 16, 16) == 0 && tp_dwconv_hs_tay_slots(16, -4, 16) == 0);
  EXPECT(tp_dwconv_hs_tay_slots(16, 16, -8) == 0 && tp_dwconv_hs_tay_slots(16, 16, 2) == 0);
  EXPECT(tp_dwconv_hs_tay_slots(2147483647, 2147483647, 2147483644) == 0);  // no overflow, out of range
  EXPECT(tp_dwconv_hs_tay_slots(1 << 20, 4, 4) == (1 << 20));

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("dwconv_hs validation ok\n");
  return 0;
}
