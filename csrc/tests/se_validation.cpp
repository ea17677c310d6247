// Host-side validation of the squeeze-and-excitation launchers (csrc/kernels/squeeze_excite.hip),
// built with AddressSanitizer + UBSan on the host code like dwconv_validation.cpp. Every launcher
// must reject, BEFORE touching the GPU, null pointers, non-positive sizes, pointers that are not
// 16-byte aligned on the float4 path, operands of 2^31 bytes or more and grids past the launch
// limits; the split helper must stay in range over every (B, HW, C). Runs on a CPU-only machine:
// no kernel is launched.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned stand-ins: never dereferenced
static float* const A4 = reinterpret_cast<float*>(68);   // 4-byte aligned only
static float* const A1 = reinterpret_cast<float*>(66);   // not even a float's alignment
static const hipError_t BAD = hipErrorInvalidValue;

// the four activation launchers on one shape, every pointer valid: rejected for the shape alone
static bool act_reject(int B, int HW, int C) {
  const int sp = tp_se_splits(B, HW, C);
  return tp_se_pool(A16, A16, A16, sp, B, HW, C, nullptr) == BAD &&
         tp_se_bwd_reduce(A16, A16, A16, A16, sp, B, HW, C, nullptr) == BAD &&
         tp_se_scale(A16, A16, A16, B, HW, C, nullptr) == BAD &&
         tp_se_bwd_dx(A16, A16, A16, A16, B, HW, C, nullptr) == BAD;
}

// the two FC launchers on one shape, every pointer valid
static bool fc_reject(int B, int C, int Cs, int gate) {
  return tp_se_gate_fwd(A16, A16, A16, A16, A16, A16, A16, B, C, Cs, gate, nullptr) == BAD &&
         tp_se_gate_bwd(A16, A16, A16, A16, A16, A16, A16, A16, B, C, Cs, gate, nullptr) == BAD;
}

int main() {
  float* n = nullptr;
  // non-positive sizes
  EXPECT(act_reject(0, 49, 16));
  EXPECT(act_reject(2, 0, 16));
  EXPECT(act_reject(2, 49, 0));
  EXPECT(act_reject(-1, 49, 16));
  EXPECT(act_reject(2, -49, 16));
  EXPECT(act_reject(2, 49, -16));
  EXPECT(fc_reject(0, 16, 8, 0));
  EXPECT(fc_reject(2, 0, 8, 0));
  EXPECT(fc_reject(2, 16, 0, 0));
  EXPECT(fc_reject(2, 16, -8, 1));
  EXPECT(fc_reject(2, 16, 8, 2));   // no such gate
  EXPECT(fc_reject(2, 16, 8, -1));
  // operands of 2^31 bytes or more (and arguments whose products overflow 32 / 64 bits)
  EXPECT(act_reject(128, 256 * 256, 64));  // exactly 2^31 bytes
  EXPECT(act_reject(4096, 256 * 256, 67));
  EXPECT(act_reject(2147483647, 2147483647, 2147483647));
  EXPECT(act_reject(1, 2147483647, 1));
  EXPECT(act_reject(1, 1, 2147483647));
  EXPECT(fc_reject(2147483647, 2147483647, 2147483647, 0));
  EXPECT(fc_reject(1 << 20, 1 << 10, 8, 0));  // (B, C) rows of 2^32 bytes
  // grids past the launch limits: more images than a grid dimension takes, rows that do not fit
  // the LDS of the FC kernels
  EXPECT(act_reject(65536, 1, 4));
  EXPECT(act_reject(1 << 20, 1, 1));
  EXPECT(fc_reject(2, 12288, 1, 0));
  EXPECT(fc_reject(2, 8192, 4097, 1));
  EXPECT(fc_reject(1 << 24, 4, 4, 0));
  // null pointers, one operand at a time (128 images of 960 channels: one split, no workspace)
  EXPECT(tp_se_splits(128, 49, 960) == 1 && tp_se_splits(128, 49, 963) == 1);
  EXPECT(tp_se_pool(n, A16, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_pool(A16, n, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_bwd_reduce(n, A16, A16, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_bwd_reduce(A16, n, A16, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_bwd_reduce(A16, A16, n, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_scale(n, A16, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_scale(A16, n, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_scale(A16, A16, n, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_bwd_dx(n, A16, A16, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_bwd_dx(A16, n, A16, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_bwd_dx(A16, A16, n, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_bwd_dx(A16, A16, A16, n, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_gate_fwd(n, A16, n, A16, n, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_fwd(A16, n, n, A16, n, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_fwd(A16, A16, n, n, n, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_fwd(A16, A16, n, A16, n, n, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_fwd(A16, A16, n, A16, n, A16, n, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(n, A16, A16, A16, A16, A16, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(A16, n, A16, A16, A16, A16, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(A16, A16, n, A16, A16, A16, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(A16, A16, A16, n, A16, A16, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(A16, A16, A16, A16, n, A16, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(A16, A16, A16, A16, A16, n, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(A16, A16, A16, A16, A16, A16, n, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(A16, A16, A16, A16, A16, A16, A16, n, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_wgrad(n, A16, A16, n, 4, 16, 8, 8, 1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, n, A16, n, 4, 16, 8, 8, 1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, A16, n, n, 4, 16, 8, 8, 1, nullptr) == BAD);
  // misaligned pointers on the float4 path (C % 4 == 0), one operand at a time; 4-byte alignment
  // everywhere else
  EXPECT(tp_se_pool(A4, A16, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_pool(A16, A4, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_pool(A1, A16, n, 1, 128, 49, 963, nullptr) == BAD);
  EXPECT(tp_se_bwd_reduce(A4, A16, A16, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_bwd_reduce(A16, A4, A16, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_bwd_reduce(A16, A16, A4, n, 1, 128, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_scale(A4, A16, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_scale(A16, A4, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_scale(A16, A16, A4, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_scale(A16, A16, A1, 2, 49, 13, nullptr) == BAD);
  EXPECT(tp_se_bwd_dx(A4, A16, A16, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_bwd_dx(A16, A4, A16, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_bwd_dx(A16, A16, A4, A16, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_bwd_dx(A16, A16, A16, A4, 2, 49, 16, nullptr) == BAD);
  EXPECT(tp_se_gate_fwd(A1, A16, n, A16, n, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_fwd(A16, A16, A1, A16, n, A16, A16, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_gate_bwd(A16, A16, A16, A16, A16, A16, A16, A1, 2, 16, 8, 0, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A1, A16, A16, n, 4, 16, 8, 8, 1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, A16, A16, A1, 4, 16, 8, 8, 1, nullptr) == BAD);
  // reduce: a split count that is not the helper's, a missing workspace when the pixels are split
  EXPECT(tp_se_splits(1, 56 * 56, 16) > 1);
  EXPECT(tp_se_pool(A16, A16, A16, tp_se_splits(2, 49, 960) + 1, 2, 49, 960, nullptr) == BAD);
  EXPECT(tp_se_pool(A16, A16, n, tp_se_splits(1, 56 * 56, 16), 1, 56 * 56, 16, nullptr) == BAD);
  EXPECT(tp_se_bwd_reduce(A16, A16, A16, A4, tp_se_splits(1, 56 * 56, 16), 1, 56 * 56, 16, nullptr) == BAD);
  // wgrad: bad sizes and strides
  EXPECT(tp_se_wgrad(A16, A16, A16, n, 0, 16, 8, 8, 1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, A16, A16, n, 4, 0, 8, 8, 1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, A16, A16, n, 4, 16, -8, 8, 1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, A16, A16, n, 4, 16, 8, 0, 1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, A16, A16, n, 4, 16, 8, 8, -1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, A16, A16, n, 4, 16, 8, 1ll << 40, 1, nullptr) == BAD);
  EXPECT(tp_se_wgrad(A16, A16, A16, n, 4, 1 << 15, 1 << 15, 1 << 15, 1, nullptr) == BAD);  // dW of 2^32 bytes
  EXPECT(tp_se_wgrad(A16, A16, A16, n, 2147483647, 2147483647, 2147483647, 1, 1, nullptr) == BAD);

  // splits: at least one, at most 64, none empty, the workspace below 2^31 bytes
  for (int b = 1; b <= 4096; b = b < 8 ? b + 1 : b * 2)
    for (int hw = 1; hw <= (1 << 16); hw = hw < 64 ? hw + 1 : hw + hw / 7 + 1)
      for (int c = 1; c <= 4096; c = c < 70 ? c + 1 : c + c / 9 + 1) {
        const int sp = tp_se_splits(b, hw, c);
        EXPECT(sp >= 1 && sp <= 64 && sp <= hw);
        const int ppc = (hw + sp - 1) / sp;
        EXPECT((long long)(sp - 1) * ppc < hw);
        EXPECT((long long)sp * b * c * 4 < (1ll << 31));
      }
  EXPECT(tp_se_splits(0, 49, 16) == 1 && tp_se_splits(2, -4, 16) == 1 && tp_se_splits(2, 49, 0) == 1);
  EXPECT(tp_se_splits(2147483647, 2147483647, 2147483647) >= 1);

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("se validation ok\n");
  return 0;
}
