// Host-side validation of the depthwise-conv launchers (csrc/kernels/dwconv.hip), built with
// AddressSanitizer + UBSan on the host code like launcher_validation.cpp. Every launcher must
// reject, BEFORE touching the GPU, an unsupported kernel size / stride / padding, an empty output,
// pointers that are not 16-byte aligned on the float4 path and operands of 2^31 bytes or more; the
// workspace-size helper must stay in range over every (P, C). Runs on a CPU-only machine: no
// kernel is launched.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

// the three launchers on one geometry (null operands: never touched when the call is rejected)
static bool all_reject(int B, int H, int W, int C, int k, int s, int pad) {
  float* n = nullptr;
  double* ws = reinterpret_cast<double*>(16);
  float* dw = reinterpret_cast<float*>(16);
  const bool f = tp_dwconv_fwd(n, n, n, n, B, H, W, C, C, k, s, pad, nullptr) == hipErrorInvalidValue;
  const bool d = tp_dwconv_dgrad(n, n, n, B, H, W, C, C, k, s, pad, nullptr) == hipErrorInvalidValue;
  const bool g = tp_dwconv_wgrad(n, n, dw, n, ws, 1, B, H, W, C, C, k, s, pad, (long long)k * k, k, 1, nullptr) ==
                 hipErrorInvalidValue;
  return f && d && g;
}

int main() {
  // unsupported kernel size, stride, padding
  EXPECT(all_reject(2, 8, 8, 16, 1, 1, 0));
  EXPECT(all_reject(2, 8, 8, 16, 4, 1, 1));
  EXPECT(all_reject(2, 8, 8, 16, 7, 1, 3));
  EXPECT(all_reject(2, 8, 8, 16, 3, 0, 1));
  EXPECT(all_reject(2, 8, 8, 16, 3, 3, 1));
  EXPECT(all_reject(2, 8, 8, 16, 5, 4, 2));
  EXPECT(all_reject(2, 8, 8, 16, 3, 1, -1));
  EXPECT(all_reject(2, 8, 8, 16, 3, 1, 3));  // pad > k - 1
  EXPECT(all_reject(2, 8, 8, 16, 5, 2, 5));
  // empty tensors / empty output
  EXPECT(all_reject(0, 8, 8, 16, 3, 1, 1));
  EXPECT(all_reject(2, 0, 8, 16, 3, 1, 1));
  EXPECT(all_reject(2, 8, 8, 0, 3, 1, 1));
  EXPECT(all_reject(2, 8, -3, 16, 3, 1, 1));
  EXPECT(all_reject(2, 2, 8, 16, 3, 1, 0));   // H + 2 pad < k
  EXPECT(all_reject(2, 8, 2, 16, 5, 2, 1));   // W + 2 pad < k
  EXPECT(all_reject(1, 1, 1, 67, 5, 1, 1));
  // operands of 2^31 bytes or more (and arguments whose products overflow 32 / 64 bits)
  EXPECT(all_reject(128, 256, 256, 64, 3, 1, 1));               // exactly 2^31 bytes
  EXPECT(all_reject(4096, 256, 256, 67, 3, 2, 1));
  EXPECT(all_reject(2147483647, 2147483647, 2147483647, 2147483647, 3, 1, 1));
  EXPECT(all_reject(1, 2147483647, 1, 1, 3, 1, 1));
  EXPECT(all_reject(1, 1, 1, 2147483647, 3, 1, 1));
  // shapes that fit in 2^31 bytes but would need more 256-thread blocks than a grid takes (2^32
  // threads): millions of rows of one element (forward / dgrad), millions of channels (the fold)
  float* n = nullptr;
  EXPECT(tp_dwconv_fwd(n, n, n, n, 1 << 12, 1 << 13, 1, 1, 1, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_dgrad(n, n, n, 1 << 12, 1 << 13, 1, 1, 1, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(n, n, reinterpret_cast<float*>(16), n, reinterpret_cast<double*>(16),
                         tp_dwconv_wgrad_chunks(1, 1 << 25), 1, 1, 1, 1 << 25, 1 << 25, 3, 1, 1, 9, 3, 1, nullptr) ==
         hipErrorInvalidValue);
  // misaligned pointers on the float4 path (C % 4 == 0), one operand at a time
  float* a16 = reinterpret_cast<float*>(64);
  float* a4 = reinterpret_cast<float*>(68);
  double* ws = reinterpret_cast<double*>(64);
  EXPECT(tp_dwconv_fwd(a4, a16, n, a16, 2, 8, 8, 16, 16, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_fwd(a16, a4, n, a16, 2, 8, 8, 16, 16, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_fwd(a16, a16, a4, a16, 2, 8, 8, 16, 16, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_fwd(a16, a16, n, a4, 2, 8, 8, 16, 16, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_dgrad(a4, a16, a16, 2, 8, 8, 16, 16, 5, 2, 2, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_dgrad(a16, a4, a16, 2, 8, 8, 16, 16, 5, 2, 2, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_dgrad(a16, a16, a4, 2, 8, 8, 16, 16, 5, 2, 2, nullptr) == hipErrorInvalidValue);
  const int ch = tp_dwconv_wgrad_chunks(2 * 8 * 8, 16);
  EXPECT(tp_dwconv_wgrad(a4, a16, a16, n, ws, ch, 2, 8, 8, 16, 16, 3, 1, 1, 9, 3, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a4, a16, n, ws, ch, 2, 8, 8, 16, 16, 3, 1, 1, 9, 3, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, reinterpret_cast<double*>(72), ch, 2, 8, 8, 16, 16, 3, 1, 1, 9, 3, 1,
                         nullptr) == hipErrorInvalidValue);
  // wgrad: missing outputs / workspace, a chunk count that is not the helper's, bad dW strides
  EXPECT(tp_dwconv_wgrad(a16, a16, n, n, ws, ch, 2, 8, 8, 16, 16, 3, 1, 1, 9, 3, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, nullptr, ch, 2, 8, 8, 16, 16, 3, 1, 1, 9, 3, 1, nullptr) ==
         hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, ws, ch + 1, 2, 8, 8, 16, 16, 3, 1, 1, 9, 3, 1, nullptr) ==
         hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, ws, ch, 2, 8, 8, 16, 16, 3, 1, 1, 0, 3, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, ws, ch, 2, 8, 8, 16, 16, 3, 1, 1, 9, -3, 1, nullptr) ==
         hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, ws, ch, 2, 8, 8, 16, 16, 3, 1, 1, 1ll << 40, 3, 1, nullptr) ==
         hipErrorInvalidValue);

  // workspace chunks: at least one, never more than the pixels allow, the workspace below 2^31 bytes
  for (int p = 1; p <= (1 << 20); p = p < 64 ? p + 1 : p + p / 7 + 1)
    for (int c = 1; c <= 2048; c = c < 70 ? c + 1 : c + c / 9 + 1) {
      const int n_ch = tp_dwconv_wgrad_chunks(p, c);
      EXPECT(n_ch >= 1 && n_ch <= 1024 && (n_ch == 1 || (long long)n_ch * 256 <= p));
      EXPECT((long long)n_ch * 26 * c * 8 < (1ll << 31));
    }
  EXPECT(tp_dwconv_wgrad_chunks(1 << 20, 2048) >= 1 && tp_dwconv_wgrad_chunks(1 << 20, 1) == 1024);
  EXPECT(tp_dwconv_wgrad_chunks(0, 16) == 1 && tp_dwconv_wgrad_chunks(16, -4) == 1);
  EXPECT(tp_dwconv_wgrad_chunks(2147483647, 2147483647) >= 1);

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("dwconv validation ok\n");
  return 0;
}
