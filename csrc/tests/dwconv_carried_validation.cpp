// Host-side validation of the carried-width depthwise-conv launchers (tp_dwconv_* at Cw < C,
// csrc/kernels/dwconv.hip) and of the BatchNorm launchers' activation code (batchnorm.hip), built
// with AddressSanitizer + UBSan on the host code like dwconv_validation.cpp. A carried width has
// the activations at C channels per pixel and the parameter at Cw <= C; the launchers must reject,
// BEFORE touching the GPU, Cw <= 0, Cw > C, Cw < C at a C that is no multiple of 4, misaligned
// pointers, and the grid and 2 GiB limits of the plain launchers; the BatchNorm forward launchers
// an activation code outside 0..2 and a ReLU6 forward without a mask to write. Runs on a CPU-only
// machine: no kernel is launched (every call here is one that must be rejected).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "tp_expect.h"
#include "tp_launchers.h"

// the three launchers on one geometry (null operands: never touched when the call is rejected)
static bool all_reject(int B, int H, int W, int C, int Cw, int k, int s, int pad) {
  float* n = nullptr;
  double* ws = reinterpret_cast<double*>(16);
  float* dw = reinterpret_cast<float*>(16);
  const int P = B > 0 && H > 0 && W > 0 ? 1 : 0;  // (any chunk count: the width is checked first)
  const bool f = tp_dwconv_fwd(n, n, n, n, B, H, W, C, Cw, k, s, pad, nullptr) == hipErrorInvalidValue;
  const bool d = tp_dwconv_dgrad(n, n, n, B, H, W, C, Cw, k, s, pad, nullptr) == hipErrorInvalidValue;
  const bool g = tp_dwconv_wgrad(n, n, dw, n, ws, tp_dwconv_wgrad_chunks(P, C), B, H, W, C, Cw, k, s, pad,
                                 (long long)k * k, k, 1, nullptr) == hipErrorInvalidValue;
  return f && d && g;
}

int main() {
  // the parameter's width: positive, at most the carried width, and a carried width is a multiple of 4
  EXPECT(all_reject(2, 8, 8, 16, 0, 3, 1, 1));
  EXPECT(all_reject(2, 8, 8, 16, -4, 3, 1, 1));
  EXPECT(all_reject(2, 8, 8, 16, 17, 3, 1, 1));
  EXPECT(all_reject(2, 8, 8, 16, 2147483647, 5, 2, 2));
  EXPECT(all_reject(2, 8, 8, 15, 13, 3, 1, 1));  // Cw < C, C % 4 != 0
  EXPECT(all_reject(2, 8, 8, 67, 66, 5, 1, 2));
  EXPECT(all_reject(2, 8, 8, 6, 4, 3, 2, 1));
  // the plain launchers' geometry rules hold at a carried width
  EXPECT(all_reject(2, 8, 8, 16, 13, 4, 1, 1));
  EXPECT(all_reject(2, 8, 8, 16, 13, 3, 3, 1));
  EXPECT(all_reject(2, 8, 8, 16, 13, 3, 1, 3));
  EXPECT(all_reject(0, 8, 8, 16, 13, 3, 1, 1));
  EXPECT(all_reject(2, 2, 8, 16, 13, 3, 1, 0));
  // operands of 2^31 bytes or more are sized by the carried width
  EXPECT(all_reject(128, 256, 256, 64, 61, 3, 1, 1));  // exactly 2^31 bytes
  EXPECT(all_reject(4096, 256, 256, 68, 67, 3, 2, 1));
  EXPECT(all_reject(2147483647, 2147483647, 2147483647, 2147483644, 5, 3, 1, 1));
  // more 256-thread blocks than a grid takes: millions of rows (forward / dgrad), millions of channels (the fold)
  float* n = nullptr;
  EXPECT(tp_dwconv_fwd(n, n, n, n, 1 << 12, 1 << 13, 1, 4, 1, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_dgrad(n, n, n, 1 << 12, 1 << 13, 1, 4, 3, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(n, n, reinterpret_cast<float*>(16), n, reinterpret_cast<double*>(16),
                         tp_dwconv_wgrad_chunks(1, 1 << 25), 1, 1, 1, 1 << 25, 5, 3, 1, 1, 9, 3, 1, nullptr) ==
         hipErrorInvalidValue);
  // misaligned pointers: a carried width always runs float4 accesses (16-byte alignment)
  const float* a4 = reinterpret_cast<const float*>(4);
  float* a16 = reinterpret_cast<float*>(16);
  double* ws = reinterpret_cast<double*>(16);
  EXPECT(tp_dwconv_fwd(a4, a16, n, a16, 2, 8, 8, 16, 13, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_fwd(a16, a4, n, a16, 2, 8, 8, 16, 13, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_fwd(a16, a16, a4, a16, 2, 8, 8, 16, 13, 3, 1, 1, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_fwd(a16, a16, n, const_cast<float*>(a4), 2, 8, 8, 16, 13, 3, 1, 1, nullptr) ==
         hipErrorInvalidValue);
  EXPECT(tp_dwconv_dgrad(a4, a16, a16, 2, 8, 8, 16, 13, 5, 2, 2, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_dgrad(a16, a4, a16, 2, 8, 8, 16, 13, 5, 2, 2, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_dgrad(a16, a16, const_cast<float*>(a4), 2, 8, 8, 16, 13, 5, 2, 2, nullptr) ==
         hipErrorInvalidValue);
  const int ch = tp_dwconv_wgrad_chunks(2 * 8 * 8, 16);
  EXPECT(tp_dwconv_wgrad(a4, a16, a16, n, ws, ch, 2, 8, 8, 16, 13, 3, 1, 1, 9, 3, 1, nullptr) ==
         hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a4, a16, n, ws, ch, 2, 8, 8, 16, 13, 3, 1, 1, 9, 3, 1, nullptr) ==
         hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, reinterpret_cast<double*>(72), ch, 2, 8, 8, 16, 13, 3, 1, 1, 9, 3, 1,
                         nullptr) == hipErrorInvalidValue);
  EXPECT(tp_dwconv_wgrad(a16, a16, n, n, ws, ch, 2, 8, 8, 16, 13, 3, 1, 1, 9, 3, 1, nullptr) ==
         hipErrorInvalidValue);  // no dw
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, ws, ch + 1, 2, 8, 8, 16, 13, 3, 1, 1, 9, 3, 1, nullptr) ==
         hipErrorInvalidValue);  // the workspace is sized by the carried width's chunk count
  EXPECT(tp_dwconv_wgrad(a16, a16, a16, n, ws, ch, 2, 8, 8, 16, 13, 3, 1, 1, 1ll << 40, 3, 1, nullptr) ==
         hipErrorInvalidValue);  // a dW stride past the 32-bit range

  // BatchNorm forward: activation codes 0 (none), 1 (ReLU), 2 (ReLU6, with a mask to write) only
  uint8_t* mk = reinterpret_cast<uint8_t*>(16);
  for (int bad : {-1, 3, 4, 256, -2147483647 - 1, 2147483647}) {
    EXPECT(tp_bn_fwd_train(n, n, 64, 8, 8, n, n, 1e-5f, 0.1f, n, n, n, n, n, n, nullptr, n, bad, mk, nullptr,
                           nullptr) == hipErrorInvalidValue);
    EXPECT(tp_bn_fwd_train_pre(n, n, 64, 8, 8, n, n, 1e-5f, 0.1f, n, n, n, n, n, n, nullptr, nullptr, 1, n, bad, mk,
                               nullptr, nullptr) == hipErrorInvalidValue);
    EXPECT(tp_bn_fwd_train(n, n, 64, 8, 8, n, n, 1e-5f, 0.1f, n, n, n, n, n, n, nullptr, n, bad, nullptr, nullptr,
                           nullptr) == hipErrorInvalidValue);
  }
  EXPECT(tp_bn_fwd_train(n, n, 64, 8, 8, n, n, 1e-5f, 0.1f, n, n, n, n, n, n, nullptr, n, 2, nullptr, nullptr,
                         nullptr) == hipErrorInvalidValue);  // ReLU6 without a mask
  EXPECT(tp_bn_fwd_train_pre(n, n, 64, 8, 8, n, n, 1e-5f, 0.1f, n, n, n, n, n, n, nullptr, nullptr, 1, n, 2, nullptr,
                             nullptr, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_bn_fwd_train(n, n, 64, 8, 8, n, n, 1e-5f, 0.1f, n, n, n, n, n, n, nullptr, n, 2, nullptr, nullptr,
                         nullptr) == hipErrorInvalidValue);  // (the mask-free entry points cannot run ReLU6)

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("dwconv carried validation ok\n");
  return 0;
}
