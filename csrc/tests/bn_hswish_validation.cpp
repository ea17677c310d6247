// Host-side validation of the fused BatchNorm + Hardswish launchers (tp_bn_hswish_fwd_train /
// tp_bn_hswish_bwd_train, csrc/kernels/batchnorm.hip), built with AddressSanitizer + UBSan on the host
// code like se_validation.cpp. Both must reject, BEFORE touching any pointer, non-positive C / P / Cr,
// Cr > C and activations of 2^32 elements or more; the backward also a missing af / bf (the forward's
// folded affine rows, which it recomputes the pre-activation from). Runs on a CPU-only machine: no
// kernel is launched (every call here is one that must be rejected).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned stand-in: never dereferenced
static double* const W16 = reinterpret_cast<double*>(64);
static const hipError_t BAD = hipErrorInvalidValue;

// forward and backward on one shape, first with null operands, then with every pointer "valid":
// rejected for the shape alone
static bool shape_reject(int P, int C, int Cr) {
  float* n = nullptr;
  const bool f0 = tp_bn_hswish_fwd_train(n, n, P, C, Cr, n, n, 1e-3f, 0.01f, n, n, n, n, n, n, nullptr, nullptr,
                                         nullptr) == BAD;
  const bool b0 = tp_bn_hswish_bwd_train(n, n, n, P, C, Cr, n, n, n, n, n, n, n, n, n, n, nullptr, nullptr) == BAD;
  const bool f1 = tp_bn_hswish_fwd_train(A16, A16, P, C, Cr, A16, A16, 1e-3f, 0.01f, A16, A16, A16, A16, A16, A16, W16,
                                         nullptr, nullptr) == BAD;
  const bool b1 = tp_bn_hswish_bwd_train(A16, A16, A16, P, C, Cr, A16, A16, A16, A16, A16, A16, A16, A16, A16, A16,
                                         W16, nullptr) == BAD;
  return f0 && b0 && f1 && b1;
}

int main() {
  // non-positive sizes
  EXPECT(shape_reject(0, 16, 16));
  EXPECT(shape_reject(-60, 16, 16));
  EXPECT(shape_reject(60, 0, 0));
  EXPECT(shape_reject(60, -16, 1));
  EXPECT(shape_reject(60, 16, 0));
  EXPECT(shape_reject(60, 16, -13));
  EXPECT(shape_reject(-2147483647 - 1, -2147483647 - 1, -2147483647 - 1));
  // more parameter channels than the activation carries
  EXPECT(shape_reject(60, 16, 17));
  EXPECT(shape_reject(60, 13, 14));
  EXPECT(shape_reject(60, 16, 2147483647));
  // 2^32 elements or more (and products that overflow 32 bits)
  EXPECT(shape_reject(1 << 16, 1 << 16, 1 << 16));  // exactly 2^32
  EXPECT(shape_reject(1 << 20, 4096, 4093));
  EXPECT(shape_reject(2147483647, 2147483647, 2147483647));
  EXPECT(shape_reject(2147483647, 3, 3));
  EXPECT(shape_reject(3, 2147483647, 1));
  // the backward recomputes the pre-activation from the forward's rows: both are required
  float* n = nullptr;
  EXPECT(tp_bn_hswish_bwd_train(A16, A16, A16, 60, 16, 13, A16, A16, A16, n, A16, A16, A16, A16, A16, A16, W16,
                                nullptr) == BAD);
  EXPECT(tp_bn_hswish_bwd_train(A16, A16, A16, 60, 16, 13, A16, A16, A16, A16, n, A16, A16, A16, A16, A16, W16,
                                nullptr) == BAD);
  EXPECT(tp_bn_hswish_bwd_train(A16, A16, n, 60, 13, 13, n, A16, A16, n, n, A16, A16, A16, A16, A16, W16, nullptr) ==
         BAD);  // (dx and gamma are nullable, af / bf are not)
  // Hardswish is no activation code of the existing entry points: 3 stays rejected there
  uint8_t* mk = reinterpret_cast<uint8_t*>(16);
  EXPECT(tp_bn_fwd_train(n, n, 64, 8, 8, n, n, 1e-5f, 0.1f, n, n, n, n, n, n, nullptr, n, 3, mk, nullptr, nullptr) ==
         BAD);

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("bn hswish validation ok\n");
  return 0;
}
