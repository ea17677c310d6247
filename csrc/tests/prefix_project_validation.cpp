// Host-side validation of the prefix-scan project-conv launcher (csrc/kernels/prefix_project.hip),
// built with AddressSanitizer + UBSan on the host code like dwconv_act_validation.cpp. The launcher
// must reject, BEFORE touching the GPU, an output width that is no multiple of 4, empty shapes, a
// prefix range outside the permutation (cnt < 1, p0 < 0, p0 + cnt - 1 > n, n > C), missing or
// misaligned operands and operands of 2^31 bytes or more. Runs on a CPU-only machine: no kernel is
// launched.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned, never dereferenced
static float* const A4 = reinterpret_cast<float*>(68);   // 4-byte aligned only
static float* const A2 = reinterpret_cast<float*>(66);   // off a float boundary
static int* const P4 = reinterpret_cast<int*>(68);
static int* const P2 = reinterpret_cast<int*>(66);

static bool rejects(int N, int C, int Co, int n, int p0, int cnt) {
  return tp_prefix_project(A16, A16, A16, A16, P4, A16, N, C, Co, n, p0, cnt, nullptr) == hipErrorInvalidValue;
}

int main() {
  const int MAXI = 2147483647;
  // output widths that are no multiple of 4 (the engine pads to 32)
  EXPECT(rejects(50, 64, 30, 57, 0, 2));
  EXPECT(rejects(50, 64, 2, 57, 0, 2));
  EXPECT(rejects(50, 64, 0, 57, 0, 2));
  EXPECT(rejects(50, 64, -4, 57, 0, 2));
  EXPECT(rejects(50, 64, MAXI, 57, 0, 2));
  // empty shapes
  EXPECT(rejects(0, 64, 32, 57, 0, 2));
  EXPECT(rejects(-3, 64, 32, 57, 0, 2));
  EXPECT(rejects(50, 0, 32, 0, 0, 1));
  EXPECT(rejects(50, -64, 32, 0, 0, 1));
  // the prefix range: cnt < 1, p0 < 0, p0 + cnt - 1 > n, n > C (and sums that overflow 32 bits)
  EXPECT(rejects(50, 64, 32, 57, 0, 0));
  EXPECT(rejects(50, 64, 32, 57, 0, -1));
  EXPECT(rejects(50, 64, 32, 57, -1, 2));
  EXPECT(rejects(50, 64, 32, 57, 0, 59));   // 0 + 59 - 1 = 58 > 57
  EXPECT(rejects(50, 64, 32, 57, 57, 2));   // 57 + 2 - 1 = 58 > 57
  EXPECT(rejects(50, 64, 32, 57, 58, 1));
  EXPECT(rejects(50, 64, 32, 57, MAXI, 2));
  EXPECT(rejects(50, 64, 32, 57, 2, MAXI));
  EXPECT(rejects(50, 64, 32, 57, MAXI, MAXI));
  EXPECT(rejects(50, 64, 32, 65, 0, 2));    // n > C
  EXPECT(rejects(50, 64, 32, MAXI, 0, 2));
  EXPECT(rejects(50, 64, 32, -1, 0, 1));
  // operands of 2^31 bytes or more (and arguments whose products overflow 32 / 64 bits)
  EXPECT(rejects(1 << 24, 64, 32, 57, 0, 1));          // base: exactly 2^31 bytes
  EXPECT(rejects(1 << 19, 1024, 32, 57, 0, 1));        // a: exactly 2^31 bytes
  EXPECT(rejects(4, 1 << 15, 1 << 14, 57, 0, 1));      // wt: exactly 2^31 bytes
  EXPECT(rejects(1 << 19, 64, 32, 57, 0, 32));         // out: 32 copies of 2^26 bytes
  EXPECT(rejects(1 << 10, 64, 32, 64, 0, 1 << 14 | 1));
  EXPECT(rejects(MAXI, MAXI, 2147483644, MAXI, 0, MAXI));
  EXPECT(rejects(MAXI, 1, 4, 1, 0, 1));
  EXPECT(rejects(1, MAXI, 4, 1, 0, 1));
  EXPECT(rejects(1, 1, 2147483644, 1, 0, 1));
  // missing and misaligned operands, one at a time: the float4 operands (base, wt, out) need 16
  // bytes, the scalar ones (a, fill, perm) their natural 4
  float* z = nullptr;
  int* zp = nullptr;
#define PP(base, a, fill, wt, perm, out) tp_prefix_project(base, a, fill, wt, perm, out, 50, 64, 32, 57, 1, 7, nullptr)
  EXPECT(PP(z, A16, A16, A16, P4, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, z, A16, A16, P4, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, A16, z, A16, P4, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, A16, A16, z, P4, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, A16, A16, A16, zp, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, A16, A16, A16, P4, z) == hipErrorInvalidValue);
  EXPECT(PP(A4, A16, A16, A16, P4, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, A16, A16, A4, P4, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, A16, A16, A16, P4, A4) == hipErrorInvalidValue);
  EXPECT(PP(A16, A2, A16, A16, P4, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, A16, A2, A16, P4, A16) == hipErrorInvalidValue);
  EXPECT(PP(A16, A16, A16, A16, P2, A16) == hipErrorInvalidValue);
#undef PP

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("prefix_project validation ok\n");
  return 0;
}
