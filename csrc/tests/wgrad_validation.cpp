// Host-side validation of the conv weight-gradient launchers (csrc/kernels/conv_wgrad.hip,
// csrc/kernels/wino_wgrad.hip), built with AddressSanitizer + UBSan on the host code like
// prefix_project_validation.cpp. Both launchers must reject, BEFORE touching the GPU and before any
// arithmetic on the sizes (an empty batch and a zero stride used to divide by zero): missing or
// misaligned operands, empty shapes, a bad geometry (ks < 1, stride < 1, pad < 0, a kernel larger
// than the padded map), pixel counts that do not fit 32 bits, non-positive output strides and an
// unknown tile config. Every call below differs from a launchable one in the one argument its
// comment names. Runs on a CPU-only machine: no kernel is launched.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned, never dereferenced
static float* const A4 = reinterpret_cast<float*>(68);   // 4-byte aligned only
static float* const A2 = reinterpret_cast<float*>(66);   // off a float boundary
static float* const Z = nullptr;
static const hipError_t BAD = hipErrorInvalidValue;
static const long long FS[4] = {576, 9, 3, 1};  // a contiguous (64, 64, 3, 3) parameter

// 3x3 conv on (B, H, W, Cin) -> Cout, Kpad = 9 * Cin rounded up to 32
static hipError_t geom(int B, int H, int W, int Cin, int Cout, int ks, int stride, int pad, long long kpad = -1) {
  const long long k = kpad >= 0 ? kpad : ((long long)ks * ks * Cin + 31) / 32 * 32;
  return tp_conv_wgrad(A16, A16, A16, A16, B, H, W, Cin, Cout, ks, stride, pad, (int)k, 0, 1, nullptr, 0, 0, nullptr, 1,
                       0, 0, nullptr);
}

static hipError_t ptrs(const float* g, const float* x, float* dw, float* ws, float* fin) {
  return tp_conv_wgrad(g, x, dw, ws, 2, 8, 8, 64, 64, 3, 1, 1, 576, 0, 2, fin, 64, 64, FS, 1, 0, 0, nullptr);
}

static hipError_t fin_strides(long long s0, long long s1, long long s2, long long s3, int co = 64, int ci = 64) {
  const long long fs[4] = {s0, s1, s2, s3};
  return tp_conv_wgrad(A16, A16, Z, A16, 2, 8, 8, 64, 64, 3, 1, 1, 576, 0, 1, A4, co, ci, fs, 1, 0, 0, nullptr);
}

static hipError_t wino(const float* g, const float* x, float* ws, int B, int H, int W, int Cin, int Cout, int cfg,
                       int splits, float* fin, int co, int ci, const long long* fs) {
  return tp_wino_wgrad(g, x, ws, B, H, W, Cin, Cout, cfg, splits, fin, co, ci, fs, nullptr);
}

int main() {
  const int MAXI = 2147483647;
  // ---------------------------------------------------------------- tp_conv_wgrad
  // the checks the launcher already had (from launcher_validation.cpp, now with real pointers)
  EXPECT(geom(2, 8, 8, 6, 64, 3, 1, 1, 64) == BAD);     // Cin % 4
  EXPECT(geom(2, 8, 8, 64, 64, 3, 1, 1, 96) == BAD);    // Kpad small
  EXPECT(tp_conv_wgrad(A16, A16, A16, A16, 2, 8, 8, 64, 64, 3, 1, 1, 576, 7, 1, nullptr, 0, 0, nullptr, 1, 0, 0,
                       nullptr) == BAD);                // bad cfg
  EXPECT(geom(2, 8, 8, 64, 62, 3, 1, 1) == BAD);        // Cout % 4
  EXPECT(geom(2, 8, 8, 64, 64, 3, 1, 1, 580) == BAD);   // Kpad % 32
  // empty shapes: B = 0 divided by zero (splits = min(splits, 0 slices))
  EXPECT(geom(0, 8, 8, 64, 64, 3, 1, 1) == BAD);
  EXPECT(geom(-2, 8, 8, 64, 64, 3, 1, 1) == BAD);
  EXPECT(geom(2, 0, 8, 64, 64, 3, 1, 1) == BAD);
  EXPECT(geom(2, -8, 8, 64, 64, 3, 1, 1) == BAD);
  EXPECT(geom(2, 8, 0, 64, 64, 3, 1, 1) == BAD);
  EXPECT(geom(2, 8, -8, 64, 64, 3, 1, 1) == BAD);
  EXPECT(geom(2, 8, 8, 0, 64, 3, 1, 1) == BAD);
  EXPECT(geom(2, 8, 8, -64, 64, 3, 1, 1, 576) == BAD);
  EXPECT(geom(2, 8, 8, 64, 0, 3, 1, 1) == BAD);
  EXPECT(geom(2, 8, 8, 64, -64, 3, 1, 1) == BAD);
  // geometry: stride = 0 divided by zero
  EXPECT(geom(2, 8, 8, 64, 64, 0, 1, 1, 576) == BAD);   // ks < 1
  EXPECT(geom(2, 8, 8, 64, 64, -3, 1, 1) == BAD);
  EXPECT(geom(2, 8, 8, 64, 64, 3, 0, 1) == BAD);        // stride < 1
  EXPECT(geom(2, 8, 8, 64, 64, 3, -1, 1) == BAD);
  EXPECT(geom(2, 8, 8, 64, 64, 3, 1, -1) == BAD);       // pad < 0
  // a kernel larger than the padded map: Ho = Wo = -4 gave P = 32 > 0 and a launch
  EXPECT(geom(2, 2, 2, 64, 64, 7, 1, 0) == BAD);
  EXPECT(geom(2, 2, 8, 64, 64, 7, 1, 0) == BAD);        // Ho alone
  EXPECT(geom(2, 8, 2, 64, 64, 7, 1, 0) == BAD);        // Wo alone
  EXPECT(geom(2, 2, 2, 64, 64, 4, 2, 0) == BAD);        // numerator -2, stride 2: C++ division gives Ho = 0
  EXPECT(geom(2, 2, 2, 64, 64, 3, 2, 0) == BAD);        // numerator -1, stride 2: C++ division gives Ho = 1
  // pixel counts and operand sizes that overflow 32 bits (P is formed in 64 bits, then narrowed)
  EXPECT(geom(1 << 16, 1 << 8, 1 << 8, 4, 4, 1, 1, 0) == BAD);       // P = 2^32 (wraps to 0 in 32 bits)
  EXPECT(geom((1 << 16) + 1, 1 << 8, 1 << 8, 4, 4, 1, 1, 0) == BAD);  // P = 2^32 + 2^16 (wraps to 65536)
  EXPECT(geom(MAXI, MAXI, MAXI, 4, 4, 1, 1, 0) == BAD);
  EXPECT(geom(MAXI, 1, 1, 4, 4, 1, 1, 0) == BAD);
  EXPECT(geom(1, MAXI, 1, 4, 4, 1, 1, 0) == BAD);
  EXPECT(geom(1, 1, MAXI, 4, 4, 1, 1, 0) == BAD);
  EXPECT(geom(1, 1, 1, 4, 4, 1, 1, MAXI) == BAD);                    // 2 * pad in 64 bits
  EXPECT(geom(1, 1, 1, 4, 4, 1, 1, 1 << 30) == BAD);
  EXPECT(geom(1 << 13, 1 << 8, 1 << 8, 4, 4, 1, 1, 0) == BAD);       // x, g: exactly 2^31 bytes
  EXPECT(geom(2, 8, 8, 2147483644, 4, 1, 1, 0, 0) == BAD);           // Kpad < Kc in 64 bits
  EXPECT(geom(2, 8, 8, 1 << 20, 4, 46341, 1, 46340, 2147483616) == BAD);  // ks * ks * Cin overflows 32 bits
  // missing and misaligned operands, one at a time (2 splits, a parameter-layout output)
  EXPECT(ptrs(Z, A16, A16, A16, A4) == BAD);
  EXPECT(ptrs(A16, Z, A16, A16, A4) == BAD);
  EXPECT(ptrs(A16, A16, A16, Z, A4) == BAD);    // 2 splits without a workspace
  EXPECT(ptrs(A16, A16, Z, A16, Z) == BAD);     // neither dw nor fin
  EXPECT(ptrs(A4, A16, A16, A16, A4) == BAD);
  EXPECT(ptrs(A16, A4, A16, A16, A4) == BAD);
  EXPECT(ptrs(A16, A16, A4, A16, A4) == BAD);
  EXPECT(ptrs(A16, A16, A16, A4, A4) == BAD);
  EXPECT(ptrs(A16, A16, A16, A16, A2) == BAD);
  EXPECT(ptrs(A2, A16, A16, A16, A4) == BAD);
  // the parameter-layout output: channel counts and strides
  EXPECT(fin_strides(576, 9, 3, 1, 0, 64) == BAD);
  EXPECT(fin_strides(576, 9, 3, 1, 64, 0) == BAD);
  EXPECT(fin_strides(576, 9, 3, 1, 68, 64) == BAD);
  EXPECT(fin_strides(576, 9, 3, 1, 64, 68) == BAD);
  EXPECT(fin_strides(0, 9, 3, 1) == BAD);
  EXPECT(fin_strides(576, 0, 3, 1) == BAD);
  EXPECT(fin_strides(576, 9, 0, 1) == BAD);
  EXPECT(fin_strides(576, 9, 3, 0) == BAD);
  EXPECT(fin_strides(-576, 9, 3, 1) == BAD);
  EXPECT(fin_strides(576, 9, 3, -1) == BAD);
  EXPECT(tp_conv_wgrad(A16, A16, Z, A16, 2, 8, 8, 64, 64, 3, 1, 1, 576, 0, 1, A4, 64, 64, nullptr, 1, 0, 0,
                       nullptr) == BAD);  // fin without strides
  // splits and batches
  EXPECT(tp_conv_wgrad(A16, A16, A16, A16, 2, 8, 8, 64, 64, 3, 1, 1, 576, 0, 0, nullptr, 0, 0, nullptr, 1, 0, 0,
                       nullptr) == BAD);
  EXPECT(tp_conv_wgrad(A16, A16, A16, A16, 2, 8, 8, 64, 64, 3, 1, 1, 576, 0, 1, nullptr, 0, 0, nullptr, 0, 0, 0,
                       nullptr) == BAD);
  EXPECT(tp_conv_wgrad(A16, A16, A16, A16, 2, 8, 8, 64, 64, 3, 1, 1, 576, 0, 1, nullptr, 0, 0, nullptr, 65536, 0, 0,
                       nullptr) == BAD);
  EXPECT(tp_conv_wgrad(A16, A16, A16, A16, 2, 8, 8, 64, 64, 3, 1, 1, 576, 0, 1, A4, 64, 64, FS, 16, 0, 0, nullptr) ==
         BAD);  // batched GEMMs have no parameter-layout output
  EXPECT(tp_conv_wgrad(A16, A16, A16, A16, 2, 8, 8, 64, 64, 3, 1, 1, 576, -1, 1, nullptr, 0, 0, nullptr, 1, 0, 0,
                       nullptr) == BAD);  // cfg < 0

  // ---------------------------------------------------------------- tp_wino_wgrad
  // launchable: wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS)
  EXPECT(wino(Z, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, Z, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, Z, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, Z, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, nullptr) == BAD);
  EXPECT(wino(A4, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A4, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A4, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A2, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 0, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);   // empty shapes
  EXPECT(wino(A16, A16, A16, -2, 8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 0, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, -8, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 0, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, -8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 0, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, -64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 0, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 4, 64, 0, 1, A4, 64, 4, FS) == BAD);     // Cin < 8
  EXPECT(wino(A16, A16, A16, 2, 7, 8, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);   // odd H
  EXPECT(wino(A16, A16, A16, 2, 8, 7, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);   // odd W
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 62, 64, 0, 1, A4, 64, 62, FS) == BAD);   // Cin % 4
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 62, 0, 1, A4, 62, 64, FS) == BAD);   // Cout % 4
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 0, A4, 64, 64, FS) == BAD);   // splits < 1
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 0, 64, FS) == BAD);    // fin_co / fin_ci
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 0, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, -1, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, -1, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 68, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 68, FS) == BAD);
  for (int i = 0; i < 4; ++i) {
    long long fs[4] = {576, 9, 3, 1};
    fs[i] = 0;
    EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, fs) == BAD);
    fs[i] = -FS[i];
    EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 0, 1, A4, 64, 64, fs) == BAD);
  }
  // an unknown tile config is refused before the transform kernels are launched
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 3, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, -1, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 2, 8, 8, 64, 64, 7, 4, A4, 64, 64, FS) == BAD);
  // tile counts and operands past 32 bits
  EXPECT(wino(A16, A16, A16, MAXI, 2147483646, 2147483646, 64, 64, 0, 1, A4, 64, 64, FS) == BAD);
  EXPECT(wino(A16, A16, A16, 1 << 20, 64, 64, 8, 8, 0, 1, A4, 8, 8, FS) == BAD);   // T = 2^30: T * Cin * 4 = 2^35
  EXPECT(wino(A16, A16, A16, 1 << 12, 64, 64, 128, 8, 0, 1, A4, 8, 8, FS) == BAD);  // V plane: exactly 2^31 bytes
  EXPECT(wino(A16, A16, A16, 1 << 12, 64, 64, 8, 128, 0, 1, A4, 8, 8, FS) == BAD);  // dM plane: exactly 2^31 bytes
  EXPECT(wino(A16, A16, A16, 1, 2, 2, 2147483644, 8, 0, 1, A4, 8, 8, FS) == BAD);   // Cin + 31 overflows 32 bits
  EXPECT(wino(A16, A16, A16, 1, 2, 2, 8, 2147483644, 0, 1, A4, 8, 8, FS) == BAD);
  // the workspace helper: V + dM + dU (+ splits slabs of dU's size when split)
  EXPECT(tp_wino_wgrad_ws_elems(2, 8, 8, 64, 64, 1) == 16ll * 32 * 64 * 2 + 16ll * 64 * 64);
  EXPECT(tp_wino_wgrad_ws_elems(2, 8, 8, 36, 64, 3) == 16ll * 32 * (36 + 64) + 16ll * 64 * 64 * 4);

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("wgrad validation ok\n");
  return 0;
}
