// Host-side validation of the nine-product 2x2-map conv launchers (csrc/kernels/conv2x2_fast.hip and
// the batched GEMM launcher of conv_mfma.hip), built with AddressSanitizer + UBSan on the host code
// like prefix_project_validation.cpp. The launchers must reject, BEFORE touching the GPU, channel
// counts off the K-slice / float4 granules, empty shapes, unknown tile configs, split counts that
// are not normalised, operands of 2^31 bytes or more, and missing or misaligned operands. Runs on
// a CPU-only machine: no kernel is launched.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned, never dereferenced
static float* const A4 = reinterpret_cast<float*>(68);   // 4-byte aligned only
static uint8_t* const B4 = reinterpret_cast<uint8_t*>(68);
static uint8_t* const B1 = reinterpret_cast<uint8_t*>(65);

static bool fwd_rejects(int B, int C, int K, int cfg, int splits) {
  return tp_conv2x2_fast_fwd(A16, A16, B, C, K, cfg, splits, A16, A16, 1, 0, A16, nullptr, A16, A16, nullptr) ==
         hipErrorInvalidValue;
}

static bool bwd_rejects(int B, int Cg, int Cin, int cfg, int splits, int tay_mode) {
  return tp_conv2x2_fast_dgrad(A16, nullptr, A16, B, Cg, Cin, cfg, splits, A16, A16, A16, tay_mode, A16, A16, A16,
                               nullptr) == hipErrorInvalidValue;
}

static bool gemm_rejects(int nbatch, int M, int K, int N, int cfg, int splits) {
  return tp_conv_igemm_batched(A16, A16, nbatch, M, K, N, cfg, splits, A16, nullptr) == hipErrorInvalidValue;
}

int main() {
  const int MAXI = 2147483647;
  // the split normalisation the launchers insist on: no empty K range
  EXPECT(tp_conv_norm_splits(1, 512) == 1);
  EXPECT(tp_conv_norm_splits(2, 512) == 2);
  EXPECT(tp_conv_norm_splits(3, 128) == 2);  // 4 slices in ranges of 2
  EXPECT(tp_conv_norm_splits(7, 64) == 2);
  EXPECT(tp_conv_norm_splits(0, 64) == 1);
  EXPECT(tp_conv_norm_splits(-5, 64) == 1);
  EXPECT(tp_conv_norm_splits(4, 0) == 1);
  EXPECT(tp_conv_norm_splits(MAXI, 2147483616) == 67108863);
  for (int dir = 0; dir < 2; ++dir) {
    auto rejects = [&](int B, int Ci, int Co, int cfg, int splits) {
      return dir ? bwd_rejects(B, Ci, Co, cfg, splits, 0) : fwd_rejects(B, Ci, Co, cfg, splits);
    };
    // input channels off the 32-wide K slice, output channels off the float4 granule
    EXPECT(rejects(8, 48, 64, 0, 1));
    EXPECT(rejects(8, 16, 64, 0, 1));
    EXPECT(rejects(8, 0, 64, 0, 1));
    EXPECT(rejects(8, -32, 64, 0, 1));
    EXPECT(rejects(8, 64, 30, 0, 1));
    EXPECT(rejects(8, 64, 0, 0, 1));
    EXPECT(rejects(8, 64, -4, 0, 1));
    // empty batches
    EXPECT(rejects(0, 64, 64, 0, 1));
    EXPECT(rejects(-1, 64, 64, 0, 1));
    // tile configs
    EXPECT(rejects(8, 64, 64, -1, 1));
    EXPECT(rejects(8, 64, 64, 7, 1));
    EXPECT(rejects(8, 64, 64, 32, 1));  // stream-K flag: not offered here
    EXPECT(rejects(8, 64, 64, 256, 1));
    EXPECT(rejects(8, 64, 64, MAXI, 1));
    // splits: below 1, more than K slices, not normalised, more slabs than grid.y holds
    EXPECT(rejects(8, 64, 64, 0, 0));
    EXPECT(rejects(8, 64, 64, 0, -2));
    EXPECT(rejects(8, 64, 64, 0, 3));
    EXPECT(rejects(8, 128, 64, 0, 3));
    EXPECT(rejects(8, 64, 64, 0, MAXI));
    EXPECT(rejects(8, 1 << 20, 64, 0, 8192));
    // operands of 2^31 bytes or more per batch (and products that overflow 32 bits)
    EXPECT(rejects(1 << 20, 512, 64, 0, 1));   // V: 2^31 bytes per product
    EXPECT(rejects(1 << 20, 64, 512, 0, 1));   // slab: 2^31 bytes
    EXPECT(rejects(8, 1 << 15, 1 << 14, 0, 1));  // U: 2^31 bytes per product
    EXPECT(rejects(MAXI, 2147483616, 2147483644, 0, 1));
    EXPECT(rejects(MAXI, 32, 4, 0, 1));
  }
  EXPECT(bwd_rejects(8, 64, 64, 0, 1, -1));
  EXPECT(bwd_rejects(8, 64, 64, 0, 1, 3));
  // the batched GEMM launcher itself
  EXPECT(gemm_rejects(0, 8, 64, 64, 0, 1));
  EXPECT(gemm_rejects(9, 0, 64, 64, 0, 1));
  EXPECT(gemm_rejects(9, 8, 48, 64, 0, 1));
  EXPECT(gemm_rejects(9, 8, 0, 64, 0, 1));
  EXPECT(gemm_rejects(9, 8, 64, 0, 0, 1));
  EXPECT(gemm_rejects(9, 8, 64, 64, 7, 1));
  EXPECT(gemm_rejects(9, 8, 64, 64, 0, 3));
  EXPECT(gemm_rejects(9, 8, 64, 64, 0, 0));
  EXPECT(gemm_rejects(65536, 8, 64, 64, 0, 1));
  EXPECT(gemm_rejects(32768, 8, 64, 64, 0, 2));
  EXPECT(gemm_rejects(MAXI, 8, 64, 64, 0, 2));
  EXPECT(gemm_rejects(9, 1 << 20, 512, 64, 0, 1));
  EXPECT(gemm_rejects(9, 1 << 20, 64, 2048, 0, 1));
  EXPECT(gemm_rejects(9, MAXI, 2147483616, MAXI, 0, 1));
  float* z = nullptr;
  EXPECT(tp_conv_igemm_batched(z, A16, 9, 8, 64, 64, 0, 1, A16, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_conv_igemm_batched(A16, z, 9, 8, 64, 64, 0, 1, A16, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_conv_igemm_batched(A16, A16, 9, 8, 64, 64, 0, 1, z, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_conv_igemm_batched(A4, A16, 9, 8, 64, 64, 0, 1, A16, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_conv_igemm_batched(A16, A4, 9, 8, 64, 64, 0, 1, A16, nullptr) == hipErrorInvalidValue);
  EXPECT(tp_conv_igemm_batched(A16, A16, 9, 8, 64, 64, 0, 1, A4, nullptr) == hipErrorInvalidValue);
  // missing and misaligned operands of the forward, one at a time (scale / shift are nullable; the
  // argmax bytes are needed with the pool only and read as dwords)
#define FW(x, u, sc, sh, pool, out, am, V, S) \
  tp_conv2x2_fast_fwd(x, u, 8, 64, 64, 0, 1, sc, sh, 1, pool, out, am, V, S, nullptr)
  EXPECT(FW(z, A16, A16, A16, 0, A16, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, z, A16, A16, 0, A16, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A16, 0, z, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A16, 0, A16, nullptr, z, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A16, 0, A16, nullptr, A16, z) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A16, 1, A16, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A16, 1, A16, B1, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A4, A16, A16, A16, 0, A16, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A4, A16, A16, 0, A16, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A4, A16, 0, A16, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A4, 0, A16, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A16, 0, A4, nullptr, A16, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A16, 0, A16, nullptr, A4, A16) == hipErrorInvalidValue);
  EXPECT(FW(A16, A16, A16, A16, 0, A16, nullptr, A16, A4) == hipErrorInvalidValue);
#undef FW
  // ... and of the data gradient (bn_scale nullable; one of out / taylor is needed)
#define BW(g, am, u, act, sc, tay, out, V, S) \
  tp_conv2x2_fast_dgrad(g, am, u, 8, 64, 64, 0, 1, act, sc, tay, 0, out, V, S, nullptr)
  EXPECT(BW(z, B4, A16, A16, A16, A16, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, z, A16, A16, A16, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, z, A16, A16, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A16, A16, z, z, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A16, A16, A16, A16, z, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A16, A16, A16, A16, A16, z) == hipErrorInvalidValue);
  EXPECT(BW(A4, B4, A16, A16, A16, A16, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B1, A16, A16, A16, A16, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A4, A16, A16, A16, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A4, A16, A16, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A16, A4, A16, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A16, A16, A4, A16, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A16, A16, A16, A4, A16, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A16, A16, A16, A16, A4, A16) == hipErrorInvalidValue);
  EXPECT(BW(A16, B4, A16, A16, A16, A16, A16, A16, A4) == hipErrorInvalidValue);
#undef BW

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("conv2x2_fast validation ok\n");
  return 0;
}
