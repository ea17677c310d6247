// Host-side validation of the elementwise launchers (csrc/kernels/channel_reduce.hip, prune_ops.hip,
// shapley.hip, train_ops.hip, data_ops.hip), built with AddressSanitizer + UBSan on the host code like
// se_validation.cpp. Every launcher must reject, BEFORE touching the GPU, null pointers, non-positive
// sizes, modes and pool geometries that do not exist, batches past the grid limits and operands whose
// 32-bit index math would overflow; zero-work calls (an empty idx / keep, K = 0, n = 0) succeed without
// a launch; the reduction's workspace size covers what either NHWC kernel indexes; the dropout
// generator reproduces Philox4x32-10 vectors on the host, counters past 2^32 included. Runs on a
// CPU-only machine: no kernel is launched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned stand-ins: never dereferenced
static float* const A4 = reinterpret_cast<float*>(68);   // 4-byte aligned only
static double* const D16 = reinterpret_cast<double*>(64);
static int* const I16 = reinterpret_cast<int*>(64);
static int64_t* const L16 = reinterpret_cast<int64_t*>(64);
static uint8_t* const U16 = reinterpret_cast<uint8_t*>(64);
static const hipError_t BAD = hipErrorInvalidValue, OK = hipSuccess;
static const int BIG = 2147483647;

static bool reduce_reject(int B, int C, int S, int mode, int cl) {
  return tp_channel_reduce(A16, A16, A16, A16, B, C, S, mode, cl, nullptr) == BAD;
}

static void check_channel_reduce() {
  float* n = nullptr;
  for (int cl = 0; cl < 2; ++cl) {
    EXPECT(reduce_reject(0, 8, 16, 0, cl));
    EXPECT(reduce_reject(2, 0, 16, 0, cl));
    EXPECT(reduce_reject(2, 8, 0, 0, cl));
    EXPECT(reduce_reject(-2, 8, 16, 0, cl));
    EXPECT(reduce_reject(2, -8, 16, 0, cl));
    EXPECT(reduce_reject(2, 8, -16, 0, cl));
    EXPECT(reduce_reject(2, 8, 16, -1, cl));  // no such mode
    EXPECT(reduce_reject(2, 8, 16, 5, cl));
    EXPECT(reduce_reject(BIG, BIG, BIG, 0, cl));
    for (int mode = 0; mode < 5; ++mode) {
      const bool need_a = mode == 0 || mode == 1 || mode == 3, need_g = mode != 3;
      EXPECT(tp_channel_reduce(A16, A16, n, A16, 2, 32, 16, mode, cl, nullptr) == BAD);
      if (need_a) EXPECT(tp_channel_reduce(n, A16, A16, A16, 2, 32, 16, mode, cl, nullptr) == BAD);
      if (need_g) EXPECT(tp_channel_reduce(A16, n, A16, A16, 2, 32, 16, mode, cl, nullptr) == BAD);
    }
  }
  // the NHWC kernels launch grid.y = B
  EXPECT(reduce_reject(65536, 4, 4, 0, 1));
  EXPECT(reduce_reject(65536, 32, 4, 2, 1));
  EXPECT(reduce_reject(1 << 20, 1, 1, 3, 1));
  // B * C * chunks past 2^31: the workspace index
  EXPECT(tp_channel_reduce_ws_elems(65535, 8192, 4096, 1) == -1);
  EXPECT(reduce_reject(65535, 8192, 4096, 0, 1));
  EXPECT(tp_channel_reduce_ws_elems(BIG, BIG, BIG, 1) == -1 && tp_channel_reduce_ws_elems(BIG, BIG, 1, 0) == -1);
  EXPECT(tp_channel_reduce_ws_elems(0, 8, 8, 1) == -1 && tp_channel_reduce_ws_elems(8, -1, 8, 1) == -1 &&
         tp_channel_reduce_ws_elems(8, 8, 0, 0) == -1);
  // the workspace covers what either NHWC kernel indexes: ws[(b * chunks + z) * C + c]; no chunk
  // count past the 64 the kernels were written for, none past the positions
  for (int b = 1; b <= 4096; b = b < 4 ? b + 1 : b * 4)
    for (int c = 1; c <= 2048; c = c < 70 ? c + 1 : c + c / 5 + 1)
      for (int s = 1; s <= (1 << 16); s = s < 40 ? s + 1 : s + s / 6 + 1) {
        const int ws = tp_channel_reduce_ws_elems(b, c, s, 1);
        EXPECT(ws >= 0 && tp_channel_reduce_ws_elems(b, c, s, 0) == 0);
        for (int vec = 0; vec < 2; ++vec) {
          if (vec && c % 32) {
            EXPECT(tp_channel_reduce_chunks(b, c, s, 1) == 0);
            continue;
          }
          const int k = tp_channel_reduce_chunks(b, c, s, vec);
          EXPECT(k >= 1 && k <= 64 && k <= s);
          if (k > 1) EXPECT((long long)ws >= (long long)b * k * c);
          const int chunk = (s + k - 1) / k;
          EXPECT((long long)chunk * k >= s);  // the chunks cover every position
        }
      }
  EXPECT(tp_channel_reduce_chunks(0, 32, 64, 1) == 0 && tp_channel_reduce_chunks(2, 32, -1, 0) == 0);

  EXPECT(tp_column_accumulate(nullptr, D16, D16, 4, 8, nullptr) == BAD);
  EXPECT(tp_column_accumulate(A16, nullptr, D16, 4, 8, nullptr) == BAD);
  EXPECT(tp_column_accumulate(A16, D16, nullptr, 0, 8, nullptr) == BAD);
  EXPECT(tp_column_accumulate(A16, D16, nullptr, 4, 0, nullptr) == BAD);
  EXPECT(tp_column_accumulate(A16, D16, D16, -4, 8, nullptr) == BAD);
  EXPECT(tp_column_accumulate(A16, D16, D16, 4, -8, nullptr) == BAD);
}

static void check_score_fold() {
  float* T[17];
  double* acc[17];
  int B[17], C[17], R[17];
  for (int i = 0; i < 17; ++i) {
    T[i] = A16;
    acc[i] = D16;
    B[i] = 7;
    C[i] = 33;
    R[i] = 1;
  }
  EXPECT(tp_score_fold_ws_elems(B, C, 3) == 3 * 33);
  EXPECT(tp_score_fold_ws_elems(B, C, 0) == -1 && tp_score_fold_ws_elems(B, C, 17) == -1 &&
         tp_score_fold_ws_elems(nullptr, C, 3) == -1 && tp_score_fold_ws_elems(B, nullptr, 3) == -1);
  EXPECT(tp_score_fold_multi(T, acc, B, C, R, 0, 1, 0, D16, nullptr) == BAD);
  EXPECT(tp_score_fold_multi(T, acc, B, C, R, -1, 1, 0, D16, nullptr) == BAD);
  EXPECT(tp_score_fold_multi(T, acc, B, C, R, 17, 1, 0, D16, nullptr) == BAD);
  EXPECT(tp_score_fold_multi(nullptr, acc, B, C, R, 3, 1, 0, D16, nullptr) == BAD);
  EXPECT(tp_score_fold_multi(T, nullptr, B, C, R, 3, 1, 0, D16, nullptr) == BAD);
  EXPECT(tp_score_fold_multi(T, acc, nullptr, C, R, 3, 1, 0, D16, nullptr) == BAD);
  EXPECT(tp_score_fold_multi(T, acc, B, nullptr, R, 3, 1, 0, D16, nullptr) == BAD);
  EXPECT(tp_score_fold_multi(T, acc, B, C, nullptr, 3, 1, 0, D16, nullptr) == BAD);
  EXPECT(tp_score_fold_multi(T, acc, B, C, R, 3, 1, 0, nullptr, nullptr) == BAD);  // accumulators need ws
  EXPECT(tp_score_fold_multi(T, acc, B, C, R, 3, 1, 3, D16, nullptr) == BAD);      // no such ``after``
  EXPECT(tp_score_fold_multi(T, acc, B, C, R, 3, 1, -1, D16, nullptr) == BAD);
  T[1] = nullptr;
  EXPECT(tp_score_fold_multi(T, acc, B, C, R, 3, 1, 0, D16, nullptr) == BAD);
  T[1] = A16;
  for (int bad : {0, -5}) {
    B[2] = bad;
    EXPECT(tp_score_fold_multi(T, acc, B, C, R, 3, 1, 0, D16, nullptr) == BAD && tp_score_fold_ws_elems(B, C, 3) == -1);
    B[2] = 7;
    C[0] = bad;
    EXPECT(tp_score_fold_multi(T, acc, B, C, R, 3, 1, 0, D16, nullptr) == BAD && tp_score_fold_ws_elems(B, C, 3) == -1);
    C[0] = 33;
    R[1] = bad;
    EXPECT(tp_score_fold_multi(T, acc, B, C, R, 3, 1, 0, D16, nullptr) == BAD);
    R[1] = 1;
  }
  B[0] = BIG;  // count * row chunks * C past 2^31
  C[1] = BIG;
  EXPECT(tp_score_fold_ws_elems(B, C, 3) == -1);
  EXPECT(tp_score_fold_multi(T, acc, B, C, R, 3, 1, 0, D16, nullptr) == BAD);
}

static void check_prune_ops() {
  // channel_fill / nan_channels
  EXPECT(tp_channel_fill(nullptr, 2, 6, 9, L16, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 2, 6, 9, nullptr, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 0, 6, 9, L16, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 2, 0, 9, L16, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 2, 6, 0, L16, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, -2, 6, 9, L16, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 2, -6, 9, L16, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 2, 6, -9, L16, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 2, 6, 9, L16, -1, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 1ll << 62, BIG, 1ll << 62, L16, 2, 0.f, nullptr) == BAD);
  EXPECT(tp_channel_fill(A16, 2, 6, 9, nullptr, 0, 0.f, nullptr) == OK);  // an empty idx: nothing to do
  EXPECT(tp_channel_fill(A16, 2, 6, 9, L16, 0, 0.f, nullptr) == OK);
  EXPECT(tp_nan_channels(nullptr, 2, 6, 9, U16, nullptr) == BAD);
  EXPECT(tp_nan_channels(A16, 2, 6, 9, nullptr, nullptr) == BAD);
  EXPECT(tp_nan_channels(A16, 0, 6, 9, U16, nullptr) == BAD);
  EXPECT(tp_nan_channels(A16, 2, 0, 9, U16, nullptr) == BAD);
  EXPECT(tp_nan_channels(A16, 2, 6, 0, U16, nullptr) == BAD);
  EXPECT(tp_nan_channels(A16, -2, 6, 9, U16, nullptr) == BAD);
  EXPECT(tp_nan_channels(A16, 2, -6, 9, U16, nullptr) == BAD);
  EXPECT(tp_nan_channels(A16, 2, 6, -9, U16, nullptr) == BAD);
  EXPECT(tp_nan_channels(A16, 1ll << 62, BIG, 1ll << 62, U16, nullptr) == BAD);
  // gather_multi
  const void* srcs[9];
  void* dsts[9];
  long long outer[9], n[9], inner[9];
  for (int i = 0; i < 9; ++i) {
    srcs[i] = A16;
    dsts[i] = A16;
    outer[i] = 3;
    n[i] = 8;
    inner[i] = 5;
  }
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 0, 4, L16, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, -1, 4, L16, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 9, 4, L16, 4, nullptr) == BAD);
  for (int es : {0, 3, 5, 16, -4}) EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, es, L16, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(nullptr, dsts, outer, n, inner, 2, 4, L16, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(srcs, nullptr, outer, n, inner, 2, 4, L16, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(srcs, dsts, nullptr, n, inner, 2, 4, L16, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(srcs, dsts, outer, nullptr, inner, 2, 4, L16, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, nullptr, 2, 4, L16, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, 4, nullptr, 4, nullptr) == BAD);
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, 4, L16, -4, nullptr) == BAD);
  srcs[1] = nullptr;
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, 4, L16, 4, nullptr) == BAD);
  srcs[1] = A16;
  dsts[0] = nullptr;
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, 4, L16, 4, nullptr) == BAD);
  dsts[0] = A4;
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, 8, L16, 4, nullptr) == BAD);  // 8-byte elements at 4
  dsts[0] = A16;
  outer[1] = -3;
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, 4, L16, 4, nullptr) == BAD);
  outer[1] = 1ll << 40;
  inner[1] = 1ll << 40;
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, 4, L16, 4, nullptr) == BAD);
  outer[1] = 3;
  inner[1] = 5;
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 8, 4, nullptr, 0, nullptr) == OK);  // an empty keep
  EXPECT(tp_gather_multi(srcs, dsts, outer, n, inner, 2, 1, L16, 0, nullptr) == OK);
  // the engine's NHWC pools
  EXPECT(tp_maxpool2_nhwc(nullptr, A16, U16, 2, 4, 4, 8, nullptr) == BAD);
  EXPECT(tp_maxpool2_nhwc(A16, nullptr, U16, 2, 4, 4, 8, nullptr) == BAD);
  EXPECT(tp_maxpool2_nhwc(A16, A16, nullptr, 2, 4, 4, 8, nullptr) == BAD);
  EXPECT(tp_unpool2_nhwc(nullptr, U16, A16, 2, 4, 4, 8, nullptr) == BAD);
  EXPECT(tp_unpool2_nhwc(A16, nullptr, A16, 2, 4, 4, 8, nullptr) == BAD);
  EXPECT(tp_unpool2_nhwc(A16, U16, nullptr, 2, 4, 4, 8, nullptr) == BAD);
  const int dims[][4] = {{0, 4, 4, 8}, {2, 0, 4, 8}, {2, 4, 0, 8}, {2, 4, 4, 0}, {-2, 4, 4, 8},
                         {2, -4, 4, 8}, {2, 4, -4, 8}, {2, 4, 4, -8}, {2, 1, 4, 8}, {2, 4, 1, 8}};
  for (const auto& d : dims) {
    EXPECT(tp_maxpool2_nhwc(A16, A16, U16, d[0], d[1], d[2], d[3], nullptr) == BAD);
    EXPECT(tp_unpool2_nhwc(A16, U16, A16, d[0], d[1], d[2], d[3], nullptr) == BAD);
  }
  EXPECT(tp_maxpool_nhwc(nullptr, A16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, nullptr, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A4, A16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A4, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 8, 3, 0, 1, nullptr) == BAD);  // stride 0: was a division by zero
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 8, 0, 2, 0, nullptr) == BAD);  // window 0
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 8, 0, 0, 0, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 8, 3, -2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 8, -3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 8, 3, 2, -1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 8, 3, 2, 2, nullptr) == BAD);   // padding past half the window
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 8, 9, 2, 0, nullptr) == BAD);   // window past the image
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 6, 3, 2, 1, nullptr) == BAD);   // C % 4
  EXPECT(tp_maxpool_nhwc(A16, A16, 0, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 0, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, -6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, 7, 6, 0, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_nhwc(A16, A16, 2, BIG, BIG, 8, BIG, 1, BIG, nullptr) == BAD);
  EXPECT(tp_avgpool_nhwc(nullptr, A16, 2, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_nhwc(A16, nullptr, 2, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_nhwc(A16, A16, 0, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_nhwc(A16, A16, 2, 0, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_nhwc(A16, A16, 2, 49, 0, nullptr) == BAD);
  EXPECT(tp_avgpool_nhwc(A16, A16, -2, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_nhwc(A16, A16, 2, -49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_nhwc(A16, A16, 2, 49, -8, nullptr) == BAD);
}

static void check_shapley() {
  // prefix_mask(z, out, rank, N, C, S, channels_last, p0, K)
  for (int cl = 0; cl < 2; ++cl) {
    EXPECT(tp_prefix_mask(nullptr, A16, I16, 96, 6, 16, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, nullptr, I16, 96, 6, 16, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, nullptr, 96, 6, 16, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 0, 6, 16, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, -96, 6, 16, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 96, 0, 16, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 96, -6, 16, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 96, 6, 0, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 96, 6, -16, cl, 0, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 96, 6, 16, cl, -1, 2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 96, 6, 16, cl, 0, -2, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 97, 6, 16, cl, 0, 2, nullptr) == BAD);  // not whole (C, S) images
    EXPECT(tp_prefix_mask(A16, A16, I16, 96, 6, 16, cl, BIG, BIG, nullptr) == BAD);  // p0 + k is 32-bit
    EXPECT(tp_prefix_mask(A16, A16, I16, 1ll << 62, BIG, 1, cl, 0, BIG - 1, nullptr) == BAD);
    EXPECT(tp_prefix_mask(A16, A16, I16, 96, 6, 16, cl, 3, 0, nullptr) == OK);  // K = 0: nothing to do
    EXPECT(tp_prefix_mask(A4, A4, I16, 98, 7, 7, cl, 3, 0, nullptr) == OK);
  }
  // shapley_scatter(L, perm, sv, row0, B, n, k0, K, scale)
  double* nd = nullptr;
  EXPECT(tp_shapley_scatter(nullptr, I16, D16, 0, 4, 12, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, nullptr, D16, 0, 4, 12, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, nd, 0, 4, 12, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 0, 12, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, -4, 12, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 4, 0, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 4, -12, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, -1, 4, 12, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 4, 12, -1, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 4, 12, 0, -3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 4, 12, 10, 3, 1.0, nullptr) == BAD);  // k0 + K past the permutation
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 1 << 16, BIG, 0, 1 << 15, 1.0, nullptr) == BAD);  // K * B = 2^31
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 1 << 16, BIG, 0, (1 << 15) - 1, 1.0, nullptr) == BAD);  // (K+1) * B
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, BIG, BIG, 0, BIG, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_scatter(A16, I16, D16, BIG, 4, 12, 0, 3, 1.0, nullptr) == BAD);  // row0 + b is 32-bit
  EXPECT(tp_shapley_scatter(A16, I16, D16, 0, 4, 12, 5, 0, 1.0, nullptr) == OK);     // K = 0
  // shapley_column(L, perm, sv_col, B, k0, K, scale)
  EXPECT(tp_shapley_column(nullptr, I16, D16, 4, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, nullptr, D16, 4, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, I16, nd, 4, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, I16, D16, 0, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, I16, D16, -4, 0, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, I16, D16, 4, -1, 3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, I16, D16, 4, 0, -3, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, I16, D16, 1 << 16, 0, (1 << 15) - 1, 1.0, nullptr) == BAD);  // (K+1) * B = 2^31
  EXPECT(tp_shapley_column(A16, I16, D16, BIG, 0, BIG, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, I16, D16, 4, BIG, BIG, 1.0, nullptr) == BAD);
  EXPECT(tp_shapley_column(A16, I16, D16, 4, 5, 0, 1.0, nullptr) == OK);  // K = 0
  // cross_entropy(logits, target, loss, grad, B, NC, gscale); grad is optional
  EXPECT(tp_cross_entropy(nullptr, L16, A16, A16, 4, 10, 1.f, nullptr) == BAD);
  EXPECT(tp_cross_entropy(A16, nullptr, A16, A16, 4, 10, 1.f, nullptr) == BAD);
  EXPECT(tp_cross_entropy(A16, L16, nullptr, A16, 4, 10, 1.f, nullptr) == BAD);
  EXPECT(tp_cross_entropy(A16, L16, A16, nullptr, 0, 10, 1.f, nullptr) == BAD);
  EXPECT(tp_cross_entropy(A16, L16, A16, nullptr, 4, 0, 1.f, nullptr) == BAD);
  EXPECT(tp_cross_entropy(A16, L16, A16, A16, -4, 10, 1.f, nullptr) == BAD);
  EXPECT(tp_cross_entropy(A16, L16, A16, A16, 4, -10, 1.f, nullptr) == BAD);
  EXPECT(tp_cross_entropy(A16, L16, A16, A16, 1 << 25, 10, 1.f, nullptr) == BAD);  // 64 * B threads are 32-bit
  EXPECT(tp_cross_entropy(A16, L16, A16, A16, BIG, BIG, 1.f, nullptr) == BAD);
  // prefix_tri_operands(z, W, perm, B, C, N, p0, cnt, Kc, T, Wsub)
  EXPECT(tp_prefix_tri_operands(nullptr, A16, I16, 4, 16, 8, 0, 4, 4, A16, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, nullptr, I16, 4, 16, 8, 0, 4, 4, A16, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, nullptr, 4, 16, 8, 0, 4, 4, A16, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 16, 8, 0, 4, 4, nullptr, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 16, 8, 0, 4, 4, A16, nullptr, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 0, 16, 8, 0, 4, 4, A16, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 0, 8, 0, 4, 4, A16, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 16, 0, 0, 4, 4, A16, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 16, 8, -1, 4, 4, A16, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 16, 8, 0, 0, 4, A16, A16, nullptr) == BAD);
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 16, 8, 0, 5, 4, A16, A16, nullptr) == BAD);  // cnt > Kc
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 16, 8, 14, 4, 4, A16, A16, nullptr) == BAD);  // past the channels
  EXPECT(tp_prefix_tri_operands(A16, A16, I16, 4, 16, 8, BIG, BIG, BIG, A16, A16, nullptr) == BAD);
}

static void check_train_ops() {
  // dropout(x, y, n, seed, p)
  EXPECT(tp_dropout(nullptr, A16, 8, 1, 0.5, nullptr) == BAD);
  EXPECT(tp_dropout(A16, nullptr, 8, 1, 0.5, nullptr) == BAD);
  EXPECT(tp_dropout(A4, A16, 8, 1, 0.5, nullptr) == BAD);  // the body loads and stores float4
  EXPECT(tp_dropout(A16, A4, 8, 1, 0.5, nullptr) == BAD);
  EXPECT(tp_dropout(A4, A4, 3, 1, 0.5, nullptr) == BAD);
  EXPECT(tp_dropout(A16, A16, -8, 1, 0.5, nullptr) == BAD);
  for (double p : {1.0, 1.5, -0.1, -1.0, (double)HUGE_VAL, (double)NAN}) EXPECT(tp_dropout(A16, A16, 8, 1, p, nullptr) == BAD);
  EXPECT(tp_dropout(A16, A16, 0, 1, 0.5, nullptr) == OK);  // n = 0: nothing to do
  EXPECT(tp_dropout(nullptr, nullptr, 0, 1, 0.0, nullptr) == OK);
  // the generator: the kernel's counter form (ctr_lo, ctr_hi, 0, 0) with a 64-bit key. The round function
  // reproduces the published Random123 Philox4x32-10 vectors; these three come from the same transcription
  struct {
    unsigned long long ctr, key;
    unsigned w[4];
  } const vec[] = {{0ull, 0ull, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
                   {1ull, 0ull, {0xf8e4cca4u, 0x5cb200dbu, 0xb1a574ebu, 0x097eff67u}},
                   {(1ull << 32) + 5, 0x0123456789abcdefull, {0xb8b243f7u, 0xda8fb9a8u, 0x46004299u, 0xe54c389cu}}};
  for (const auto& v : vec) {
    unsigned w[4] = {0, 0, 0, 0};
    tp_philox4x32(v.ctr, v.key, w);
    EXPECT(w[0] == v.w[0] && w[1] == v.w[1] && w[2] == v.w[2] && w[3] == v.w[3]);
  }
  // training pools
  EXPECT(tp_maxpool_fwd_arg(nullptr, A16, U16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_fwd_arg(A16, nullptr, U16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_fwd_arg(A16, A16, nullptr, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_bwd(nullptr, U16, A16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_bwd(A16, nullptr, A16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_bwd(A16, U16, nullptr, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_fwd_arg(A4, A16, U16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_fwd_arg(A16, A4, U16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_fwd_arg(A16, A16, U16 + 1, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_bwd(A4, U16, A16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_bwd(A16, U16 + 2, A16, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  EXPECT(tp_maxpool_bwd(A16, U16, A4, 2, 7, 6, 8, 3, 2, 1, nullptr) == BAD);
  // (B, H, W, C, k, s, pad)
  const int geo[][7] = {{0, 7, 6, 8, 3, 2, 1}, {2, 0, 6, 8, 3, 2, 1}, {2, 7, 0, 8, 3, 2, 1}, {2, 7, 6, 0, 3, 2, 1},
                        {-2, 7, 6, 8, 3, 2, 1}, {2, -7, 6, 8, 3, 2, 1}, {2, 7, -6, 8, 3, 2, 1}, {2, 7, 6, -8, 3, 2, 1},
                        {2, 7, 6, 6, 3, 2, 1}, {2, 7, 6, 8, 0, 2, 0}, {2, 7, 6, 8, 3, 0, 1}, {2, 7, 6, 8, 0, 0, 0},
                        {2, 7, 6, 8, -3, 2, 1}, {2, 7, 6, 8, 3, -2, 1}, {2, 7, 6, 8, 3, 2, -1}, {2, 7, 6, 8, 3, 2, 2},
                        {2, 7, 6, 8, 7, 2, 0}, {2, 20, 20, 8, 16, 2, 0}, {2, BIG, BIG, 8, 65536, 1, 0},
                        {BIG, BIG, BIG, BIG - 3, 3, 1, 1}};
  for (const auto& g : geo) {
    EXPECT(tp_maxpool_fwd_arg(A16, A16, U16, g[0], g[1], g[2], g[3], g[4], g[5], g[6], nullptr) == BAD);
    EXPECT(tp_maxpool_bwd(A16, U16, A16, g[0], g[1], g[2], g[3], g[4], g[5], g[6], nullptr) == BAD);
  }
  EXPECT(tp_avgpool_bwd(nullptr, A16, 2, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, nullptr, 2, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A4, A16, 2, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, A4, 2, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, A16, 0, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, A16, 2, 0, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, A16, 2, 49, 0, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, A16, -2, 49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, A16, 2, -49, 8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, A16, 2, 49, -8, nullptr) == BAD);
  EXPECT(tp_avgpool_bwd(A16, A16, 2, 49, 6, nullptr) == BAD);  // C % 4
}

static void check_data_ops() {
  // augment_u8(src, idx, aug, B, C, H, W, pad, mean, inv_std, out); aug is optional
  EXPECT(tp_augment_u8(nullptr, L16, I16, 2, 3, 8, 8, 1, A16, A16, A16, nullptr) == BAD);
  EXPECT(tp_augment_u8(U16, nullptr, I16, 2, 3, 8, 8, 1, A16, A16, A16, nullptr) == BAD);
  EXPECT(tp_augment_u8(U16, L16, nullptr, 2, 3, 8, 8, 1, nullptr, A16, A16, nullptr) == BAD);
  EXPECT(tp_augment_u8(U16, L16, nullptr, 2, 3, 8, 8, 1, A16, nullptr, A16, nullptr) == BAD);
  EXPECT(tp_augment_u8(U16, L16, nullptr, 2, 3, 8, 8, 1, A16, A16, nullptr, nullptr) == BAD);
  const int d[][5] = {{0, 3, 8, 8, 1}, {2, 0, 8, 8, 1}, {2, 3, 0, 8, 1}, {2, 3, 8, 0, 1}, {-2, 3, 8, 8, 1},
                      {2, -3, 8, 8, 1}, {2, 3, -8, 8, 1}, {2, 3, 8, -8, 1}, {2, 3, 8, 8, -1}};
  for (const auto& g : d)
    EXPECT(tp_augment_u8(U16, L16, I16, g[0], g[1], g[2], g[3], g[4], A16, A16, A16, nullptr) == BAD);
}

int main() {
  check_channel_reduce();
  check_score_fold();
  check_prune_ops();
  check_shapley();
  check_train_ops();
  check_data_ops();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("elementwise validation ok\n");
  return 0;
}
