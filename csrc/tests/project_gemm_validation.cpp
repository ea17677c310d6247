// Host-side validation of the project GEMM launchers (csrc/kernels/scaled_project.hip, silu_project.hip,
// silu_prefix_project.hip), built with AddressSanitizer + UBSan on the host code like
// prefix_project_validation.cpp. Each launcher must reject, BEFORE touching the GPU, what its header comment
// promises: missing or misaligned operands, empty shapes, widths that are no multiple of 4 (forward and prefix:
// above 128), rows that are not B * HW, a prefix range outside the permutation, a wrong slab slot count or
// tay_mode, and operands of 2^31 bytes or more; the 64-bit size products must not overflow on the way. Every
// case starts from arguments the launcher accepts and breaks ONE of them, so it is the named check that
// fires. tp_silu_project_tay_slots is compared with a brute-force count of the 64-row tiles an image meets.
// Runs on a CPU-only machine: no kernel is launched.
//
// Two promised checks cannot be reached alone: the dgrad's R * B * C >= 2^29 (R <= HW for the one R the
// launcher takes, so R * B * C <= N * C, which the shape check bounds first), and the scaled bias stack
// (never larger than the out stack, which is checked before it). They are met here only together with that
// earlier check.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "tp_expect.h"
#include "tp_launchers.h"

static float* const A16 = reinterpret_cast<float*>(64);  // aligned, never dereferenced
static float* const A4 = reinterpret_cast<float*>(68);   // 4-byte aligned only
static int* const P16 = reinterpret_cast<int*>(64);
static int* const P4 = reinterpret_cast<int*>(68);
static int* const P2 = reinterpret_cast<int*>(66);
static float* const NUL = nullptr;
static const int MAXI = 2147483647, MAX4 = 2147483644;  // MAX4: the largest multiple of 4
static const hipError_t BAD = hipErrorInvalidValue;

// ------------------------------------------------------------------ tp_scaled_project
struct Sp {  // a shape the launcher accepts: 3 images of 49 rows, 40 -> 36 channels, 6 copies
  const float *a = A16, *sc = A16, *wt = A16, *bias = A16, *res = A16;
  float* out = A16;
  int N = 147, C = 40, Co = 36, B = 3, HW = 49, cnt = 6;
  bool rejected() const { return tp_scaled_project(a, sc, wt, bias, res, out, N, C, Co, B, HW, cnt, nullptr) == BAD; }
};

static void scaled_project() {
  { Sp s; s.a = NUL; EXPECT(s.rejected()); }
  { Sp s; s.sc = NUL; EXPECT(s.rejected()); }
  { Sp s; s.wt = NUL; EXPECT(s.rejected()); }
  { Sp s; s.bias = NUL; EXPECT(s.rejected()); }
  { Sp s; s.out = NUL; EXPECT(s.rejected()); }
  { Sp s; s.a = A4; EXPECT(s.rejected()); }
  { Sp s; s.sc = A4; EXPECT(s.rejected()); }
  { Sp s; s.wt = A4; EXPECT(s.rejected()); }
  { Sp s; s.bias = A4; EXPECT(s.rejected()); }
  { Sp s; s.res = A4; EXPECT(s.rejected()); }
  { Sp s; s.out = A4; EXPECT(s.rejected()); }
  for (int w : {0, -4, 2, 30, MAXI, MAX4}) {
    { Sp s; s.C = w; EXPECT(s.rejected()); }
    { Sp s; s.Co = w; EXPECT(s.rejected()); }
  }
  { Sp s; s.N = 0, s.B = 0; EXPECT(s.rejected()); }
  { Sp s; s.N = -147, s.B = -3; EXPECT(s.rejected()); }
  { Sp s; s.N = 0; EXPECT(s.rejected()); }
  { Sp s; s.cnt = 0; EXPECT(s.rejected()); }
  { Sp s; s.cnt = -1; EXPECT(s.rejected()); }
  { Sp s; s.HW = 0; EXPECT(s.rejected()); }
  { Sp s; s.HW = -49, s.B = -3; EXPECT(s.rejected()); }  // B * HW == N with both negative
  { Sp s; s.HW = 50; EXPECT(s.rejected()); }
  { Sp s; s.B = 2; EXPECT(s.rejected()); }
  { Sp s; s.N = 148; EXPECT(s.rejected()); }
  { Sp s; s.B = s.HW = 65537, s.N = 131073; EXPECT(s.rejected()); }  // B * HW = 2^32 + N: no 32-bit wrap
  // operands of exactly 2^31 bytes, one at a time
  { Sp s; s.N = s.B = 1 << 19, s.HW = 1, s.C = 1024, s.Co = 4, s.cnt = 1; EXPECT(s.rejected()); }        // a
  { Sp s; s.N = s.B = 4, s.HW = 1, s.C = 1 << 15, s.Co = 1 << 14, s.cnt = 1; EXPECT(s.rejected()); }     // wt
  { Sp s; s.N = 1 << 24, s.B = 1 << 12, s.HW = 1 << 12, s.C = 4, s.Co = 32, s.cnt = 1; EXPECT(s.rejected()); }  // res, out
  { Sp s; s.N = s.B = 64, s.HW = 1, s.C = 64, s.Co = 4, s.cnt = 1 << 17; EXPECT(s.rejected()); }         // the sc stack
  { Sp s; s.N = s.B = 64, s.HW = 1, s.C = 4, s.Co = 64, s.cnt = 1 << 17; EXPECT(s.rejected()); }         // bias (and out)
  { Sp s; s.N = 1 << 19, s.B = 1 << 10, s.HW = 1 << 9, s.C = 4, s.Co = 32, s.cnt = 32; EXPECT(s.rejected()); }  // the out stack
  // INT_MAX in every integer slot, singly and together
  { Sp s; s.N = MAXI; EXPECT(s.rejected()); }
  { Sp s; s.N = s.B = MAXI, s.HW = 1; EXPECT(s.rejected()); }
  { Sp s; s.N = s.HW = MAXI, s.B = 1; EXPECT(s.rejected()); }
  { Sp s; s.B = MAXI; EXPECT(s.rejected()); }
  { Sp s; s.HW = MAXI; EXPECT(s.rejected()); }
  { Sp s; s.cnt = MAXI; EXPECT(s.rejected()); }
  { Sp s; s.N = s.B = s.HW = s.cnt = MAXI, s.C = s.Co = MAX4; EXPECT(s.rejected()); }
  { Sp s; s.N = s.B = (1 << 29) - 1, s.HW = 1, s.C = s.Co = (1 << 29) - 4, s.cnt = (1 << 29) - 1; EXPECT(s.rejected()); }
  { Sp s; s.N = s.B = 4, s.HW = 1, s.C = s.Co = 4, s.cnt = (1 << 29) - 1; EXPECT(s.rejected()); }
}

// ------------------------------------------------------------------ tp_silu_project_fwd
struct Fw {  // 3 images of 65 rows, 36 -> 24 channels, with res and apoz
  const float *z = A16, *wt = A16, *scale = A16, *shift = A16, *res = A16;
  float *out = A16, *apoz = A16;
  int N = 195, C = 36, Co = 24, B = 3, HW = 65;
  bool rejected() const { return tp_silu_project_fwd(z, wt, scale, shift, res, out, apoz, N, C, Co, B, HW, nullptr) == BAD; }
};

static void silu_project_fwd() {
  { Fw s; s.z = NUL; EXPECT(s.rejected()); }
  { Fw s; s.wt = NUL; EXPECT(s.rejected()); }
  { Fw s; s.scale = NUL; EXPECT(s.rejected()); }
  { Fw s; s.shift = NUL; EXPECT(s.rejected()); }
  { Fw s; s.out = NUL; EXPECT(s.rejected()); }
  { Fw s; s.z = A4; EXPECT(s.rejected()); }
  { Fw s; s.wt = A4; EXPECT(s.rejected()); }
  { Fw s; s.scale = A4; EXPECT(s.rejected()); }
  { Fw s; s.shift = A4; EXPECT(s.rejected()); }
  { Fw s; s.res = A4; EXPECT(s.rejected()); }
  { Fw s; s.out = A4; EXPECT(s.rejected()); }
  { Fw s; s.apoz = A4; EXPECT(s.rejected()); }
  for (int w : {0, -4, 2, 30, MAXI, MAX4}) {
    { Fw s; s.C = w; EXPECT(s.rejected()); }
    { Fw s; s.Co = w; EXPECT(s.rejected()); }
  }
  { Fw s; s.Co = 132; EXPECT(s.rejected()); }
  { Fw s; s.N = 0, s.B = 0; EXPECT(s.rejected()); }
  { Fw s; s.N = -195, s.B = -3; EXPECT(s.rejected()); }
  { Fw s; s.HW = 0; EXPECT(s.rejected()); }
  { Fw s; s.HW = -65, s.B = -3; EXPECT(s.rejected()); }
  { Fw s; s.HW = 64; EXPECT(s.rejected()); }
  { Fw s; s.B = 4; EXPECT(s.rejected()); }
  { Fw s; s.N = 196; EXPECT(s.rejected()); }
  { Fw s; s.B = s.HW = 65537, s.N = 131073; EXPECT(s.rejected()); }  // B * HW = 2^32 + N: no 32-bit wrap
  { Fw s; s.N = s.B = 1 << 19, s.HW = 1, s.C = 1024, s.Co = 4; EXPECT(s.rejected()); }    // z
  { Fw s; s.N = s.B = 4, s.HW = 1, s.C = 1 << 22, s.Co = 128; EXPECT(s.rejected()); }     // wt
  { Fw s; s.N = s.B = 1 << 22, s.HW = 1, s.C = 4, s.Co = 128; EXPECT(s.rejected()); }     // res, out
  { Fw s; s.N = MAXI; EXPECT(s.rejected()); }
  { Fw s; s.N = s.B = MAXI, s.HW = 1; EXPECT(s.rejected()); }
  { Fw s; s.N = s.HW = MAXI, s.B = 1; EXPECT(s.rejected()); }
  { Fw s; s.B = MAXI; EXPECT(s.rejected()); }
  { Fw s; s.HW = MAXI; EXPECT(s.rejected()); }
  { Fw s; s.N = s.B = s.HW = MAXI, s.C = s.Co = MAX4; EXPECT(s.rejected()); }
  { Fw s; s.N = s.B = MAXI, s.HW = 1, s.C = MAX4, s.Co = 128; EXPECT(s.rejected()); }
}

// ------------------------------------------------------------------ tp_silu_project_dgrad
struct Dg {  // 3 images of 65 rows (2 slots), 24 -> 36 channels, Sensitivity slab
  const float *g = A16, *wtT = A16, *z = A16;
  float *dz = A16, *tay = A16;
  int R = 2, mode = 1, N = 195, C = 36, Co = 24, B = 3, HW = 65;
  bool rejected() const { return tp_silu_project_dgrad(g, wtT, z, dz, tay, R, mode, N, C, Co, B, HW, nullptr) == BAD; }
};

static void silu_project_dgrad() {
  EXPECT(tp_silu_project_tay_slots(65, 36) == 2);  // what Dg assumes
  { Dg s; s.g = NUL; EXPECT(s.rejected()); }
  { Dg s; s.wtT = NUL; EXPECT(s.rejected()); }
  { Dg s; s.z = NUL; EXPECT(s.rejected()); }
  { Dg s; s.dz = NUL; EXPECT(s.rejected()); }
  { Dg s; s.g = A4; EXPECT(s.rejected()); }
  { Dg s; s.wtT = A4; EXPECT(s.rejected()); }
  { Dg s; s.z = A4; EXPECT(s.rejected()); }
  { Dg s; s.dz = A4; EXPECT(s.rejected()); }
  { Dg s; s.tay = A4; EXPECT(s.rejected()); }
  for (int w : {0, -4, 2, 30, MAXI, MAX4}) {
    { Dg s; s.C = w; EXPECT(s.rejected()); }
    { Dg s; s.Co = w; EXPECT(s.rejected()); }
  }
  { Dg s; s.N = 0, s.B = 0; EXPECT(s.rejected()); }
  { Dg s; s.N = -195, s.B = -3; EXPECT(s.rejected()); }
  { Dg s; s.HW = 0; EXPECT(s.rejected()); }
  { Dg s; s.HW = -65, s.B = -3; EXPECT(s.rejected()); }
  { Dg s; s.HW = 64, s.R = 1; EXPECT(s.rejected()); }  // R right for the wrong HW: B * HW != N
  { Dg s; s.B = 4; EXPECT(s.rejected()); }
  { Dg s; s.B = s.HW = 65537, s.N = 131073, s.R = tp_silu_project_tay_slots(65537, 36); EXPECT(s.rejected()); }
  { Dg s; s.mode = -1; EXPECT(s.rejected()); }
  { Dg s; s.mode = 2; EXPECT(s.rejected()); }
  { Dg s; s.mode = MAXI; EXPECT(s.rejected()); }
  { Dg s; s.R = 1; EXPECT(s.rejected()); }
  { Dg s; s.R = 3; EXPECT(s.rejected()); }
  { Dg s; s.R = 0; EXPECT(s.rejected()); }
  { Dg s; s.R = -2; EXPECT(s.rejected()); }
  { Dg s; s.R = MAXI; EXPECT(s.rejected()); }
  { Dg s; s.N = 192, s.HW = 64, s.R = 2; EXPECT(s.rejected()); }  // 64 divides HW: one slot, not two
  { Dg s; s.N = 192, s.HW = 64, s.R = 0; EXPECT(s.rejected()); }
  { Dg s; s.N = s.B = 1 << 19, s.HW = 1, s.R = 1, s.C = 1024, s.Co = 4; EXPECT(s.rejected()); }        // z, dz, tay
  { Dg s; s.N = s.B = 4, s.HW = 1, s.R = 1, s.C = 1 << 15, s.Co = 1 << 14; EXPECT(s.rejected()); }     // wtT
  { Dg s; s.N = s.B = 1 << 19, s.HW = 1, s.R = 1, s.C = 4, s.Co = 1024; EXPECT(s.rejected()); }        // g
  { Dg s; s.N = MAXI; EXPECT(s.rejected()); }
  { Dg s; s.N = s.B = MAXI, s.HW = 1, s.R = 1; EXPECT(s.rejected()); }
  { Dg s; s.N = s.HW = MAXI, s.B = 1, s.R = tp_silu_project_tay_slots(MAXI, 36); EXPECT(s.rejected()); }
  { Dg s; s.B = MAXI; EXPECT(s.rejected()); }
  { Dg s; s.HW = MAXI; EXPECT(s.rejected()); }
  { Dg s; s.N = s.B = s.HW = s.R = s.mode = MAXI, s.C = s.Co = MAX4; EXPECT(s.rejected()); }
}

// ------------------------------------------------------------------ tp_silu_project_tay_slots
static void tay_slots() {
  EXPECT(tp_silu_project_tay_slots(0, 8) == 0 && tp_silu_project_tay_slots(-64, 8) == 0);
  EXPECT(tp_silu_project_tay_slots(64, 0) == 0 && tp_silu_project_tay_slots(64, -8) == 0);
  EXPECT(tp_silu_project_tay_slots(64, 2) == 0 && tp_silu_project_tay_slots(64, 30) == 0);
  EXPECT(tp_silu_project_tay_slots(64, MAXI) == 0);
  EXPECT(tp_silu_project_tay_slots(MAXI, MAX4) == (1 << 25) + 1);  // no overflow: (2^31 - 1 - 1 + 63) / 64 + 1
  EXPECT(tp_silu_project_tay_slots(1 << 30, 4) == 1 << 24);
  // the 64-row tiles image b of HW rows meets, rows b HW .. (b + 1) HW - 1; b HW mod 64 has a period of at most 64
  for (int HW = 1; HW <= 300; ++HW) {
    int most = 0;
    for (int b = 0; b < 64; ++b) {
      const int tiles = ((b + 1) * HW - 1) / 64 - (b * HW) / 64 + 1;
      most = tiles > most ? tiles : most;
    }
    for (int C : {4, 64, 132}) {
      const int r = tp_silu_project_tay_slots(HW, C);
      if (r != most) std::fprintf(stderr, "tay_slots(%d, %d) = %d, an image meets %d tiles\n", HW, C, r, most);
      EXPECT(r == most);
    }
  }
}

// ------------------------------------------------------------------ tp_silu_prefix_project
struct Xp {  // 50 rows, 64 -> 32 channels, a permutation of 57 real channels, prefixes 1 .. 7
  const float *z = A16, *wt = A16, *shift = A16, *res = A16;
  const int *perm = P4, *rank = P16;
  float* out = A16;
  int N = 50, C = 64, Co = 32, n = 57, p0 = 1, cnt = 7;
  bool rejected() const { return tp_silu_prefix_project(z, wt, shift, res, perm, rank, out, N, C, Co, n, p0, cnt, nullptr) == BAD; }
};

static bool xp_range(int n, int p0, int cnt) {
  Xp s;
  s.n = n, s.p0 = p0, s.cnt = cnt;
  return s.rejected();
}

static void silu_prefix_project() {
  { Xp s; s.z = NUL; EXPECT(s.rejected()); }
  { Xp s; s.wt = NUL; EXPECT(s.rejected()); }
  { Xp s; s.shift = NUL; EXPECT(s.rejected()); }
  { Xp s; s.perm = nullptr; EXPECT(s.rejected()); }
  { Xp s; s.rank = nullptr; EXPECT(s.rejected()); }
  { Xp s; s.out = NUL; EXPECT(s.rejected()); }
  { Xp s; s.z = A4; EXPECT(s.rejected()); }
  { Xp s; s.wt = A4; EXPECT(s.rejected()); }
  { Xp s; s.shift = A4; EXPECT(s.rejected()); }
  { Xp s; s.res = A4; EXPECT(s.rejected()); }
  { Xp s; s.rank = P4; EXPECT(s.rejected()); }
  { Xp s; s.out = A4; EXPECT(s.rejected()); }
  { Xp s; s.perm = P2; EXPECT(s.rejected()); }
  for (int w : {0, -4, 2, 30, MAXI, MAX4}) {
    { Xp s; s.C = w, s.n = 0, s.p0 = 0, s.cnt = 1; EXPECT(s.rejected()); }  // n <= C whatever C is
    { Xp s; s.Co = w; EXPECT(s.rejected()); }
  }
  { Xp s; s.Co = 132; EXPECT(s.rejected()); }
  { Xp s; s.N = 0; EXPECT(s.rejected()); }
  { Xp s; s.N = -3; EXPECT(s.rejected()); }
  // the prefix range: cnt < 1, p0 < 0, p0 + cnt - 1 > n, n > C, n < 0 (and sums that overflow 32 bits)
  EXPECT(xp_range(57, 0, 0));
  EXPECT(xp_range(57, 0, -1));
  EXPECT(xp_range(57, -1, 2));
  EXPECT(xp_range(57, 0, 59));   // 0 + 59 - 1 = 58 > 57
  EXPECT(xp_range(57, 57, 2));   // 57 + 2 - 1 = 58 > 57
  EXPECT(xp_range(57, 58, 1));
  EXPECT(xp_range(57, MAXI, 2));
  EXPECT(xp_range(57, 2, MAXI));
  EXPECT(xp_range(57, MAXI, MAXI));
  EXPECT(xp_range(65, 0, 2));    // n > C
  EXPECT(xp_range(MAXI, 0, 2));
  EXPECT(xp_range(-1, 0, 1));
  EXPECT(xp_range(-1, 0, 0));
  // operands of exactly 2^31 bytes
  { Xp s; s.N = 1 << 19, s.C = 1024, s.Co = 4; EXPECT(s.rejected()); }                 // z
  { Xp s; s.N = 4, s.C = 1 << 22, s.Co = 128; EXPECT(s.rejected()); }                  // wt
  { Xp s; s.N = 1 << 22, s.C = 64, s.Co = 128, s.cnt = 1; EXPECT(s.rejected()); }      // res, one copy of out
  { Xp s; s.N = 1 << 19, s.Co = 32, s.n = 57, s.p0 = 0, s.cnt = 32; EXPECT(s.rejected()); }  // the out stack
  { Xp s; s.N = MAXI; EXPECT(s.rejected()); }
  { Xp s; s.N = s.n = s.p0 = s.cnt = MAXI, s.C = s.Co = MAX4; EXPECT(s.rejected()); }
  { Xp s; s.N = MAXI, s.C = MAX4, s.n = MAX4, s.p0 = 0, s.cnt = MAX4 + 1, s.Co = 128; EXPECT(s.rejected()); }
  { Xp s; s.N = (1 << 29) - 1, s.C = 4, s.n = 4, s.p0 = 0, s.cnt = 5, s.Co = 128; EXPECT(s.rejected()); }
}

int main() {
  scaled_project();
  silu_project_fwd();
  silu_project_dgrad();
  tay_slots();
  silu_prefix_project();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("project_gemm validation ok\n");
  return 0;
}
