// Torch-side helpers of the two binding files (bindings.cpp, engine_bindings.cpp): the stream, the launch
// check and the operand checks that every op repeats. Written once here so that the copies cannot drift;
// no kernel file includes this header (kernels see no torch types).
//
// ``like`` is the operand the op's device guard is set from: every other operand must live on its device.
#pragma once
#include <torch/library.h>
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

#include <tuple>

#include "tp_launchers.h"

inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

#define TP_CHECK_HIP(expr)                                                                \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    TORCH_CHECK(_e == hipSuccess, "tpamd kernel launch failed: ", hipGetErrorString(_e)); \
  } while (0)

using OptTensor = c10::optional<at::Tensor>;

inline bool present(const OptTensor& t) { return t.has_value() && t->defined(); }

inline float* ptr_or_null(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

constexpr int64_t kAnyDims = -1;    // contiguous, any number of dims
constexpr int64_t kAnyLayout = -2;  // dtype and device only: the op copies the operand or reads its strides

// A float32 GPU operand; dim >= 0 or kAnyDims: contiguous too (with that many dims).
inline void need(const at::Tensor& t, const char* name, int64_t dim = kAnyLayout, const at::Tensor* like = nullptr) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32, got ", t.scalar_type());
  TORCH_CHECK(like == nullptr || t.device() == like->device(), name, " must be on the device of the other operands");
  if (dim == kAnyLayout) return;
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(dim < 0 || t.dim() == dim, name, " must have ", dim, " dims, got ", t.dim());
}

// An operand its kernels read as float4 (a view at an odd storage offset is not).
inline void need_aligned16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

// Nullable vector of exactly n elements (a short one would be read out of bounds).
inline float* vec_ptr(const OptTensor& t, int64_t n, const char* name, const at::Tensor& like) {
  if (!present(t)) return nullptr;
  need(*t, name, 1, &like);
  TORCH_CHECK(t->numel() == n, name, " must have ", n, " elements");
  return t->data_ptr<float>();
}

// Nullable per-channel vector of a conv / BN epilogue.
inline const float* opt_ptr(const OptTensor& t, int64_t n, const char* name, const at::Tensor& like) {
  const float* p = vec_ptr(t, n, name, like);
  // the epilogues read per-channel vectors as float4
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, name, " must be 16-byte aligned");
  return p;
}

// Nullable (B, H, W, C) NHWC operand of an epilogue: a residual, a mask, a BN input.
inline const float* nhwc_ptr(const OptTensor& t, const char* name, int64_t B, int64_t H, int64_t W, int64_t C,
                             const at::Tensor& like) {
  if (!present(t)) return nullptr;
  need(*t, name, 4, &like);
  TORCH_CHECK(t->size(0) == B && t->size(1) == H && t->size(2) == W && t->size(3) == C, name, " must be (", B, ", ", H,
              ", ", W, ", ", C, "), got ", t->sizes());
  return t->data_ptr<float>();
}

// Nullable residual of a (B, H, W, C) output, added at every s-th pixel: (B, ceil(H/s), ceil(W/s), C).
inline const float* res_ptr(const OptTensor& res, int64_t B, int64_t H, int64_t W, int64_t C, int64_t s,
                            const at::Tensor& like) {
  TORCH_CHECK(s >= 1, "res_stride must be >= 1");
  return nhwc_ptr(res, "res", B, (H + s - 1) / s, (W + s - 1) / s, C, like);
}

// Nullable operand of ``like``'s own shape.
inline const float* same_shape_ptr(const OptTensor& t, const char* name, const at::Tensor& like) {
  if (!present(t)) return nullptr;
  need(*t, name, kAnyDims, &like);
  TORCH_CHECK(t->sizes() == like.sizes(), name, " must have the shape ", like.sizes());
  return t->data_ptr<float>();
}

// (B, C) counts of positive outputs, accumulated by a forward epilogue (nullable).
inline float* count_ptr(const OptTensor& apoz, int64_t B, int64_t C, const at::Tensor& like) {
  if (!present(apoz)) return nullptr;
  need(*apoz, "apoz", kAnyDims, &like);
  TORCH_CHECK(apoz->numel() == B * C, "apoz must be a contiguous float32 (B, C) = (", B, ", ", C, ") tensor");
  return apoz->data_ptr<float>();
}

// Taylor / Sensitivity partial slab (R', B, C), accumulated by a backward epilogue (nullable): whole slots,
// exactly R of them or (kernels that fold into the first R) at least R.
inline float* taylor_ptr(const OptTensor& t, int64_t R, bool exact, int64_t B, int64_t C, const at::Tensor& like) {
  if (!present(t)) return nullptr;
  need(*t, "taylor", kAnyDims, &like);
  const int64_t slot = B * C, n = t->numel();
  TORCH_CHECK(slot > 0 && n % slot == 0 && (exact ? n == R * slot : n >= R * slot),
              "taylor must be a contiguous float32 (R, B, C) GPU tensor of (", B, ", ", C, ") partial slots with R ",
              exact ? "= " : ">= ", R);
  return t->data_ptr<float>();
}

// Tay_mode of a backward epilogue: 0 Taylor, 1 Sensitivity, (max_mode 2) 2 Sensitivity masked by act > 0.
inline int tay_mode_arg(int64_t tay_mode, int64_t max_mode) {
  TORCH_CHECK(tay_mode >= 0 && tay_mode <= max_mode, "bad tay_mode ", tay_mode, " (0 .. ", max_mode, ")");
  return (int)tay_mode;
}

// The uint8 argmax bytes of a max-pool, one per element of ``like`` (on its device: the kernels
// dereference the pointer).
inline const uint8_t* argmax_ptr(const at::Tensor& am, const char* name, const at::Tensor& like) {
  TORCH_CHECK(am.is_cuda() && am.device() == like.device() && am.scalar_type() == at::kByte && am.is_contiguous() &&
                  am.sizes() == like.sizes(), name, " must be contiguous uint8 argmax bytes ", like.sizes(),
              " on the device of the other operands");
  return am.data_ptr<uint8_t>();
}

// Gradient g of a (B, H, W, .) activation: at full resolution, or with g_argmax the 2x2-pooled gradient whose
// full-resolution form the argmax bytes imply. Returns the bytes (null: not pooled).
inline const uint8_t* pooled_grad(const at::Tensor& g, const OptTensor& g_argmax, int64_t B, int64_t H, int64_t W) {
  TORCH_CHECK(g.size(0) == B, "batch mismatch");
  if (!present(g_argmax)) {
    TORCH_CHECK(g.size(1) == H && g.size(2) == W, "grad shape mismatch");
    return nullptr;
  }
  TORCH_CHECK(g.size(1) * 2 == H && g.size(2) * 2 == W, "pooled grad shape mismatch");
  return argmax_ptr(*g_argmax, "g_argmax", g);
}

// ReLU bit mask of ``elems`` elements, 4 per byte (nullable).
inline const uint8_t* bit_mask_ptr(const OptTensor& t, int64_t elems, const at::Tensor& like, const char* what) {
  if (!present(t)) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kByte && t->is_contiguous() && t->numel() == (elems + 3) / 4 &&
                  t->device() == like.device(),
              what, " must be a ReLU bit mask of ceil(elements / 4) uint8 on the device");
  return t->data_ptr<uint8_t>();
}

// A BatchNorm module's num_batches_tracked, incremented by the finalize kernel (nullable).
inline long long* counter_ptr(const OptTensor& t, const at::Tensor& like) {
  if (!present(t)) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->numel() == 1 && t->device() == like.device(),
              "num_batches must be a one-element int64 GPU tensor");
  return reinterpret_cast<long long*>(t->data_ptr<int64_t>());
}

// The (2, C) rows a, b of a fused BN forward (unit stride along C; float4 reads when C % 4 == 0).
inline std::tuple<const float*, const float*> affine_rows(const at::Tensor& ab, int64_t C, const at::Tensor& like) {
  need(ab, "ab", kAnyLayout, &like);
  TORCH_CHECK(ab.dim() == 2 && ab.size(0) == 2 && ab.size(1) == C, "ab must be (2, ", C, "), got ", ab.sizes());
  TORCH_CHECK(ab.stride(1) == 1 && ab.stride(0) >= C, "ab: rows of unit stride");
  const float* a = ab.data_ptr<float>();
  const float* b = a + ab.stride(0);
  TORCH_CHECK(C % 4 != 0 || (reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0),
              "ab rows must be 16-byte aligned");
  return {a, b};
}

// Output (B, H, W, K) of a forward conv on x, or with ``pool`` the 2x2-pooled output + its argmax bytes.
inline std::tuple<at::Tensor, at::Tensor> conv_out(const at::Tensor& x, int64_t B, int64_t H, int64_t W, int64_t K,
                                                   bool pool) {
  if (!pool) return {at::empty({B, H, W, K}, x.options()), at::Tensor()};
  return {at::empty({B, H / 2, W / 2, K}, x.options()), at::empty({B, H / 2, W / 2, K}, x.options().dtype(at::kByte))};
}

// Parameter-shaped gradient output (Cout_r <= Cout, Cin_r <= Cin, ks, ks), written through its own strides
// (real channels only). Positive strides: with a zero stride (an expanded tensor) the kernel's writes overlap.
struct ParamOut {
  float* p = nullptr;
  int co = 0, ci = 0;
  long long fs[4] = {0, 0, 0, 0};
};
inline ParamOut param_out(const at::Tensor& o, int64_t Cout, int64_t Cin, int64_t ks, const at::Tensor& like) {
  need(o, "out", kAnyLayout, &like);
  TORCH_CHECK(o.dim() == 4 && o.size(0) > 0 && o.size(0) <= Cout && o.size(1) > 0 && o.size(1) <= Cin &&
                  o.size(2) == ks && o.size(3) == ks, "out must be (Cout_r <= Cout, Cin_r <= Cin, ks, ks)");
  TORCH_CHECK(o.stride(0) > 0 && o.stride(1) > 0 && o.stride(2) > 0 && o.stride(3) > 0, "out: positive strides only");
  ParamOut r;
  r.p = o.data_ptr<float>();
  r.co = (int)o.size(0);
  r.ci = (int)o.size(1);
  for (int i = 0; i < 4; ++i) r.fs[i] = o.stride(i);
  return r;
}

// The launchers' split normalisation over ``units`` K steps: no more splits than units, none of them empty.
inline int64_t norm_splits(int64_t splits, int64_t units) {
  if (units < 1) return 1;
  splits = std::max<int64_t>(1, std::min<int64_t>(splits, units));
  const int64_t per = (units + splits - 1) / splits;
  return (units + per - 1) / per;
}

// Split-K workspace: sp slabs of ``elems`` floats (undefined for one K pass).
inline at::Tensor splitk_ws(int64_t sp, int64_t elems, const at::Tensor& like) {
  return sp > 1 ? at::empty({sp * elems}, like.options()) : at::Tensor();
}

// A GEN conv launch whose cfg may carry the stream-K flag (32): its fixup workspace and the cfg to launch
// with. The flag is stripped when stream-K does not apply to the op (``applies``: one K pass, GEN 1) or at
// this shape (the launcher then runs the data-parallel grid).
constexpr int64_t kCfgSK = 32;
struct SkPlan {
  at::Tensor ws;
  int64_t cfg;
};
inline SkPlan sk_plan(bool applies, int64_t cfg, int64_t ks, bool tay, int64_t M, int64_t N, const at::Tensor& like) {
  if (cfg < 0 || !(cfg & kCfgSK)) return {at::Tensor(), cfg};
  const long long n = applies ? tp_conv_sk_ws_floats((int)(cfg & ~kCfgSK), (int)ks, 0, tay ? 1 : 0, (int)M, (int)N) : 0;
  if (n > 0) return {at::empty({(int64_t)n}, like.options()), cfg};
  return {at::Tensor(), cfg & ~kCfgSK};
}
