// torch.ops.tpamd.* registrations of the engine kernels: the implicit-GEMM, GEN and first-layer convs and the
// Shapley prefix GEMM (conv_mfma.hip), the 2x2-map conv (conv2x2_fast.hip), Winograd F(2x2) / F(4x4)
// (winograd.hip, wino4.hip), the weight gradients (conv_wgrad.hip, wino_wgrad.hip), weight packing
// (weight_pack.hip), training BatchNorm (batchnorm.hip) and the NHWC pools (prune_ops.hip). The operand
// checks shared by these ops are in tp_bind.h.
#include "tp_bind.h"

namespace {

enum { EPI_FWD = 0, EPI_FWD_POOL = 1, EPI_BWD = 2 };

void check_igemm_cfg(int64_t cfg, int64_t ks) {
  TORCH_CHECK((cfg >= 0 && cfg <= 6) || (ks == 3 && (cfg == 256 || cfg == 258 || cfg == 259)),
              "bad tile config (bf16 operands: 256 + {0, 2, 3}, 3x3 only)");
}

// Forward conv / linear: x (B,H,W,Cin) NHWC, w (Cout, K) with K = ks*ks*Cin.
// Returns out (B,H,W,Cout) or pooled (B,H/2,W/2,Cout) + argmax bytes.
std::tuple<at::Tensor, at::Tensor> conv_fwd(const at::Tensor& x, const at::Tensor& w, const OptTensor& scale,
                                            const OptTensor& shift, bool relu, bool pool, int64_t ks, int64_t cfg,
                                            int64_t splits, const OptTensor& apoz, double slope) {
  need(x, "x", 4);
  need(w, "w", 2, &x);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3), Cout = w.size(0);
  TORCH_CHECK(ks == 1 || ks == 3, "ks must be 1 or 3");
  TORCH_CHECK(w.size(1) == ks * ks * Cin, "weight K mismatch: ", w.size(1), " vs ", ks * ks * Cin);
  TORCH_CHECK(Cin % 32 == 0, "Cin must be a multiple of 32");
  TORCH_CHECK(!pool || (H % 2 == 0 && W % 2 == 0), "pooling needs even H, W");
  check_igemm_cfg(cfg, ks);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* sc = opt_ptr(scale, Cout, "scale", x);
  const float* sh = opt_ptr(shift, Cout, "shift", x);
  auto [out, am] = conv_out(x, B, H, W, Cout, pool);
  const int64_t sp = norm_splits(splits, ks * ks * Cin / 32);
  at::Tensor ws = splitk_ws(sp, B * H * W * Cout, x);
  float* ap = count_ptr(apoz, B, Cout, x);  // counts of positive (pre-pool) outputs
  TP_CHECK_HIP(tp_conv_igemm(x.data_ptr<float>(), nullptr, w.data_ptr<float>(), (int)B, (int)H, (int)W, (int)Cin,
                             (int)Cout, (int)ks, pool ? 1 : 0, 0, pool ? EPI_FWD_POOL : EPI_FWD, (int)cfg, (int)sp, sc,
                             sh, relu ? 1 : 0, out.data_ptr<float>(), pool ? am.data_ptr<uint8_t>() : nullptr, nullptr,
                             nullptr, (int)(H * W), 0, ptr_or_null(ws), 0, ap, (float)slope, cur_stream()));
  return {out, am};
}

// dgrad + fused consumer epilogue.
// g: grad w.r.t. the conv output, (B,H,W,Cout); or, with g_argmax, the masked grad at pooled
//    resolution (B,H/2,W/2,Cout) whose full-resolution form is implied by the argmax bytes.
// wt: flipped/transposed weight (Cin, ks*ks*Cout). act: activation at the conv input (B,H,W,Cin).
// taylor (B,Cin) fp32 accumulated atomically with sum_hw -(dL/dact * act) (nullable).
// Returns dL/d(pre-activation) * bn_scale masked by act>0 (B,H,W,Cin), or an empty tensor.
at::Tensor conv_dgrad(const at::Tensor& g, const OptTensor& g_argmax, const at::Tensor& wt, const at::Tensor& act,
                      const OptTensor& bn_scale, const OptTensor& taylor, bool want_out, int64_t ks, int64_t cfg,
                      int64_t splits, int64_t tay_group, int64_t tay_mode, double slope) {
  need(g, "g", 4);
  need(wt, "wt", 2, &g);
  need(act, "act", 4, &g);
  const int64_t B = act.size(0), H = act.size(1), W = act.size(2), Cin = act.size(3);
  const int64_t Cout = g.size(3);
  const uint8_t* am = pooled_grad(g, g_argmax, B, H, W);
  TORCH_CHECK(wt.size(0) == Cin && wt.size(1) == ks * ks * Cout, "wt must be (Cin, ks*ks*Cout)");
  TORCH_CHECK(Cout % 32 == 0, "Cout must be a multiple of 32 for dgrad");
  TORCH_CHECK(tay_group >= 0 && (tay_group == 0 || Cin % tay_group == 0), "tay_group must divide Cin");
  check_igemm_cfg(cfg, ks);
  const int tm = tay_mode_arg(tay_mode, 2);  // the launcher passes it on unchecked
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const float* sc = opt_ptr(bn_scale, Cin, "bn_scale", g);
  float* tay = taylor_ptr(taylor, 1, false, B, Cin, g);  // (B, Cin) or (R, B, Cin): slot 0 is written
  at::Tensor out;
  if (want_out) out = at::empty({B, H, W, Cin}, g.options());
  const int64_t sp = norm_splits(splits, ks * ks * Cout / 32);
  at::Tensor ws = splitk_ws(sp, B * H * W * Cin, g);
  TP_CHECK_HIP(tp_conv_igemm(g.data_ptr<float>(), am, wt.data_ptr<float>(), (int)B, (int)H, (int)W, (int)Cout,
                             (int)Cin, (int)ks, 0, am ? 1 : 0, EPI_BWD, (int)cfg, (int)sp, sc, nullptr, 0,
                             ptr_or_null(out), nullptr, act.data_ptr<float>(), tay, (int)(H * W), (int)tay_group,
                             ptr_or_null(ws), tm, nullptr, (float)slope, cur_stream()));
  return out;
}

// 3x3 / pad-1 conv on 2x2 maps as 9 channel products (conv2x2_fast.hip). x (B,2,2,C); u9 (9,K,C) =
// G w G^T. Returns out (B,2,2,K), or pooled (B,1,1,K) + argmax bytes.
std::tuple<at::Tensor, at::Tensor> conv2x2_fast_fwd(const at::Tensor& x, const at::Tensor& u9, const OptTensor& scale,
                                                    const OptTensor& shift, bool relu, bool pool, int64_t cfg,
                                                    int64_t splits) {
  need(x, "x", 4);
  need(u9, "u9", 3, &x);
  const int64_t B = x.size(0), C = x.size(3), K = u9.size(1);
  TORCH_CHECK(x.size(1) == 2 && x.size(2) == 2, "x must be (B, 2, 2, C)");
  TORCH_CHECK(u9.size(0) == 9 && u9.size(2) == C, "u9 must be (9, K, C)");
  TORCH_CHECK(B > 0 && C % 32 == 0 && K % 4 == 0, "C must be a multiple of 32 and K of 4");
  TORCH_CHECK(cfg >= 0 && cfg <= 6, "bad tile config");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* sc = opt_ptr(scale, K, "scale", x);
  const float* sh = opt_ptr(shift, K, "shift", x);
  const int64_t sp = tp_conv_norm_splits((int)std::max<int64_t>(1, std::min<int64_t>(splits, 1 << 16)), (int)C);
  auto [out, am] = conv_out(x, B, 2, 2, K, pool);
  // workspaces from the caching allocator (capturable in a HIP graph, like the split-K slabs)
  at::Tensor V = at::empty({9, B, C}, x.options()), slabs = at::empty({9 * sp, B, K}, x.options());
  TP_CHECK_HIP(tp_conv2x2_fast_fwd(x.data_ptr<float>(), u9.data_ptr<float>(), (int)B, (int)C, (int)K, (int)cfg,
                                   (int)sp, sc, sh, relu ? 1 : 0, pool ? 1 : 0, out.data_ptr<float>(),
                                   pool ? am.data_ptr<uint8_t>() : nullptr, V.data_ptr<float>(),
                                   slabs.data_ptr<float>(), cur_stream()));
  return {out, am};
}

// Its data gradient with the conv_dgrad epilogue contract (tay_group = Cin: taylor is (4, B, Cin), one
// slot per pixel, accumulated). g (B,2,2,Cg), or the pooled (B,1,1,Cg) with g_argmax; u9t (9,Cin,Cg).
at::Tensor conv2x2_fast_dgrad(const at::Tensor& g, const OptTensor& g_argmax, const at::Tensor& u9t,
                              const at::Tensor& act, const OptTensor& bn_scale, const OptTensor& taylor, bool want_out,
                              int64_t cfg, int64_t splits, int64_t tay_mode) {
  need(g, "g", 4);
  need(u9t, "u9t", 3, &g);
  need(act, "act", 4, &g);
  const int64_t B = act.size(0), Cin = act.size(3), Cg = g.size(3);
  TORCH_CHECK(act.size(1) == 2 && act.size(2) == 2 && B > 0, "act must be a non-empty (B, 2, 2, Cin)");
  const uint8_t* am = pooled_grad(g, g_argmax, B, 2, 2);
  TORCH_CHECK(u9t.size(0) == 9 && u9t.size(1) == Cin && u9t.size(2) == Cg, "u9t must be (9, Cin, Cg)");
  TORCH_CHECK(Cg % 32 == 0 && Cin % 4 == 0, "Cg must be a multiple of 32 and Cin of 4");
  TORCH_CHECK(cfg >= 0 && cfg <= 6, "bad tile config");
  const int tm = tay_mode_arg(tay_mode, 2);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const float* sc = opt_ptr(bn_scale, Cin, "bn_scale", g);
  float* tay = taylor_ptr(taylor, 4, true, B, Cin, g);  // one slot per pixel
  TORCH_CHECK(want_out || tay, "nothing to compute: no output and no taylor slab");
  at::Tensor out;
  if (want_out) out = at::empty({B, 2, 2, Cin}, g.options());
  const int64_t sp = tp_conv_norm_splits((int)std::max<int64_t>(1, std::min<int64_t>(splits, 1 << 16)), (int)Cg);
  at::Tensor V = at::empty({9, B, Cg}, g.options()), slabs = at::empty({9 * sp, B, Cin}, g.options());
  TP_CHECK_HIP(tp_conv2x2_fast_dgrad(g.data_ptr<float>(), am, u9t.data_ptr<float>(), (int)B, (int)Cg, (int)Cin,
                                     (int)cfg, (int)sp, act.data_ptr<float>(), sc, tay, tm, ptr_or_null(out),
                                     V.data_ptr<float>(), slabs.data_ptr<float>(), cur_stream()));
  return out;
}

// First conv layer (tiny Cin) on the VALU: NCHW input -> NHWC output, BN affine + ReLU fused.
// ``wt``: optional tap-major copy of w, [Cin][3][3][Cout], packed once by the caller (the
// wave-uniform kernel's operand layout); built here per call when absent.
at::Tensor conv_first(const at::Tensor& x, const at::Tensor& w, const at::Tensor& scale, const at::Tensor& shift,
                      bool relu, const OptTensor& wt_packed) {
  need(x, "x", 4);
  need(w, "w", 4, &x);
  const int64_t B = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3), Cout = w.size(0);
  TORCH_CHECK(w.size(1) == Cin && w.size(2) == 3 && w.size(3) == 3, "w must be (Cout, Cin, 3, 3)");
  // one element per output channel of w (the engine pads the vectors with the weight)
  const float* sc = vec_ptr(scale, Cout, "scale", x);
  const float* sh = vec_ptr(shift, Cout, "shift", x);
  TORCH_CHECK(sc && sh, "scale and shift must be defined");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto out = at::empty({B, H, W, Cout}, x.options());
  if ((Cout == 16 || Cout == 32 || Cout == 64) && Cin <= 16) {  // wave-uniform weights (scalar loads)
    at::Tensor wt;
    if (present(wt_packed)) {
      wt = *wt_packed;
      need(wt, "wt", 4, &x);
      TORCH_CHECK(wt.size(0) == Cin && wt.size(1) == 3 && wt.size(2) == 3 && wt.size(3) == Cout,
                  "wt must be (Cin, 3, 3, Cout)");
    } else {
      wt = w.permute({1, 2, 3, 0}).contiguous();  // [Cin][3][3][Cout]
    }
    TP_CHECK_HIP(tp_conv_first_wave(x.data_ptr<float>(), wt.data_ptr<float>(), sc, sh, out.data_ptr<float>(), (int)B,
                                    (int)Cin, (int)H, (int)W, (int)Cout, relu ? 1 : 0, cur_stream()));
    return out;
  }
  TP_CHECK_HIP(tp_conv_first_direct(x.data_ptr<float>(), w.data_ptr<float>(), sc, sh, out.data_ptr<float>(), (int)B,
                                    (int)Cin, (int)H, (int)W, (int)Cout, relu ? 1 : 0, cur_stream()));
  return out;
}

// Winograd U images of a 3x3 weight: w (K, C, 3, 3) -> (C/8, K/32, 4096); flip_t: the data-gradient
// operand of the forward weight w (Cout = K', Cin = C', 3, 3) -> images of (C', K') with rotated taps.
// bf16: the bf16 images of the BF kernels (same shape, dtype bfloat16; opt-in compute_dtype).
at::Tensor wino_weights(const at::Tensor& w, bool flip_t, int64_t K, int64_t C, bool bf16) {
  need(w, "w", 4);
  TORCH_CHECK(w.size(2) == 3 && w.size(3) == 3, "w must be (.., .., 3, 3)");
  // K, C: the padded GEMM sizes (0 = the weight's own); the source may be narrower (zero padding)
  if (K <= 0) K = flip_t ? w.size(1) : w.size(0);
  if (C <= 0) C = flip_t ? w.size(0) : w.size(1);
  TORCH_CHECK(K % 32 == 0 && C % 8 == 0, "Winograd images need K % 32 == 0 and C % 8 == 0");
  TORCH_CHECK(flip_t ? (w.size(0) <= C && w.size(1) <= K) : (w.size(0) <= K && w.size(1) <= C),
              "weight wider than the padded GEMM");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(w.device());
  auto u = at::empty({C / 8, K / 32, 4096}, w.options().dtype(bf16 ? at::kBFloat16 : at::kFloat));
  if (bf16)
    TP_CHECK_HIP(tp_wino_weights_bf16(w.data_ptr<float>(), u.data_ptr(), (int)K, (int)C, flip_t ? 1 : 0,
                                      (int)w.size(0), (int)w.size(1), cur_stream()));
  else
    TP_CHECK_HIP(tp_wino_weights(w.data_ptr<float>(), u.data_ptr<float>(), (int)K, (int)C, flip_t ? 1 : 0,
                                 (int)w.size(0), (int)w.size(1), cur_stream()));
  return u;
}

// Conv weight (O, I, KS, KS) -> a zero-padded GEMM operand (rows, cols): mode 0 forward
// [n][(kh, kw, ci)], 1 stride-1 dgrad [ci][(kh, kw, co)] with flipped taps, 2 strided dgrad
// (natural taps); cpad = channel granule of the column index.
at::Tensor pack_conv_weight(const at::Tensor& w, int64_t rows, int64_t cols, int64_t cpad, int64_t mode) {
  need(w, "w", 4);
  TORCH_CHECK(w.size(2) == w.size(3), "square kernels only");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(w.device());
  auto out = at::empty({rows, cols}, w.options());
  TP_CHECK_HIP(tp_pack_conv_weight(w.data_ptr<float>(), out.data_ptr<float>(), (int)w.size(0), (int)w.size(1),
                                   (int)w.size(2), (int)rows, (int)cols, (int)cpad, (int)mode, cur_stream()));
  return out;
}

// Every operand of ``pack_conv_weight`` for a list of weights in one launch: outs[i] (rows, cols)
// <- ws[i] per cfg[4i:4i+4] = (rows, cols, cpad, mode). ws may be strided (channels_last
// parameters are read in place). The descriptors travel through pinned memory (async copy).
void pack_conv_weights_multi(const std::vector<at::Tensor>& ws, const std::vector<at::Tensor>& outs,
                             const std::vector<int64_t>& cfg) {
  constexpr int D = 14;
  const int64_t n = (int64_t)ws.size();
  TORCH_CHECK(n > 0 && (int64_t)outs.size() == n && (int64_t)cfg.size() == 4 * n,
              "pack_conv_weights_multi: ws, outs and 4 ints per operand");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ws[0].device());
  auto hd = at::empty({n * D}, at::TensorOptions().dtype(at::kLong).pinned_memory(true));
  int64_t* h = hd.data_ptr<int64_t>();
  int64_t total = 0;
  for (int64_t i = 0; i < n; ++i) {
    const at::Tensor& w = ws[i];
    const at::Tensor& o = outs[i];
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 4 && w.size(2) == w.size(3) &&
                    w.device() == ws[0].device(), "pack_conv_weights_multi: fp32 (O, I, KS, KS) GPU weights");
    const int64_t rows = cfg[4 * i], cols = cfg[4 * i + 1], cpad = cfg[4 * i + 2], mode = cfg[4 * i + 3];
    const int64_t O = w.size(0), I = w.size(1);
    TORCH_CHECK(mode >= 0 && mode <= 2 && rows > 0 && cols > 0 && cpad > 0 &&
                    (mode == 0 ? (rows >= O && cpad >= I) : (rows >= I && cpad >= O)),
                "pack_conv_weights_multi: bad operand shape");
    TORCH_CHECK(o.is_cuda() && o.scalar_type() == at::kFloat && o.is_contiguous() && o.numel() == rows * cols &&
                    o.device() == w.device(), "pack_conv_weights_multi: out must be a contiguous fp32 (rows, cols)");
    int64_t* d = h + i * D;
    d[0] = reinterpret_cast<int64_t>(w.data_ptr<float>());
    d[1] = reinterpret_cast<int64_t>(o.data_ptr<float>());
    d[2] = total;
    d[3] = O;
    d[4] = I;
    d[5] = w.size(2);
    d[6] = rows;
    d[7] = cols;
    d[8] = cpad;
    d[9] = mode;
    d[10] = w.stride(0);
    d[11] = w.stride(1);
    d[12] = w.stride(2);
    d[13] = w.stride(3);
    if (mode == 0) {
      total += (rows * cols + 4095) / 4096 * 4096;  // next operand on a chunk boundary (PACK_CHUNK)
    } else {  // one 4096-element chunk per 64 x 64 (ci, co) tile of a tap
      TORCH_CHECK(cols == w.size(2) * w.size(2) * cpad, "pack_conv_weights_multi: dgrad operands need cols = KS*KS*cpad");
      total += ((rows + 63) / 64) * w.size(2) * w.size(2) * ((cpad + 63) / 64) * 4096;
    }
  }
  auto dd = hd.to(ws[0].device(), /*non_blocking=*/true);
  TP_CHECK_HIP(tp_pack_conv_weights_multi(reinterpret_cast<const long long*>(dd.data_ptr<int64_t>()), (int)n,
                                          (long long)total, cur_stream()));
}

// Shapley prefix-delta operands: z (B, C) block output, W (N, C) next Linear, perm (n) int32
// permutation; returns T (cnt*B, Kc) lower-triangular gathered activations and Wsub (N, Kc).
std::tuple<at::Tensor, at::Tensor> prefix_tri_operands(const at::Tensor& z, const at::Tensor& w, const at::Tensor& perm,
                                                       int64_t p0, int64_t cnt, int64_t Kc) {
  need(z, "z", 2);
  need(w, "w", 2, &z);
  TORCH_CHECK(perm.is_cuda() && perm.device() == z.device() && perm.scalar_type() == at::kInt &&
                  perm.is_contiguous() && perm.dim() == 1, "perm must be a contiguous int32 GPU vector on z's device");
  const int64_t B = z.size(0), C = z.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == C, "w must be (N, C) with z's C");
  TORCH_CHECK(cnt >= 1 && Kc >= cnt && Kc % 32 == 0, "need 1 <= cnt <= Kc, Kc % 32 == 0");
  // prefixes p0 .. p0+cnt-1 read perm[p0 .. p0+cnt-2] (the last copy's extra units)
  TORCH_CHECK(p0 >= 0 && p0 + cnt - 1 <= perm.numel() && perm.numel() <= C, "prefix range out of the permutation");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(z.device());
  auto T = at::empty({cnt * B, Kc}, z.options());
  auto Ws = at::empty({N, Kc}, z.options());
  TP_CHECK_HIP(tp_prefix_tri_operands(z.data_ptr<float>(), w.data_ptr<float>(), perm.data_ptr<int>(), (int)B, (int)C,
                                      (int)N, (int)p0, (int)cnt, (int)Kc, T.data_ptr<float>(), Ws.data_ptr<float>(),
                                      cur_stream()));
  return {T, Ws};
}

// out (M, N) = act(Y0[r % B0] - T @ Wsub^T) on the MFMA GEMM (prefix-delta Shapley evaluation).
at::Tensor prefix_delta(const at::Tensor& T, const at::Tensor& wsub, const at::Tensor& neg_one, const at::Tensor& y0,
                        bool relu, double slope, int64_t cfg) {
  need(T, "T", 2);
  need(wsub, "wsub", 2, &T);
  need(y0, "y0", 2, &T);
  const int64_t M = T.size(0), Kc = T.size(1), N = wsub.size(0), B0 = y0.size(0);
  TORCH_CHECK(wsub.size(1) == Kc && y0.size(1) == N, "shape mismatch: T (M, Kc), wsub (N, Kc), y0 (B0, N)");
  TORCH_CHECK(M > 0 && Kc > 0 && N > 0 && B0 > 0, "empty operand: T (", M, ", ", Kc, "), y0 (", B0, ", ", N, ")");
  TORCH_CHECK(M < (1ll << 31) && Kc < (1ll << 31) && N < (1ll << 31), "operand sizes are 32-bit");
  TORCH_CHECK(Kc % 32 == 0 && N % 4 == 0 && M % B0 == 0, "need Kc % 32 == 0, N % 4 == 0, M % B0 == 0");
  TORCH_CHECK(cfg >= 0 && cfg <= 6, "bad tile config");
  TORCH_CHECK(neg_one.defined(), "neg_one must be the (N,) scale vector");
  const float* no = opt_ptr(neg_one, N, "neg_one", T);
  // float4 operand loads and epilogue reads: a contiguous view at an odd offset must not reach the kernel
  for (const at::Tensor* t : {&T, &wsub, &y0})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr<float>()) % 16 == 0,
                "T, wsub and y0 must be 16-byte aligned");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(T.device());
  auto out = at::empty({M, N}, T.options());
  TP_CHECK_HIP(tp_prefix_delta_gemm(T.data_ptr<float>(), wsub.data_ptr<float>(), no, y0.data_ptr<float>(), (int)M,
                                    (int)Kc, (int)N, (int)B0, relu ? 1 : 0, (float)slope, (int)cfg,
                                    out.data_ptr<float>(), cur_stream()));
  return out;
}

// fp32 images, or bf16 ones (the BF kernels; staged input modes only): returns the staged-flag bit
int need_u(const at::Tensor& u, int64_t C, int64_t K, const at::Tensor& like) {
  TORCH_CHECK(u.is_cuda() && u.device() == like.device() && u.is_contiguous() && u.dim() == 3 &&
                  (u.scalar_type() == at::kFloat || u.scalar_type() == at::kBFloat16),
              "u must be a contiguous float32 or bfloat16 tensor (C/8, K/32, 4096) on the other operands' device");
  TORCH_CHECK(C % 8 == 0 && K % 32 == 0 && u.size(0) == C / 8 && u.size(1) == K / 32 && u.size(2) == 4096,
              "u must be the Winograd U images (C/8, K/32, 4096) = (", C / 8, ", ", K / 32, ", 4096), got ",
              u.sizes());
  return u.scalar_type() == at::kBFloat16 ? 2 : 0;
}

// Winograd F(2x2,3x3) forward: x (B,H,W,C) NHWC, u (16, C, K) from winograd_weights().
std::tuple<at::Tensor, at::Tensor> conv_wino_fwd(const at::Tensor& x, const at::Tensor& u, const OptTensor& scale,
                                                 const OptTensor& shift, bool relu, bool pool, int64_t splits,
                                                 bool staged, const OptTensor& apoz) {
  need(x, "x", 4);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), K = u.size(1) * 32;
  const int ubf = need_u(u, C, K, x);
  TORCH_CHECK(!ubf || staged, "bf16 U images need the staged kernels");
  TORCH_CHECK(!pool || (H % 2 == 0 && W % 2 == 0), "Winograd with pooling needs even H, W");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* sc = opt_ptr(scale, K, "scale", x);
  const float* sh = opt_ptr(shift, K, "shift", x);
  auto [out, am] = conv_out(x, B, H, W, K, pool);
  const int64_t sp = norm_splits(splits, C / 8);
  at::Tensor ws = splitk_ws(sp, B * H * W * K, x);
  float* ap = count_ptr(apoz, B, K, x);
  TP_CHECK_HIP(tp_conv_wino(x.data_ptr<float>(), nullptr, static_cast<const float*>(u.data_ptr()), (int)B, (int)H,
                            (int)W, (int)C, (int)K, 0, pool ? EPI_FWD_POOL : EPI_FWD, (int)sp, (staged ? 1 : 0) | ubf,
                            sc, sh, relu ? 1 : 0, out.data_ptr<float>(), pool ? am.data_ptr<uint8_t>() : nullptr,
                            nullptr, nullptr, ap, ptr_or_null(ws), 0, cur_stream()));
  return {out, am};
}

// Winograd dgrad with the conv_dgrad epilogue contract; ut = winograd_weights of the
// flipped/transposed kernel, (16, Cout, Cin).
at::Tensor conv_wino_dgrad(const at::Tensor& g, const OptTensor& g_argmax, const at::Tensor& ut, const at::Tensor& act,
                           const OptTensor& bn_scale, const OptTensor& taylor, bool want_out, int64_t splits,
                           bool staged, int64_t tay_mode) {
  need(g, "g", 4);
  need(act, "act", 4, &g);
  const int64_t B = act.size(0), H = act.size(1), W = act.size(2), Cin = act.size(3), Cout = g.size(3);
  const int ubf = need_u(ut, Cout, Cin, g);
  TORCH_CHECK(!ubf || staged, "bf16 U images need the staged kernels");
  const uint8_t* am = pooled_grad(g, g_argmax, B, H, W);  // (pooled: H, W are even)
  const int tm = tay_mode_arg(tay_mode, 2);               // the launcher passes it on unchecked
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const float* sc = opt_ptr(bn_scale, Cin, "bn_scale", g);
  // at least winograd_taylor_slots(H, W) partial slots
  float* tay = taylor_ptr(taylor, tp_wino_taylor_slots((int)H, (int)W), false, B, Cin, g);
  at::Tensor out;
  if (want_out) out = at::empty({B, H, W, Cin}, g.options());
  const int64_t sp = norm_splits(splits, Cout / 8);
  at::Tensor ws = splitk_ws(sp, B * H * W * Cin, g);
  TP_CHECK_HIP(tp_conv_wino(g.data_ptr<float>(), am, static_cast<const float*>(ut.data_ptr()), (int)B, (int)H, (int)W,
                            (int)Cout, (int)Cin, am ? 1 : 0, EPI_BWD, (int)sp, (staged ? 1 : 0) | ubf, sc, nullptr, 0,
                            ptr_or_null(out), nullptr, act.data_ptr<float>(), tay, nullptr, ptr_or_null(ws), tm,
                            cur_stream()));
  return out;
}

// ---- Winograd F(4x4,3x3) (wino4.hip): square 4/8/16/32-pixel maps --------------------------------
at::Tensor wino4_weights(const at::Tensor& w, bool flip_t, int64_t K, int64_t C) {
  // strided weights welcome (channels_last parameters are read in place)
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 4, "w must be a 4-d float32 GPU tensor");
  TORCH_CHECK(w.stride(0) > 0 && w.stride(1) > 0 && w.stride(2) > 0 && w.stride(3) > 0, "w: positive strides only");
  TORCH_CHECK(w.size(2) == 3 && w.size(3) == 3, "w must be (.., .., 3, 3)");
  if (K <= 0) K = flip_t ? w.size(1) : w.size(0);
  if (C <= 0) C = flip_t ? w.size(0) : w.size(1);
  TORCH_CHECK(K % 32 == 0 && C % 8 == 0, "F(4x4) U images need K % 32 == 0 and C % 8 == 0");
  TORCH_CHECK(flip_t ? (w.size(0) <= C && w.size(1) <= K) : (w.size(0) <= K && w.size(1) <= C),
              "weight wider than the padded GEMM");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(w.device());
  auto u = at::empty({C / 8, K / 32, (int64_t)tp_wino4_u_img()}, w.options());
  TP_CHECK_HIP(tp_wino4_weights_strided(w.data_ptr<float>(), u.data_ptr<float>(), (int)K, (int)C, flip_t ? 1 : 0,
                                        (int)w.size(0), (int)w.size(1), w.stride(0), w.stride(1), (int)w.stride(2),
                                        (int)w.stride(3), cur_stream()));
  return u;
}

void need_u4(const at::Tensor& u, int64_t C, int64_t K, const at::Tensor& like) {
  need(u, "u", 3, &like);
  TORCH_CHECK(C % 8 == 0 && K % 32 == 0 && u.size(0) == C / 8 && u.size(1) == K / 32 && u.size(2) == tp_wino4_u_img(),
              "u must be the F(4x4) U images (C/8, K/32, ", tp_wino4_u_img(), "), got ", u.sizes());
}

// F(4x4) U images of many 3x3 weights in one launch: us[i] <- ws[i] per cfg[3i:3i+3] = (K, C,
// flip_t) (the padded GEMM widths, as wino4_weights). ws may be strided (channels_last).
void wino4_weights_multi(const std::vector<at::Tensor>& ws, const std::vector<at::Tensor>& us,
                         const std::vector<int64_t>& cfg) {
  constexpr int D = 12;
  const int64_t n = (int64_t)ws.size();
  TORCH_CHECK(n > 0 && (int64_t)us.size() == n && (int64_t)cfg.size() == 3 * n,
              "wino4_weights_multi: ws, us and 3 ints per operand");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ws[0].device());
  auto hd = at::empty({n * D}, at::TensorOptions().dtype(at::kLong).pinned_memory(true));
  int64_t* h = hd.data_ptr<int64_t>();
  int64_t total = 0;
  for (int64_t i = 0; i < n; ++i) {
    const at::Tensor& w = ws[i];
    const int64_t K = cfg[3 * i], C = cfg[3 * i + 1], flip = cfg[3 * i + 2];
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 4 && w.size(2) == 3 && w.size(3) == 3 &&
                    w.device() == ws[0].device() && w.stride(0) > 0 && w.stride(1) > 0 && w.stride(2) > 0 &&
                    w.stride(3) > 0, "wino4_weights_multi: fp32 (O, I, 3, 3) GPU weights");
    TORCH_CHECK(K > 0 && C > 0 && K % 32 == 0 && C % 8 == 0 &&
                    (flip ? (w.size(0) <= C && w.size(1) <= K) : (w.size(0) <= K && w.size(1) <= C)),
                "wino4_weights_multi: bad padded widths");
    need_u4(us[i], C, K, w);
    int64_t* d = h + i * D;
    d[0] = reinterpret_cast<int64_t>(w.data_ptr<float>());
    d[1] = reinterpret_cast<int64_t>(us[i].data_ptr<float>());
    d[2] = total;
    d[3] = K;
    d[4] = C;
    d[5] = flip ? 1 : 0;
    d[6] = w.size(0);
    d[7] = w.size(1);
    d[8] = w.stride(0);
    d[9] = w.stride(1);
    d[10] = w.stride(2);
    d[11] = w.stride(3);
    total += C * K;  // a multiple of 256: every block stays inside one operand
  }
  auto dd = hd.to(ws[0].device(), /*non_blocking=*/true);
  TP_CHECK_HIP(tp_wino4_weights_multi(reinterpret_cast<const long long*>(dd.data_ptr<int64_t>()), (int)n,
                                      (long long)total, cur_stream()));
}

std::tuple<at::Tensor, at::Tensor> conv_wino4_fwd(const at::Tensor& x, const at::Tensor& u, const OptTensor& scale,
                                                  const OptTensor& shift, bool relu, bool pool, const OptTensor& apoz,
                                                  int64_t splits, int64_t variant, int64_t ko) {
  need(x, "x", 4);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), Kc = u.size(1) * 32;
  need_u4(u, C, Kc, x);
  TORCH_CHECK(tp_wino4_ok((int)H, (int)W, (int)C, (int)Kc), "F(4x4) Winograd needs square 4/8/16/32 (or, split-points "
              "variant 3 without pooling, 56/28/14/7) maps, C % 8 == 0, "
              "K % 32 == 0; got ", x.sizes(), " K=", Kc);
  // ko: stored output channels (pruned widths: the U images / MFMAs are 32-padded, HBM rows are not)
  const int64_t K = ko > 0 ? ko : Kc;
  TORCH_CHECK(K % 4 == 0 && K <= Kc && K > Kc - 32, "ko must be a multiple of 4 in (K - 32, K]; got ko=", ko, " K=", Kc);
  TORCH_CHECK(K == Kc || splits <= 1, "ko < K needs one K pass (splits=1)");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* sc = opt_ptr(scale, K, "scale", x);
  const float* sh = opt_ptr(shift, K, "shift", x);
  auto [out, am] = conv_out(x, B, H, W, K, pool);
  float* ap = count_ptr(apoz, B, K, x);
  // (clamped only: the launcher drops the empty splits and the slabs of the rest still fit)
  const int64_t sp = std::max<int64_t>(1, std::min<int64_t>(splits, C / 8));
  at::Tensor ws = splitk_ws(sp, B * H * W * K, x);
  TP_CHECK_HIP(tp_conv_wino4(x.data_ptr<float>(), u.data_ptr<float>(), (int)B, (int)H, (int)C, (int)Kc,
                             pool ? EPI_FWD_POOL : EPI_FWD, sc, sh, relu ? 1 : 0, out.data_ptr<float>(),
                             pool ? am.data_ptr<uint8_t>() : nullptr, nullptr, nullptr, ap, 0, (int)sp,
                             ptr_or_null(ws), (int)variant, cur_stream(), nullptr, (int)K));
  return {out, am};
}

// F(4x4) dgrad with the conv_wino_dgrad epilogue contract (input: the unpooled grad). unpool_am
// (B, H, W, Cin) uint8, with want_out and one K pass: the output is written unpooled through those
// 2x2-pool argmax bytes at (B, 2H, 2W, Cin) — the operand of the previous layer's data gradient
at::Tensor conv_wino4_dgrad(const at::Tensor& g, const at::Tensor& ut, const at::Tensor& act, const OptTensor& bn_scale,
                            const OptTensor& taylor, bool want_out, int64_t tay_mode, int64_t splits, int64_t variant,
                            const OptTensor& unpool_am) {
  need(g, "g", 4);
  need(act, "act", 4, &g);
  // Cin: the stored input-gradient channels (act's width); the U images cover Cin rounded up to 32
  const int64_t B = act.size(0), H = act.size(1), W = act.size(2), Cin = act.size(3), Cout = g.size(3);
  const int64_t Kc = ut.dim() == 3 ? ut.size(1) * 32 : 0;
  need_u4(ut, Cout, Kc, g);
  TORCH_CHECK(Cin % 4 == 0 && Cin <= Kc && Cin > Kc - 32, "act width must be the U images' output width up to its "
              "32-granule; got ", Cin, " vs ", Kc);
  TORCH_CHECK(g.size(0) == B && g.size(1) == H && g.size(2) == W, "grad shape mismatch");
  TORCH_CHECK(tp_wino4_ok((int)H, (int)W, (int)Cout, (int)Kc), "F(4x4) dgrad needs square 4/8/16/32/56/28/14/7 maps, "
              "Cout % 8 == 0, Cin % 32 == 0");
  const int tm = tay_mode_arg(tay_mode, 2);  // the launcher passes it on unchecked
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const float* sc = opt_ptr(bn_scale, Cin, "bn_scale", g);
  float* tay = taylor_ptr(taylor, tp_wino4_taylor_slots((int)H), false, B, Cin, g);
  const int64_t sp = std::max<int64_t>(1, std::min<int64_t>(splits, Cout / 8));
  TORCH_CHECK(Cin == Kc || sp == 1, "an unpadded output width needs one K pass (splits=1)");
  const uint8_t* unp = nullptr;
  if (present(unpool_am)) {  // one byte per element of act
    TORCH_CHECK(want_out && sp == 1, "fused unpooling needs want_out and one K pass (splits=1)");
    unp = argmax_ptr(*unpool_am, "unpool_am", act);
  }
  at::Tensor out;
  if (want_out) out = unp ? at::empty({B, 2 * H, 2 * W, Cin}, g.options()) : at::empty({B, H, W, Cin}, g.options());
  at::Tensor ws = splitk_ws(sp, B * H * W * Cin, g);
  TP_CHECK_HIP(tp_conv_wino4(g.data_ptr<float>(), ut.data_ptr<float>(), (int)B, (int)H, (int)Cout, (int)Kc,
                             EPI_BWD, sc, nullptr, 0, ptr_or_null(out), nullptr, act.data_ptr<float>(), tay, nullptr,
                             tm, (int)sp, ptr_or_null(ws), (int)variant, cur_stream(), unp, (int)Cin));
  return out;
}

}  // namespace

int64_t wino_taylor_slots(int64_t H, int64_t W) { return tp_wino_taylor_slots((int)H, (int)W); }

// Operands and geometry of a GEN forward conv (conv_gen, conv_gen_stats): x NHWC (B,H,W,Cin), w (Cout, K).
struct GenShape {
  int64_t B, H, W, Cin, Cout, Ho, Wo;
};
static GenShape gen_shape(const at::Tensor& x, const at::Tensor& w, int64_t ks, int64_t stride, int64_t pad) {
  need(x, "x", 4);
  need(w, "w", 2, &x);
  const int64_t H = x.size(1), W = x.size(2), Cin = x.size(3), Cout = w.size(0);
  TORCH_CHECK((Cin % 4 == 0 && Cin >= 8 && (ks == 1 || ks == 3 || ks == 5)) ||
                  (Cin == 4 && (ks == 3 || ks == 5 || ks == 7)),
              "GEN convs support ks 1/3/5 with Cin % 4 == 0 (>= 8), or ks 3/5/7 with a 4-channel input");
  TORCH_CHECK(w.size(1) == tp_conv_gen_k((int)ks, (int)Cin), "weight K mismatch");
  TORCH_CHECK(stride >= 1 && pad >= 0, "bad stride/pad");
  TORCH_CHECK(Cout % 4 == 0, "GEN convs need Cout % 4 == 0");
  return {x.size(0), H, W, Cin, Cout, (H + 2 * pad - ks) / stride + 1, (W + 2 * pad - ks) / stride + 1};
}

// General strided conv forward (ResNet): x NHWC (B,H,W,Cin) with Cin % 32 == 0 (ks 1 or 3) or
// Cin == 4 (ks 7, padded stem input); w (Cout, K) with K = conv_gen_k(ks, Cin), k = (kh,kw,ci).
// Epilogue: out = relu?(acc*scale + shift + res); apoz (B, Cout) += count(out > 0).
at::Tensor conv_gen(const at::Tensor& x, const at::Tensor& w, const OptTensor& scale, const OptTensor& shift, bool relu,
                    const OptTensor& res, const OptTensor& apoz, int64_t ks, int64_t stride, int64_t pad, int64_t cfg,
                    int64_t splits) {
  const auto [B, H, W, Cin, Cout, Ho, Wo] = gen_shape(x, w, ks, stride, pad);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* sc = opt_ptr(scale, Cout, "scale", x);
  const float* sh = opt_ptr(shift, Cout, "shift", x);
  const float* rp = res_ptr(res, B, Ho, Wo, Cout, 1, x);
  float* ap = count_ptr(apoz, B, Cout, x);
  auto out = at::empty({B, Ho, Wo, Cout}, x.options());
  const int64_t sp = norm_splits(splits, w.size(1) / 32);
  SkPlan sk = sk_plan(sp == 1 && Cin != 4, cfg, ks, false, B * Ho * Wo, Cout, x);
  if (sp > 1) sk.ws = splitk_ws(sp, B * Ho * Wo * Cout, x);
  TP_CHECK_HIP(tp_conv_gen(x.data_ptr<float>(), w.data_ptr<float>(), (int)B, (int)H, (int)W, (int)Cin, (int)Cout,
                           (int)ks, (int)stride, (int)pad, 0, 0, 0, (int)sk.cfg, (int)sp, sc, sh, relu ? 1 : 0, rp, 1,
                           nullptr, ap, out.data_ptr<float>(), ptr_or_null(sk.ws), nullptr, nullptr, 0, nullptr,
                           nullptr, nullptr, nullptr, nullptr, cur_stream()));
  return out;
}

int64_t conv_gen_k(int64_t ks, int64_t Cin) { return tp_conv_gen_k((int)ks, (int)Cin); }

// NHWC k x k / stride s / padding p max-pool (NaN-propagating, padded taps skipped)
at::Tensor maxpool_nhwc(const at::Tensor& x, int64_t k, int64_t s, int64_t pad) {
  need(x, "x", 4);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(C % 4 == 0, "maxpool_nhwc needs C % 4 == 0");
  const int64_t Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({B, Ho, Wo, C}, x.options());
  TP_CHECK_HIP(tp_maxpool_nhwc(x.data_ptr<float>(), y.data_ptr<float>(), (int)B, (int)H, (int)W, (int)C, (int)k,
                               (int)s, (int)pad, cur_stream()));
  return y;
}

// NHWC global average pool -> (B, C)
at::Tensor avgpool_nhwc(const at::Tensor& x) {
  need(x, "x", 4);
  const int64_t B = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({B, C}, x.options());
  TP_CHECK_HIP(tp_avgpool_nhwc(x.data_ptr<float>(), y.data_ptr<float>(), (int)B, (int)HW, (int)C, cur_stream()));
  return y;
}

// NHWC 2x2/stride-2 max-pool (NaN-propagating) -> (pooled, argmax bytes)
std::tuple<at::Tensor, at::Tensor> maxpool2_nhwc(const at::Tensor& x) {
  need(x, "x", 4);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(H % 2 == 0 && W % 2 == 0, "maxpool2 needs even H, W");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({B, H / 2, W / 2, C}, x.options());
  auto am = at::empty({B, H / 2, W / 2, C}, x.options().dtype(at::kByte));
  TP_CHECK_HIP(tp_maxpool2_nhwc(x.data_ptr<float>(), y.data_ptr<float>(), am.data_ptr<uint8_t>(), (int)B, (int)H,
                                (int)W, (int)C, cur_stream()));
  return {y, am};
}

// inverse of maxpool2_nhwc: scatter the pooled gradient to the argmax positions
at::Tensor unpool2_nhwc(const at::Tensor& g, const at::Tensor& am) {
  need(g, "g", 4);
  const uint8_t* amp = argmax_ptr(am, "am", g);
  const int64_t B = g.size(0), H = g.size(1) * 2, W = g.size(2) * 2, C = g.size(3);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  auto out = at::empty({B, H, W, C}, g.options());
  TP_CHECK_HIP(tp_unpool2_nhwc(g.data_ptr<float>(), amp, out.data_ptr<float>(), (int)B, (int)H, (int)W, (int)C,
                               cur_stream()));
  return out;
}

// NCHW -> NHWC with the channel dim zero-padded to Cp (first-layer input of the MFMA kernels).
at::Tensor nchw_to_nhwc_pad(const at::Tensor& x, int64_t Cp) {
  need(x, "x", 4);
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(Cp >= C && Cp % 4 == 0, "Cp must be >= C and a multiple of 4");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({B, H, W, Cp}, x.options());
  TP_CHECK_HIP(tp_nchw_to_nhwc_pad(x.data_ptr<float>(), y.data_ptr<float>(), (int)B, (int)C, (int)H, (int)W, (int)Cp,
                                   cur_stream()));
  return y;
}

// Data gradient of a ResNet conv for the backward engine: g (B, H, W, C = forward Cout) NHWC,
// wt (N = forward Cin, ks*ks*C) with k = (kh, kw, co) and the BN scale folded into co.
// transposed: output (B, Ho, Wo, N) gathers y pixel ((oh + pad - kh)/stride, ...) (strided
// conv dgrad); otherwise a plain stride-1 conv of g (1x1, or 3x3 with flipped taps).
// Epilogue: v (+ res, res_stride-scattered) then out = mask > 0 ? v : 0 when mask is given.
at::Tensor conv_gen_bwd(const at::Tensor& g, const at::Tensor& wt, const OptTensor& res, int64_t res_stride,
                        const OptTensor& mask, int64_t ks, int64_t stride, int64_t pad, int64_t Ho, int64_t Wo,
                        bool transposed, int64_t cfg, int64_t splits, const OptTensor& taylor, int64_t tay_mode) {
  need(g, "g", 4);
  need(wt, "wt", 2, &g);
  const int64_t B = g.size(0), H = g.size(1), W = g.size(2), C = g.size(3), N = wt.size(0);
  TORCH_CHECK(C % 4 == 0 && C >= 8 && (ks == 1 || ks == 3 || (ks == 5 && !transposed)),
              "conv_gen_bwd needs C % 4 == 0 (>= 8) and ks 1/3 (5 for stride-1 convs)");
  TORCH_CHECK(wt.size(1) == tp_conv_gen_k((int)ks, (int)C), "wt must be (N, ks*ks*ceil32(C))");
  TORCH_CHECK(N % 4 == 0 && res_stride >= 1 && stride >= 1 && pad >= 0, "bad N/stride/pad");
  if (!transposed) {
    TORCH_CHECK(stride == 1, "non-transposed conv_gen_bwd is stride 1");
    Ho = (H + 2 * pad - ks) + 1;
    Wo = (W + 2 * pad - ks) + 1;
  } else {
    TORCH_CHECK((Ho + 2 * pad - ks) / stride + 1 == H && (Wo + 2 * pad - ks) / stride + 1 == W,
                "Ho/Wo inconsistent with the forward conv geometry");
  }
  // the kernel tests tay_mode for zero only: 0 Taylor, 1 Sensitivity (the launcher passes it on unchecked)
  const int tm = tay_mode_arg(tay_mode, 1);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const float* rp = res_ptr(res, B, Ho, Wo, N, res_stride, g);
  const float* mp = nhwc_ptr(mask, "mask", B, Ho, Wo, N, g);
  auto out = at::empty({B, Ho, Wo, N}, g.options());
  const int64_t sp = transposed ? 1 : norm_splits(splits, wt.size(1) / 32);
  float* tp_ = nullptr;
  if (present(taylor)) {
    // fused Taylor / Sensitivity partials (R, B, N) of the masked output: a 1x1 stride-1 dgrad
    // (one K pass), or a transposed 3x3 stride-2 one at even Ho / Wo (the parity row order: one
    // slot range per stride phase, R = 4 x the slots of an Ho/2 x Wo/2 group)
    const bool t3 = transposed && ks == 3 && stride == 2 && Ho % 2 == 0 && Wo % 2 == 0;
    const int R = t3 ? 4 * tp_conv_gen_tay_slots((int)cfg, (int)(Ho * Wo / 4))
                     : tp_conv_gen_tay_slots((int)cfg, (int)(Ho * Wo));
    TORCH_CHECK(((!transposed && ks == 1) || t3) && mp != nullptr && sp == 1 && R > 0,
                "conv_gen_bwd taylor partials need a mask and a 1x1 stride-1 dgrad (one K pass) or a transposed "
                "3x3 stride-2 dgrad at even output size, and a tile config spanning <= 4 row groups");
    tp_ = taylor_ptr(taylor, R, true, B, N, g);
  }
  SkPlan sk = sk_plan(sp == 1 && !transposed, cfg, ks, tp_ != nullptr, B * Ho * Wo, N, g);
  if (sp > 1) sk.ws = splitk_ws(sp, B * Ho * Wo * N, g);
  TP_CHECK_HIP(tp_conv_gen(g.data_ptr<float>(), wt.data_ptr<float>(), (int)B, (int)H, (int)W, (int)C, (int)N,
                           (int)ks, (int)stride, (int)pad, transposed ? 1 : 0, (int)Ho, (int)Wo, (int)sk.cfg, (int)sp,
                           nullptr, nullptr, 0, rp, (int)res_stride, mp, nullptr, out.data_ptr<float>(),
                           ptr_or_null(sk.ws), nullptr, tp_, tm, nullptr, nullptr, nullptr, nullptr, nullptr,
                           cur_stream()));
  return out;
}

int64_t conv_gen_tay_slots(int64_t cfg, int64_t HWo) { return tp_conv_gen_tay_slots((int)cfg, (int)HWo); }

// Data gradient of a 1x1 stride-1 conv (the training path's residual-block conv1) with the two
// fusions of a bottleneck's backward (tp_conv_gen):
//   res_bits: ``res`` is the raw gradient of the block output's ReLU, masked here by its bit mask;
//   bn_y / bn_mean / bn_invstd (/ bn_bits): the output gradient reaches a BatchNorm (+ ReLU) whose
//     backward statistics (sum gm, sum gm * xhat) come back per M tile, [tiles][2][N] fp64.
// Returns (dx (B, H, W, N), tile statistics or an empty tensor).
std::tuple<at::Tensor, at::Tensor> conv_gen_bwd_bn(const at::Tensor& g, const at::Tensor& wt, const OptTensor& res,
                                                   int64_t res_stride, const OptTensor& res_bits,
                                                   const OptTensor& bn_y, const OptTensor& bn_mean,
                                                   const OptTensor& bn_invstd, const OptTensor& bn_bits, int64_t cfg) {
  need(g, "g", 4);
  need(wt, "wt", 2, &g);
  const int64_t B = g.size(0), H = g.size(1), W = g.size(2), C = g.size(3), N = wt.size(0), M = B * H * W;
  TORCH_CHECK(C % 4 == 0 && C >= 8 && N % 4 == 0, "conv_gen_bwd_bn needs C % 4 == 0 (>= 8) and N % 4 == 0");
  TORCH_CHECK(wt.size(1) == tp_conv_gen_k(1, (int)C), "wt must be (N, ceil32(C))");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const float* rp = res_ptr(res, B, H, W, N, res_stride, g);
  const uint8_t* rb = bit_mask_ptr(res_bits, M * N, g, "res_bits");
  TORCH_CHECK(!rb || (rp && res_stride == 1), "res_bits needs a stride-1 res");
  const float* yp = nhwc_ptr(bn_y, "bn_y", B, H, W, N, g);
  at::Tensor part;
  if (yp) {
    const int64_t tm = tp_conv_tile_m((int)cfg);
    part = at::empty({(M + tm - 1) / tm, 2, N}, g.options().dtype(at::kDouble));
  }
  const float* mp = yp ? opt_ptr(bn_mean, N, "bn_mean", g) : nullptr;
  const float* ip = yp ? opt_ptr(bn_invstd, N, "bn_invstd", g) : nullptr;
  TORCH_CHECK(!yp || (mp && ip), "bn_y needs bn_mean and bn_invstd");
  const uint8_t* bb = yp ? bit_mask_ptr(bn_bits, M * N, g, "bn_bits") : nullptr;
  auto out = at::empty({B, H, W, N}, g.options());
  const SkPlan sk = sk_plan(true, cfg, 1, false, M, N, g);
  TP_CHECK_HIP(tp_conv_gen(g.data_ptr<float>(), wt.data_ptr<float>(), (int)B, (int)H, (int)W, (int)C, (int)N, 1, 1,
                           0, 0, 0, 0, (int)sk.cfg, 1, nullptr, nullptr, 0, rp, (int)res_stride, nullptr, nullptr,
                           out.data_ptr<float>(), ptr_or_null(sk.ws), yp ? part.data_ptr<double>() : nullptr, nullptr,
                           0, rb, yp, mp, ip, bb, cur_stream()));
  return {out, part};
}

// Fixup-workspace floats of a stream-K GEN launch of tile config cfg at an M x N GEMM (0 = stream-K
// does not apply; the launcher then runs the data-parallel grid).
int64_t conv_sk_ws(int64_t cfg, int64_t ks, bool tay, int64_t M, int64_t N) {
  return tp_conv_sk_ws_floats((int)(cfg & ~kCfgSK), (int)ks, 0, tay ? 1 : 0, (int)M, (int)N);
}

// Weight gradient: g (B, Ho, Wo, Cout) and x (B, H, W, Cin) NHWC -> dW (Cout, Kpad) with column
// k = (kh, kw, ci) (Kpad = ks*ks*Cin rounded up to 32; padded columns are zero).
// ``out`` (optional): the parameter-shaped gradient (Cout_r, Cin_r, ks, ks), any positive strides,
// written directly (real channels only); the (Cout, Kpad) GEMM result is then not materialised and an
// empty tensor is returned.
at::Tensor conv_wgrad(const at::Tensor& g, const at::Tensor& x, int64_t ks, int64_t stride, int64_t pad, int64_t cfg,
                      int64_t splits, const OptTensor& out) {
  need(g, "g", 4);
  need(x, "x", 4, &g);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3), Cout = g.size(3);
  TORCH_CHECK(Cin % 4 == 0 && Cout % 4 == 0, "conv_wgrad needs Cin % 4 == 0 and Cout % 4 == 0");
  TORCH_CHECK(ks >= 1 && stride >= 1 && pad >= 0, "bad conv geometry");
  TORCH_CHECK(x.numel() > 0 && Cout > 0, "conv_wgrad: empty operand, x ", x.sizes(), " g ", g.sizes());
  TORCH_CHECK(H + 2 * pad >= ks && W + 2 * pad >= ks, "conv_wgrad: a ", ks, "x", ks, " kernel on a padded map of ",
              H + 2 * pad, "x", W + 2 * pad);
  const int64_t Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
  TORCH_CHECK(g.size(0) == B && g.size(1) == Ho && g.size(2) == Wo, "g must be (B, Ho, Wo, Cout) of this conv");
  need_aligned16(g, "g");
  need_aligned16(x, "x");
  const int64_t Kpad = (ks * ks * Cin + 31) / 32 * 32;
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const ParamOut f = present(out) ? param_out(*out, Cout, Cin, ks, g) : ParamOut();
  at::Tensor dw = f.p ? at::Tensor() : at::empty({Cout, Kpad}, g.options());
  const int64_t sp = norm_splits(splits, (B * Ho * Wo + 31) / 32);
  at::Tensor ws = splitk_ws(sp, Cout * Kpad, g);
  TP_CHECK_HIP(tp_conv_wgrad(g.data_ptr<float>(), x.data_ptr<float>(), ptr_or_null(dw), ptr_or_null(ws), (int)B, (int)H,
                             (int)W, (int)Cin, (int)Cout, (int)ks, (int)stride, (int)pad, (int)Kpad, (int)cfg, (int)sp,
                             f.p, f.co, f.ci, f.p ? f.fs : nullptr, 1, 0, 0, cur_stream()));
  return f.p ? at::empty({0}, g.options()) : dw;  // with ``out`` the result is in ``out``
}

// Training conv forward that also returns the BatchNorm statistics of its output: y (B, Ho, Wo,
// Cout) and per M tile the column sums / sums of squares, (ceil(M / tile_m(cfg)), 2, Cout) fp64
// (fold with bn_train_fwd(..., pre=)). No split-K, no epilogue besides the bias.
std::tuple<at::Tensor, at::Tensor> conv_gen_stats(const at::Tensor& x, const at::Tensor& w, const OptTensor& shift,
                                                  int64_t ks, int64_t stride, int64_t pad, int64_t cfg) {
  const auto [B, H, W, Cin, Cout, Ho, Wo] = gen_shape(x, w, ks, stride, pad);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* sh = opt_ptr(shift, Cout, "shift", x);
  auto out = at::empty({B, Ho, Wo, Cout}, x.options());
  const int64_t M = B * Ho * Wo, tm = tp_conv_tile_m((int)cfg);
  auto part = at::empty({(M + tm - 1) / tm, 2, Cout}, x.options().dtype(at::kDouble));
  const SkPlan sk = sk_plan(Cin != 4, cfg, ks, false, M, Cout, x);
  TP_CHECK_HIP(tp_conv_gen(x.data_ptr<float>(), w.data_ptr<float>(), (int)B, (int)H, (int)W, (int)Cin, (int)Cout,
                           (int)ks, (int)stride, (int)pad, 0, 0, 0, (int)sk.cfg, 1, nullptr, sh, 0, nullptr, 1, nullptr,
                           nullptr, out.data_ptr<float>(), ptr_or_null(sk.ws), part.data_ptr<double>(), nullptr, 0,
                           nullptr, nullptr, nullptr, nullptr, nullptr, cur_stream()));
  return {out, part};
}

// Winograd F(2x2,3x3) weight gradient of a stride-1 pad-1 3x3 conv: g (B, H, W, Cout), x (B, H, W,
// Cin) NHWC (H, W even, Cin % 4 == 0 and >= 8, Cout % 4 == 0: the GEMM pads Cin to its 32-wide K granule itself)
// -> ``out`` (Cout_r, Cin_r, 3, 3), any positive strides (real channels).
void wino_wgrad(const at::Tensor& g, const at::Tensor& x, int64_t cfg, int64_t splits, at::Tensor& out) {
  need(g, "g", 4);
  need(x, "x", 4, &g);
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3), Cout = g.size(3);
  TORCH_CHECK(g.size(0) == B && g.size(1) == H && g.size(2) == W, "g must be (B, H, W, Cout) of a same-size conv");
  TORCH_CHECK(x.numel() > 0 && Cout > 0, "wino_wgrad: empty operand, x ", x.sizes(), " g ", g.sizes());
  TORCH_CHECK(cfg >= 0 && cfg <= 2, "wino_wgrad: bad tile config ", cfg, " (0 .. 2)");
  need_aligned16(g, "g");
  need_aligned16(x, "x");
  TORCH_CHECK(H % 2 == 0 && W % 2 == 0 && Cin % 4 == 0 && Cin >= 8 && Cout % 4 == 0,
              "wino_wgrad needs even H/W, Cin % 4 (>= 8), Cout % 4");
  const ParamOut f = param_out(out, Cout, Cin, 3, g);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const int64_t sp = norm_splits(splits, (B * (H / 2) * (W / 2) + 31) / 32);
  auto ws = at::empty({tp_wino_wgrad_ws_elems((int)B, (int)H, (int)W, (int)Cin, (int)Cout, (int)sp)}, g.options());
  TP_CHECK_HIP(tp_wino_wgrad(g.data_ptr<float>(), x.data_ptr<float>(), ws.data_ptr<float>(), (int)B, (int)H, (int)W,
                             (int)Cin, (int)Cout, (int)cfg, (int)sp, f.p, f.co, f.ci, f.fs, cur_stream()));
}

// (G, 2, C) fp64 statistics that the producing conv reduced per M tile (conv_gen_stats, conv_gen_bwd_bn); nullable
const double* tile_stats(const OptTensor& pre, int64_t C, const at::Tensor& like) {
  if (!present(pre)) return nullptr;
  TORCH_CHECK(pre->is_cuda() && pre->scalar_type() == at::kDouble && pre->is_contiguous() && pre->dim() == 3 &&
                  pre->size(0) > 0 && pre->size(1) == 2 && pre->size(2) == C && pre->device() == like.device(),
              "pre must be (G, 2, C) float64 tile statistics on the device");
  return pre->data_ptr<double>();
}

// Training-mode BatchNorm over the last dim of a channels-last activation x (..., C).
// Updates running_mean / running_var in place (momentum, unbiased variance) when given.
// Optional fused residual add and ReLU:
// y = relu?(BN(x) + res?). Returns (y, mean, invstd).
// With ``relu`` also returns the ReLU bit mask (ceil(P*C/4) bytes; else an empty tensor) for bn_train_bwd.
// Any C (C % 4 == 0: float4 rows; else per-element). ``cr`` (0 = C): the channels with parameters /
// running statistics; x's channels c >= cr are the zero padding of a pruned width (outputs 0).
// ``act``: the activation code, 0 none, 1 ReLU, 2 ReLU6 (y = min(max(v, 0), 6)); it wins over ``relu``
// when non-zero, ``relu`` alone means 1. With an activation the bit mask is always returned (bit =
// the gradient passes: v > 0, or 0 < v < 6 for ReLU6, whose backward has no other masking mode).
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> bn_train_fwd(
    const at::Tensor& x, const OptTensor& gamma, const OptTensor& beta, const OptTensor& running_mean,
    const OptTensor& running_var, double eps, double momentum, const OptTensor& res, bool relu, const OptTensor& pre,
    const OptTensor& num_batches, int64_t cr, int64_t act_) {
  TORCH_CHECK(act_ >= 0 && act_ <= 2, "act must be 0 (none), 1 (ReLU) or 2 (ReLU6), got ", act_);
  const int act = act_ != 0 ? (int)act_ : (relu ? 1 : 0);
  need(x, "x", kAnyDims);
  const int64_t C = x.size(-1), P = x.numel() / std::max<int64_t>(C, 1);
  TORCH_CHECK(C > 0 && P > 0, "bn_train_fwd needs a non-empty batch");
  const int64_t Cr = cr > 0 ? cr : C;
  TORCH_CHECK(Cr <= C, "cr must be <= the channel count");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* ga = opt_ptr(gamma, Cr, "gamma", x);
  const float* be = opt_ptr(beta, Cr, "beta", x);
  // the running statistics are updated as a pair (a running_var alone is left untouched)
  float* rm = vec_ptr(running_mean, Cr, "running_mean", x);
  float* rv = rm ? vec_ptr(running_var, Cr, "running_var", x) : nullptr;
  TORCH_CHECK(!rm || rv, "running_mean needs running_var");
  const float* rp = same_shape_ptr(res, "res", x);
  long long* nbt = counter_ptr(num_batches, x);  // the module's num_batches_tracked
  auto y = at::empty_like(x);
  auto mk = at::empty({act ? (P * C + 3) / 4 : 0}, x.options().dtype(at::kByte));
  const int64_t Cs = (C + 3) / 4 * 4;  // row stride: every row 16-byte aligned (float4 reads) for any C
  auto stats = at::empty({4, Cs}, x.options()).narrow(1, 0, C);  // mean, invstd, a, b
  float* sp = stats.data_ptr<float>();
  if (const double* pp = tile_stats(pre, C, x)) {  // statistics reduced per tile by the producing conv
    const int64_t G = pre->size(0);
    auto ws = at::empty({2 * std::min<int64_t>(G, 256) * C}, x.options().dtype(at::kDouble));
    TP_CHECK_HIP(tp_bn_fwd_train_pre(x.data_ptr<float>(), y.data_ptr<float>(), (int)P, (int)C, (int)Cr, ga, be,
                                     (float)eps, (float)momentum, rm, rv, sp, sp + Cs, sp + 2 * Cs, sp + 3 * Cs,
                                     ws.data_ptr<double>(), pp, (int)G, rp, act,
                                     act ? mk.data_ptr<uint8_t>() : nullptr, nbt, cur_stream()));
    return {y, stats[0], stats[1], mk};
  }
  auto ws = at::empty({2 * (int64_t)tp_bn_groups((int)P, (int)C) * C}, x.options().dtype(at::kDouble));
  TP_CHECK_HIP(tp_bn_fwd_train(x.data_ptr<float>(), y.data_ptr<float>(), (int)P, (int)C, (int)Cr, ga, be, (float)eps,
                               (float)momentum, rm, rv, sp, sp + Cs, sp + 2 * Cs, sp + 3 * Cs, ws.data_ptr<double>(), rp,
                               act, act ? mk.data_ptr<uint8_t>() : nullptr, nbt, cur_stream()));
  return {y, stats[0], stats[1], mk};
}

// Backward of bn_train_fwd: (dx or undefined, dgamma, dbeta, dres or undefined). ``ym``: the
// forward output y when it was ReLU'd (the gradient is masked by y > 0 first); ``want_dres``:
// also return that masked gradient (the residual branch's gradient). ``act``: the forward's
// activation code; a ReLU6 forward (2) is masked by its bit mask only ("y > 0" is wrong for it).
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> bn_train_bwd(
    const at::Tensor& g, const at::Tensor& x, const OptTensor& gamma, const at::Tensor& mean,
    const at::Tensor& invstd, bool want_dx, const OptTensor& ym, bool want_dres, const OptTensor& mask, int64_t cr,
    const OptTensor& pre, int64_t act) {
  const bool has_mask = present(mask) && mask->numel() > 0;  // (bn_train_fwd's mask is empty without an activation)
  TORCH_CHECK(act >= 0 && act <= 2, "act must be 0 (none), 1 (ReLU) or 2 (ReLU6), got ", act);
  TORCH_CHECK(act != 2 || (!present(ym) && has_mask),
              "the backward of a ReLU6 forward takes bn_train_fwd's bit mask, not ym");
  need(g, "g", kAnyDims);
  need(x, "x", kAnyDims, &g);
  TORCH_CHECK(g.sizes() == x.sizes(), "g and x must have the same shape");
  const int64_t C = x.size(-1), P = x.numel() / std::max<int64_t>(C, 1);
  TORCH_CHECK(C > 0 && P > 0, "bn_train_bwd needs a non-empty batch");
  const int64_t Cr = cr > 0 ? cr : C;
  TORCH_CHECK(Cr <= C, "cr must be <= the channel count");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* ga = opt_ptr(gamma, Cr, "gamma", x);
  const float* mp = opt_ptr(mean, C, "mean", x);
  const float* ip = opt_ptr(invstd, C, "invstd", x);
  const float* yp = same_shape_ptr(ym, "ym", x);
  const uint8_t* mkp = has_mask ? bit_mask_ptr(mask, P * C, x, "mask") : nullptr;
  const int64_t Cs = (C + 3) / 4 * 4;
  auto coef = at::empty({5, Cs}, x.options());  // dgamma, dbeta, a, k1, k2 (16-byte aligned rows)
  at::Tensor dx, dres;
  if (want_dx) dx = at::empty_like(x);
  if (want_dres) dres = at::empty_like(x);
  float* cp = coef.data_ptr<float>();
  if (const double* pp = tile_stats(pre, C, x)) {  // statistics from the producing GEMM's epilogue (conv_gen_bwd_bn)
    const int64_t G = pre->size(0);
    auto wsp = at::empty({2 * std::min<int64_t>(G, 256) * C}, x.options().dtype(at::kDouble));
    TP_CHECK_HIP(tp_bn_bwd_train_pre(g.data_ptr<float>(), x.data_ptr<float>(), ptr_or_null(dx), (int)P, (int)C, (int)Cr,
                                     ga, mp, ip, cp, cp + Cs, cp + 2 * Cs, cp + 3 * Cs, cp + 4 * Cs,
                                     wsp.data_ptr<double>(), pp, (int)G, mkp ? nullptr : yp, ptr_or_null(dres), mkp,
                                     cur_stream()));
    return {dx, coef[0].narrow(0, 0, Cr), coef[1].narrow(0, 0, Cr), dres};
  }
  auto ws = at::empty({2 * (int64_t)tp_bn_groups((int)P, (int)C) * C}, x.options().dtype(at::kDouble));
  TP_CHECK_HIP(tp_bn_bwd_train(g.data_ptr<float>(), x.data_ptr<float>(), ptr_or_null(dx), (int)P, (int)C, (int)Cr, ga,
                               mp, ip, cp, cp + Cs, cp + 2 * Cs, cp + 3 * Cs, cp + 4 * Cs, ws.data_ptr<double>(),
                               mkp ? nullptr : yp, ptr_or_null(dres), mkp, cur_stream()));
  return {dx, coef[0].narrow(0, 0, Cr), coef[1].narrow(0, 0, Cr), dres};
}

// y = hardswish(BN(x)), training mode, over the last dim of x (..., C): the statistics, running-stat and
// ``cr`` semantics of bn_train_fwd, no residual and no mask. Returns (y, mean, invstd, ab) with ab (2, C)
// the folded affine rows a = gamma * invstd, b = beta - mean * a that bn_hswish_bwd recomputes the
// pre-activation from.
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> bn_hswish_fwd(
    const at::Tensor& x, const OptTensor& gamma, const OptTensor& beta, const OptTensor& running_mean,
    const OptTensor& running_var, double eps, double momentum, const OptTensor& num_batches, int64_t cr) {
  need(x, "x", kAnyDims);
  const int64_t C = x.dim() > 0 ? x.size(-1) : 0, P = x.numel() / std::max<int64_t>(C, 1);
  TORCH_CHECK(C > 0 && P > 0, "bn_hswish_fwd needs a non-empty batch");
  TORCH_CHECK(x.numel() < (1ll << 32), "bn_hswish_fwd: 2^32 elements or more");
  const int64_t Cr = cr > 0 ? cr : C;
  TORCH_CHECK(Cr <= C, "cr must be <= the channel count");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* ga = opt_ptr(gamma, Cr, "gamma", x);
  const float* be = opt_ptr(beta, Cr, "beta", x);
  float* rm = vec_ptr(running_mean, Cr, "running_mean", x);
  float* rv = rm ? vec_ptr(running_var, Cr, "running_var", x) : nullptr;
  TORCH_CHECK(!rm || rv, "running_mean needs running_var");
  long long* nbt = counter_ptr(num_batches, x);
  auto y = at::empty_like(x);
  const int64_t Cs = (C + 3) / 4 * 4;  // row stride: every row 16-byte aligned (float4 reads) for any C
  auto stats = at::empty({4, Cs}, x.options()).narrow(1, 0, C);  // mean, invstd, a, b
  float* sp = stats.data_ptr<float>();
  auto ws = at::empty({2 * (int64_t)tp_bn_groups((int)P, (int)C) * C}, x.options().dtype(at::kDouble));
  TP_CHECK_HIP(tp_bn_hswish_fwd_train(x.data_ptr<float>(), y.data_ptr<float>(), (int)P, (int)C, (int)Cr, ga, be,
                                      (float)eps, (float)momentum, rm, rv, sp, sp + Cs, sp + 2 * Cs, sp + 3 * Cs,
                                      ws.data_ptr<double>(), nbt, cur_stream()));
  return {y, stats[0], stats[1], stats.narrow(0, 2, 2)};
}

// Backward of bn_hswish_fwd: (dx or undefined, dgamma, dbeta). ``ab``: the forward's fourth output.
std::tuple<at::Tensor, at::Tensor, at::Tensor> bn_hswish_bwd(const at::Tensor& g, const at::Tensor& x,
                                                             const OptTensor& gamma, const at::Tensor& mean,
                                                             const at::Tensor& invstd, const at::Tensor& ab,
                                                             bool want_dx, int64_t cr) {
  need(g, "g", kAnyDims);
  need(x, "x", kAnyDims, &g);
  TORCH_CHECK(g.sizes() == x.sizes(), "g and x must have the same shape");
  const int64_t C = x.dim() > 0 ? x.size(-1) : 0, P = x.numel() / std::max<int64_t>(C, 1);
  TORCH_CHECK(C > 0 && P > 0, "bn_hswish_bwd needs a non-empty batch");
  TORCH_CHECK(x.numel() < (1ll << 32), "bn_hswish_bwd: 2^32 elements or more");
  const int64_t Cr = cr > 0 ? cr : C;
  TORCH_CHECK(Cr <= C, "cr must be <= the channel count");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const float* ga = opt_ptr(gamma, Cr, "gamma", x);
  const float* mp = opt_ptr(mean, C, "mean", x);
  const float* ip = opt_ptr(invstd, C, "invstd", x);
  const auto [af, bf] = affine_rows(ab, C, x);
  const int64_t Cs = (C + 3) / 4 * 4;
  auto coef = at::empty({5, Cs}, x.options());  // dgamma, dbeta, a, k1, k2 (16-byte aligned rows)
  at::Tensor dx;
  if (want_dx) dx = at::empty_like(x);
  float* cp = coef.data_ptr<float>();
  auto ws = at::empty({2 * (int64_t)tp_bn_groups((int)P, (int)C) * C}, x.options().dtype(at::kDouble));
  TP_CHECK_HIP(tp_bn_hswish_bwd_train(g.data_ptr<float>(), x.data_ptr<float>(), ptr_or_null(dx), (int)P, (int)C,
                                      (int)Cr, ga, mp, ip, af, bf, cp, cp + Cs, cp + 2 * Cs, cp + 3 * Cs, cp + 4 * Cs,
                                      ws.data_ptr<double>(), cur_stream()));
  return {dx, coef[0].narrow(0, 0, Cr), coef[1].narrow(0, 0, Cr)};
}

void register_engine_ops_def(torch::Library& m) {
  m.def("wino_taylor_slots(int H, int W) -> int", &wino_taylor_slots);
  m.def("wino_lds_bytes() -> int", []() -> int64_t { return tp_wino_lds_bytes(); });
  m.def("wino_staged_ok(int H, int W, bool unpool) -> bool",
        [](int64_t H, int64_t W, bool unpool) -> bool { return tp_wino_staged_ok((int)H, (int)W, unpool ? 1 : 0) != 0; });
  m.def("wino4_taylor_slots(int S) -> int", [](int64_t S) -> int64_t { return tp_wino4_taylor_slots((int)S); });
  m.def("wino4_u_img() -> int", []() -> int64_t { return tp_wino4_u_img(); });
  m.def("wino4_lds_bytes(int S, int variant=0) -> int",
        [](int64_t S, int64_t variant) -> int64_t { return tp_wino4_lds_bytes((int)S, (int)variant); });
  m.def("nchw_to_nhwc_pad(Tensor x, int Cp) -> Tensor");
  m.def("maxpool2_nhwc(Tensor x) -> (Tensor, Tensor)");
  m.def("maxpool_nhwc(Tensor x, int k, int s, int pad) -> Tensor");
  m.def("avgpool_nhwc(Tensor x) -> Tensor");
  m.def("conv_gen(Tensor x, Tensor w, Tensor? scale, Tensor? shift, bool relu, Tensor? res, Tensor(a!)? apoz, "
        "int ks, int stride, int pad, int cfg, int splits) -> Tensor");
  m.def("conv_gen_k(int ks, int Cin) -> int", &conv_gen_k);
  m.def("bn_train_fwd(Tensor x, Tensor? gamma, Tensor? beta, Tensor(a!)? running_mean, Tensor(b!)? running_var, "
        "float eps, float momentum, Tensor? res=None, bool relu=False, Tensor? pre=None, "
        "Tensor(c!)? num_batches=None, int cr=0, int act=0) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("bn_train_bwd(Tensor g, Tensor x, Tensor? gamma, Tensor mean, Tensor invstd, bool want_dx, Tensor? ym=None, "
        "bool want_dres=False, Tensor? mask=None, int cr=0, Tensor? pre=None, int act=0) "
        "-> (Tensor, Tensor, Tensor, Tensor)");
  m.def("bn_hswish_fwd(Tensor x, Tensor? gamma, Tensor? beta, Tensor(a!)? running_mean, Tensor(b!)? running_var, "
        "float eps, float momentum, Tensor(c!)? num_batches=None, int cr=0) "
        "-> (Tensor y, Tensor mean, Tensor invstd, Tensor ab)");
  m.def("bn_hswish_bwd(Tensor g, Tensor x, Tensor? gamma, Tensor mean, Tensor invstd, Tensor ab, bool want_dx, "
        "int cr=0) -> (Tensor dx, Tensor dgamma, Tensor dbeta)");
  m.def("conv_wgrad(Tensor g, Tensor x, int ks, int stride, int pad, int cfg, int splits, Tensor(a!)? out=None) "
        "-> Tensor");
  m.def("pack_conv_weight(Tensor w, int rows, int cols, int cpad, int mode) -> Tensor");
  m.def("pack_conv_weights_multi(Tensor[] ws, Tensor(a!)[] outs, int[] cfg) -> ()");
  m.def("wino4_weights_multi(Tensor[] ws, Tensor(a!)[] us, int[] cfg) -> ()");
  m.def("conv_gen_stats(Tensor x, Tensor w, Tensor? shift, int ks, int stride, int pad, int cfg) -> (Tensor, Tensor)");
  m.def("wino_wgrad(Tensor g, Tensor x, int cfg, int splits, Tensor(a!) out) -> ()");
  m.def("conv_gen_bwd(Tensor g, Tensor wt, Tensor? res, int res_stride, Tensor? mask, int ks, int stride, int pad, "
        "int Ho, int Wo, bool transposed, int cfg, int splits, Tensor(a!)? taylor=None, int tay_mode=0) -> Tensor");
  m.def("conv_gen_tay_slots(int cfg, int HWo) -> int", &conv_gen_tay_slots);
  m.def("conv_gen_bwd_bn(Tensor g, Tensor wt, Tensor? res, int res_stride, Tensor? res_bits, Tensor? bn_y, Tensor? bn_mean, "
        "Tensor? bn_invstd, Tensor? bn_bits, int cfg) -> (Tensor, Tensor)");
  m.def("conv_sk_ws(int cfg, int ks, bool tay, int M, int N) -> int", &conv_sk_ws);
  m.def("unpool2_nhwc(Tensor g, Tensor am) -> Tensor");
  m.def("conv_fwd(Tensor x, Tensor w, Tensor? scale, Tensor? shift, bool relu, bool pool, int ks, int cfg, "
        "int splits, Tensor(a!)? apoz=None, float slope=0.0) -> (Tensor, Tensor)");
  m.def("conv_dgrad(Tensor g, Tensor? g_argmax, Tensor wt, Tensor act, Tensor? bn_scale, Tensor(a!)? taylor, "
        "bool want_out, int ks, int cfg, int splits, int tay_group=0, int tay_mode=0, float slope=0.0) -> Tensor");
  m.def("conv2x2_fast_fwd(Tensor x, Tensor u9, Tensor? scale, Tensor? shift, bool relu, bool pool, int cfg, "
        "int splits) -> (Tensor, Tensor)");
  m.def("conv2x2_fast_dgrad(Tensor g, Tensor? g_argmax, Tensor u9t, Tensor act, Tensor? bn_scale, "
        "Tensor(a!)? taylor, bool want_out, int cfg, int splits, int tay_mode=0) -> Tensor");
  m.def("conv_first(Tensor x, Tensor w, Tensor scale, Tensor shift, bool relu, Tensor? wt=None) -> Tensor");
  m.def("wino_weights(Tensor w, bool flip_t, int K=0, int C=0, bool bf16=False) -> Tensor");
  m.def("prefix_tri_operands(Tensor z, Tensor w, Tensor perm, int p0, int cnt, int Kc) -> (Tensor, Tensor)");
  m.def("prefix_delta(Tensor T, Tensor wsub, Tensor neg_one, Tensor y0, bool relu, float slope, int cfg) -> Tensor");
  m.def("conv_wino_fwd(Tensor x, Tensor u, Tensor? scale, Tensor? shift, bool relu, bool pool, int splits, "
        "bool staged=True, Tensor(a!)? apoz=None) -> (Tensor, Tensor)");
  m.def("conv_wino_dgrad(Tensor g, Tensor? g_argmax, Tensor ut, Tensor act, Tensor? bn_scale, "
        "Tensor(a!)? taylor, bool want_out, int splits, bool staged=True, int tay_mode=0) -> Tensor");
  m.def("wino4_weights(Tensor w, bool flip_t, int K=0, int C=0) -> Tensor");
  m.def("conv_wino4_fwd(Tensor x, Tensor u, Tensor? scale, Tensor? shift, bool relu, bool pool, "
        "Tensor(a!)? apoz=None, int splits=1, int variant=0, int ko=0) -> (Tensor, Tensor)");
  m.def("conv_wino4_dgrad(Tensor g, Tensor ut, Tensor act, Tensor? bn_scale, Tensor(a!)? taylor, bool want_out, "
        "int tay_mode=0, int splits=1, int variant=0, Tensor? unpool_am=None) -> Tensor");
}

void register_engine_ops_impl(torch::Library& m) {
  m.impl("conv_fwd", &conv_fwd);
  m.impl("conv_dgrad", &conv_dgrad);
  m.impl("conv2x2_fast_fwd", &conv2x2_fast_fwd);
  m.impl("conv2x2_fast_dgrad", &conv2x2_fast_dgrad);
  m.impl("conv_first", &conv_first);
  m.impl("prefix_tri_operands", &prefix_tri_operands);
  m.impl("wino_weights", &wino_weights);
  m.impl("prefix_delta", &prefix_delta);
  m.impl("conv_wino_fwd", &conv_wino_fwd);
  m.impl("nchw_to_nhwc_pad", &nchw_to_nhwc_pad);
  m.impl("maxpool2_nhwc", &maxpool2_nhwc);
  m.impl("maxpool_nhwc", &maxpool_nhwc);
  m.impl("avgpool_nhwc", &avgpool_nhwc);
  m.impl("conv_gen", &conv_gen);
  m.impl("conv_gen_bwd", &conv_gen_bwd);
  m.impl("conv_gen_bwd_bn", &conv_gen_bwd_bn);
  m.impl("conv_wgrad", &conv_wgrad);
  m.impl("pack_conv_weight", &pack_conv_weight);
  m.impl("pack_conv_weights_multi", &pack_conv_weights_multi);
  m.impl("wino4_weights_multi", &wino4_weights_multi);
  m.impl("conv_gen_stats", &conv_gen_stats);
  m.impl("wino_wgrad", &wino_wgrad);
  m.impl("bn_train_fwd", &bn_train_fwd);
  m.impl("bn_train_bwd", &bn_train_bwd);
  m.impl("bn_hswish_fwd", &bn_hswish_fwd);
  m.impl("bn_hswish_bwd", &bn_hswish_bwd);
  m.impl("unpool2_nhwc", &unpool2_nhwc);
  m.impl("conv_wino_dgrad", &conv_wino_dgrad);
  m.impl("wino4_weights", &wino4_weights);
  m.impl("conv_wino4_fwd", &conv_wino4_fwd);
  m.impl("conv_wino4_dgrad", &conv_wino4_dgrad);
}
