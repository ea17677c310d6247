// C launchers exported by csrc/kernels/*.hip (no torch types cross this boundary). The only place a
// launcher is declared: every kernel file includes this header, so a definition that disagrees with its
// declaration does not compile, and every caller (the bindings, csrc/tests) sees the same signature.
// The contracts are documented at the definitions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// batchnorm.hip (Cr <= C: the channels that carry parameters; Cr = C when no width is carried)
int tp_bn_groups(int P, int C);
hipError_t tp_bn_fwd_train(const float* x, float* y, int P, int C, int Cr, const float* gamma, const float* beta,
                           float eps, float momentum, float* run_mean, float* run_var, float* mean, float* invstd,
                           float* a, float* b, double* ws, const float* res, int relu, uint8_t* mko, long long* nbt,
                           hipStream_t st);
hipError_t tp_bn_fwd_train_pre(const float* x, float* y, int P, int C, int Cr, const float* gamma, const float* beta,
                               float eps, float momentum, float* run_mean, float* run_var, float* mean, float* invstd,
                               float* a, float* b, double* ws, const double* pre, int G, const float* res, int relu,
                               uint8_t* mko, long long* nbt, hipStream_t st);
hipError_t tp_bn_bwd_train(const float* g, const float* x, float* dx, int P, int C, int Cr, const float* gamma,
                           const float* mean, const float* invstd, float* dgamma, float* dbeta, float* a, float* k1,
                           float* k2, double* ws, const float* ym, float* dres, const uint8_t* mk, hipStream_t st);
hipError_t tp_bn_bwd_train_pre(const float* g, const float* x, float* dx, int P, int C, int Cr, const float* gamma,
                               const float* mean, const float* invstd, float* dgamma, float* dbeta, float* a,
                               float* k1, float* k2, double* ws, const double* pre, int G, const float* ym,
                               float* dres, const uint8_t* mk, hipStream_t st);
// y = hardswish(BN(x)) and its backward (af / bf: the forward's a / b; no mask, no residual)
hipError_t tp_bn_hswish_fwd_train(const float* x, float* y, int P, int C, int Cr, const float* gamma,
                                  const float* beta, float eps, float momentum, float* run_mean, float* run_var,
                                  float* mean, float* invstd, float* a, float* b, double* ws, long long* nbt,
                                  hipStream_t st);
hipError_t tp_bn_hswish_bwd_train(const float* g, const float* x, float* dx, int P, int C, int Cr, const float* gamma,
                                  const float* mean, const float* invstd, const float* af, const float* bf,
                                  float* dgamma, float* dbeta, float* a, float* k1, float* k2, double* ws,
                                  hipStream_t st);
// channel_reduce.hip
hipError_t tp_channel_reduce(const float* act, const float* grad, float* out, float* ws, int B, int C, int S,
                             int mode, int channels_last, hipStream_t st);
int tp_channel_reduce_ws_elems(int B, int C, int S, int channels_last);  // -1: bad sizes / 2^31 elements and more
int tp_channel_reduce_chunks(int B, int C, int S, int vec);
hipError_t tp_column_accumulate(const float* v, double* acc_sum, double* acc_sq, int B, int C, hipStream_t st);
int tp_score_fold_ws_elems(const int* B, const int* C, int count);
hipError_t tp_score_fold_multi(float* const* T, double* const* acc, const int* B, const int* C, const int* R,
                               int count, int take_abs, int after, double* ws, hipStream_t st);
// conv2x2_fast.hip: 3x3 / pad-1 conv on 2x2 maps as 9 channel products (u9 (9, Cout, Cin) = G w G^T);
// V (9, B, Cin) and slabs (9 * splits, B, Cout) are workspaces
hipError_t tp_conv2x2_fast_fwd(const float* x, const float* u9, int B, int C, int K, int cfg, int splits,
                               const float* scale, const float* shift, int relu, int pool, float* out,
                               uint8_t* out_argmax, float* V, float* slabs, hipStream_t st);
hipError_t tp_conv2x2_fast_dgrad(const float* g, const uint8_t* g_argmax, const float* u9t, int B, int Cg, int Cin,
                                 int cfg, int splits, const float* act, const float* bn_scale, float* taylor,
                                 int tay_mode, float* out, float* V, float* slabs, hipStream_t st);
// conv_mfma.hip
hipError_t tp_conv_igemm(const float* x, const uint8_t* x_argmax, const float* w, int B, int H, int W, int Cin,
                         int Cout, int ks, int pooled_m, int unpool, int epi, int cfg, int splits, const float* scale,
                         const float* shift, int relu, float* out, uint8_t* out_argmax, const float* act,
                         float* taylor, int HWo, int tay_group, float* ws, int tay_mode, float* apoz, float slope,
                         hipStream_t st);
// nbatch independent GEMMs slab[i * splits + s] (M, N) = K range s of x[i] (M, K) . w[i] (N, K)^T
int tp_conv_norm_splits(int splits, int K);
hipError_t tp_conv_igemm_batched(const float* x, const float* w, int nbatch, int M, int K, int N, int cfg, int splits,
                                 float* slabs, hipStream_t st);
hipError_t tp_conv_epilogue_slabs(const float* ws, int splits, int B, int H, int W, int K, int epi, const float* scale,
                                  const float* shift, int relu, float* out, uint8_t* out_argmax, const float* act,
                                  float* taylor, float* apoz, int tay_mode, hipStream_t st);
hipError_t tp_conv_first_wave(const float* x, const float* wt, const float* scale, const float* shift, float* out,
                              int B, int Cin, int H, int W, int Cout, int relu, hipStream_t st);
hipError_t tp_conv_first_direct(const float* x, const float* w, const float* scale, const float* shift, float* out,
                                int B, int Cin, int H, int W, int Cout, int relu, hipStream_t st);
hipError_t tp_nchw_to_nhwc_pad(const float* x, float* y, int B, int C, int H, int W, int Cp, hipStream_t st);
long long tp_conv_sk_ws_floats(int cfg, int ks, int transposed, int tay, int M, int N);
int tp_conv_gen_k(int ks, int Cin);
hipError_t tp_prefix_delta_gemm(const float* T, const float* Wsub, const float* neg_one, const float* Y0, int M,
                                int Kc, int N, int B0, int relu, float slope, int cfg, float* out, hipStream_t st);
int tp_conv_tile_m(int cfg);
int tp_conv_gen_tay_slots(int cfg, int HWo);
// a plain forward conv passes transposed = Ho_t = Wo_t = 0, res_stride = 1, tay_mode = 0 and null for mask,
// bnpart, tay_part, res_bits and the bnb_* pointers
hipError_t tp_conv_gen(const float* x, const float* w, int B, int H, int W, int Cin, int Cout, int ks, int stride,
                       int pad, int transposed, int Ho_t, int Wo_t, int cfg, int splits, const float* scale,
                       const float* shift, int relu, const float* res, int res_stride, const float* mask, float* apoz,
                       float* out, float* ws, double* bnpart, float* tay_part, int tay_mode, const uint8_t* res_bits,
                       const float* bnb_y, const float* bnb_mean, const float* bnb_invstd, const uint8_t* bnb_bits,
                       hipStream_t st);
// conv_wgrad.hip (no parameter-layout output: fin = null, fin_co = fin_ci = 0, fs = null; one GEMM: batch = 1,
// g_bstride = x_bstride = 0)
hipError_t tp_conv_wgrad(const float* g, const float* x, float* dw, float* ws, int B, int H, int W, int Cin, int Cout,
                         int ks, int stride, int pad, int Kpad, int cfg, int splits, float* fin, int fin_co,
                         int fin_ci, const long long* fs, int batch, long long g_bstride, long long x_bstride,
                         hipStream_t st);
// data_ops.hip
hipError_t tp_augment_u8(const uint8_t* src, const int64_t* idx, const int* aug, int B, int C, int H, int W, int pad,
                         const float* mean, const float* inv_std, float* out, hipStream_t st);
// dwconv.hip: activations of C channels per pixel, a parameter of Cw <= C (C % 4 == 0 when Cw < C; Cw = C when
// no width is carried)
hipError_t tp_dwconv_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int C,
                         int Cw, int k, int s, int pad, hipStream_t st);
hipError_t tp_dwconv_dgrad(const float* g, const float* w, float* dx, int B, int H, int W, int C, int Cw, int k,
                           int s, int pad, hipStream_t st);
int tp_dwconv_wgrad_chunks(int P, int C);
hipError_t tp_dwconv_wgrad(const float* g, const float* x, float* dw, float* db, double* ws, int chunks, int B,
                           int H, int W, int C, int Cw, int k, int s, int pad, long long s0, long long s2,
                           long long s3, hipStream_t st);
// dwconv_act.hip (C % 4 == 0; activation codes 0 none, 1 ReLU, 2 ReLU6)
hipError_t tp_dwconv_act_fwd(const float* x, const float* w, const float* scale, const float* shift, float* y,
                             float* apoz, int B, int H, int W, int C, int k, int s, int pad, int in_act, int out_act,
                             hipStream_t st);
int tp_dwconv_act_tay_slots(int H, int W, int C);
hipError_t tp_dwconv_act_dgrad(const float* g, const float* y, const float* w, const float* scale, const float* z,
                               float* dz, float* tay, int R, int tay_mode, int B, int H, int W, int C, int k, int s,
                               int pad, int in_act, int out_act, hipStream_t st);
// the same with code 3 (Hardswish) on either side; pre (optional): the output's pre-activation, which is
// the y operand of the dgrad when out_act == 3
hipError_t tp_dwconv_hs_fwd(const float* x, const float* w, const float* scale, const float* shift, float* y,
                            float* apoz, float* pre, int B, int H, int W, int C, int k, int s, int pad, int in_act,
                            int out_act, hipStream_t st);
int tp_dwconv_hs_tay_slots(int H, int W, int C);
hipError_t tp_dwconv_hs_dgrad(const float* g, const float* y, const float* w, const float* scale, const float* z,
                              float* dz, float* tay, int R, int tay_mode, int B, int H, int W, int C, int k, int s,
                              int pad, int in_act, int out_act, hipStream_t st);
// prefix_project.hip: out[0] = base, out[j] = out[j-1] - (a[:, c] - fill[c]) (x) wt[c, :], c = perm[p0+j-1]
// (base (N, Co), a (N, C), fill (C), wt (C, Co), perm (n <= C), out (cnt, N, Co); Co % 4 == 0)
hipError_t tp_prefix_project(const float* base, const float* a, const float* fill, const float* wt, const int* perm,
                             float* out, int N, int C, int Co, int n, int p0, int cnt, hipStream_t st);
// prune_ops.hip
hipError_t tp_channel_fill(float* x, long long B, int C, long long S, const int64_t* idx, int nidx, float value,
                           hipStream_t st);
hipError_t tp_nan_channels(const float* x, long long B, int C, long long S, uint8_t* flags, hipStream_t st);
hipError_t tp_gather_multi(const void* const* srcs, void* const* dsts, const long long* outer, const long long* n,
                           const long long* inner, int count, int elsize, const int64_t* keep, long long nkeep,
                           hipStream_t st);
hipError_t tp_maxpool2_nhwc(const float* x, float* y, uint8_t* am, int B, int H, int W, int C, hipStream_t st);
hipError_t tp_unpool2_nhwc(const float* g, const uint8_t* am, float* out, int B, int H, int W, int C, hipStream_t st);
hipError_t tp_maxpool_nhwc(const float* x, float* y, int B, int H, int W, int C, int k, int s, int pad,
                           hipStream_t st);
hipError_t tp_avgpool_nhwc(const float* x, float* y, int B, int HW, int C, hipStream_t st);
// shapley.hip
hipError_t tp_prefix_mask(const float* z, float* out, const int* rank, long long N, int C, int S, int channels_last,
                          int p0, int K, hipStream_t st);
hipError_t tp_shapley_scatter(const float* L, const int* perm, double* sv, int row0, int B, int n, int k0, int K,
                              double scale, hipStream_t st);
hipError_t tp_shapley_column(const float* L, const int* perm, double* sv_col, int B, int k0, int K, double scale,
                             hipStream_t st);
hipError_t tp_cross_entropy(const float* logits, const int64_t* target, float* loss, float* grad, int B, int NC,
                            float gscale, hipStream_t st);
hipError_t tp_prefix_tri_operands(const float* z, const float* W, const int* perm, int B, int C, int N, int p0,
                                  int cnt, int Kc, float* T, float* Wsub, hipStream_t st);
// squeeze_excite.hip: out = x * s, s = gate(W2 . relu(W1 . mean_hw(x) + b1) + b2) on x (B, HW, C);
// gate 0 Hardsigmoid, 1 Sigmoid; w1 (Cs, C), w2 (C, Cs) row-major; ws: splits * B * C floats when
// splits = tp_se_splits(B, HW, C) > 1
int tp_se_splits(int B, int HW, int C);
hipError_t tp_se_pool(const float* x, float* p, float* ws, int splits, int B, int HW, int C, hipStream_t st);
hipError_t tp_se_gate_fwd(const float* p, const float* w1, const float* b1, const float* w2, const float* b2,
                          float* h, float* s, int B, int C, int Cs, int gate, hipStream_t st);
hipError_t tp_se_scale(const float* x, const float* s, float* out, int B, int HW, int C, hipStream_t st);
hipError_t tp_se_bwd_reduce(const float* g, const float* x, float* ds, float* ws, int splits, int B, int HW, int C,
                            hipStream_t st);
hipError_t tp_se_gate_bwd(const float* ds, const float* s, const float* h, const float* w1, const float* w2,
                          float* dz2, float* dz1, float* dp, int B, int C, int Cs, int gate, hipStream_t st);
hipError_t tp_se_bwd_dx(const float* g, const float* s, const float* dp, float* dx, int B, int HW, int C,
                        hipStream_t st);
hipError_t tp_se_wgrad(const float* a, const float* m, float* dw, float* db, int B, int R, int K, long long s0,
                       long long s1, hipStream_t st);
// train_ops.hip
void tp_philox4x32(unsigned long long ctr, unsigned long long key, unsigned* out);  // host: the dropout generator
hipError_t tp_dropout(const float* x, float* y, long long n, unsigned long long seed, double p, hipStream_t st);
hipError_t tp_maxpool_fwd_arg(const float* x, float* y, uint8_t* am, int B, int H, int W, int C, int k, int s, int pad,
                              hipStream_t st);
hipError_t tp_maxpool_bwd(const float* g, const uint8_t* am, float* dx, int B, int H, int W, int C, int k, int s,
                          int pad, hipStream_t st);
hipError_t tp_avgpool_bwd(const float* g, float* dx, int B, int HW, int C, hipStream_t st);
// weight_pack.hip
hipError_t tp_pack_conv_weights_multi(const long long* desc, int n, long long total, hipStream_t st);
hipError_t tp_pack_conv_weight(const float* w, float* out, int O, int I, int KS, int rows, int cols, int cpad,
                               int mode, hipStream_t st);
// wino4.hip (tp_conv_wino4: ko = 0 stores all K output channels)
hipError_t tp_wino4_weights_strided(const float* w, float* u, int K, int C, int flip_t, int S0, int S1,
                                    long long st0, long long st1, int st2, int st3, hipStream_t st);
hipError_t tp_wino4_weights_multi(const long long* desc, int n, long long total, hipStream_t st);
hipError_t tp_wino4_weights(const float* w, float* u, int K, int C, int flip_t, int S0, int S1, hipStream_t st);
int tp_wino4_u_img();
int tp_wino4_ok(int H, int W, int C, int K);
int tp_wino4_taylor_slots(int S);
hipError_t tp_conv_wino4(const float* x, const float* u, int B, int S, int C, int K, int epi, const float* scale,
                         const float* shift, int relu, float* out, uint8_t* out_argmax, const float* act,
                         float* taylor, float* apoz, int tay_mode, int splits, float* ws, int variant, hipStream_t st,
                         const uint8_t* unpool_am, int ko);
int tp_wino4_lds_bytes(int S, int variant);
// wino_wgrad.hip
long long tp_wino_wgrad_ws_elems(int B, int H, int W, int Cin, int Cout, int splits);
hipError_t tp_wino_wgrad(const float* g, const float* x, float* ws, int B, int H, int W, int Cin, int Cout, int cfg,
                         int splits, float* fin, int fin_co, int fin_ci, const long long* fs, hipStream_t st);
// winograd.hip (tp_wino_weights: a weight already padded to the GEMM has S0 x S1 = K x C, flipped C x K)
int tp_wino_taylor_slots(int H, int W);
hipError_t tp_wino_weights(const float* w, float* u, int K, int C, int flip_t, int S0, int S1, hipStream_t st);
hipError_t tp_wino_weights_bf16(const float* w, void* u, int K, int C, int flip_t, int S0, int S1, hipStream_t st);
int tp_wino_lds_bytes();
int tp_wino_staged_ok(int H, int W, int unpool);
void tp_wino_geometry(int H, int W, int unpool, int* out9);
hipError_t tp_conv_wino(const float* x, const uint8_t* x_argmax, const float* u, int B, int H, int W, int C, int K,
                        int unpool, int epi, int splits, int staged, const float* scale, const float* shift, int relu,
                        float* out, uint8_t* out_argmax, const float* act, float* taylor, float* apoz, float* ws,
                        int tay_mode, hipStream_t st);
}

// the torch side of the extension (bindings.cpp / engine_bindings.cpp), not a C launcher
namespace torch { class Library; }
void register_engine_ops_def(torch::Library& m);
void register_engine_ops_impl(torch::Library& m);
