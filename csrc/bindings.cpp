// torch.ops.tpamd.* registrations for the gfx950 kernels: the TORCH_LIBRARY block and the pruning,
// attribution, training, depthwise and squeeze-excite ops (the conv / GEMM / BN engine ops are in
// engine_bindings.cpp). Only these two translation units see torch headers; kernels live in
// csrc/kernels/*.hip behind C launchers. Every op validates device/dtype/layout and throws
// (TORCH_CHECK) instead of silently falling back: on a GPU box the HIP path is the one that runs, or
// the call fails. The checks both files share are in tp_bind.h.
#include "tp_bind.h"

namespace {

// Returns (B, C, S) and whether the tensor is channels_last. Accepts (B,C), (B,C,*) contiguous,
// or 4D channels_last.
struct BCS {
  int64_t B, C, S;
  bool cl;
};
BCS bcs_of(const at::Tensor& t) {
  TORCH_CHECK(t.dim() >= 2, "expected a (B, C, ...) tensor, got dim ", t.dim());
  BCS r{t.size(0), t.size(1), 1, false};
  for (int64_t d = 2; d < t.dim(); ++d) r.S *= t.size(d);
  if (t.is_contiguous()) return r;
  if (t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast)) {
    r.cl = true;
    return r;
  }
  TORCH_CHECK(false, "tensor must be contiguous (NCHW) or channels_last");
  return r;
}

at::Tensor channel_reduce(const c10::optional<at::Tensor>& act, const c10::optional<at::Tensor>& grad,
                          int64_t mode) {
  const at::Tensor& ref = act.has_value() ? *act : *grad;
  TORCH_CHECK(act.has_value() || grad.has_value(), "channel_reduce needs act or grad");
  need(ref, "input");
  BCS s = bcs_of(ref);
  if (act.has_value() && grad.has_value()) {
    TORCH_CHECK(act->sizes() == grad->sizes(), "act/grad shape mismatch");
    BCS s2 = bcs_of(*grad);
    TORCH_CHECK(s2.cl == s.cl, "act/grad layout mismatch");
    need(*grad, "grad");
  }
  const bool need_a = (mode == 0 || mode == 1 || mode == 3);
  const bool need_g = (mode != 3);
  TORCH_CHECK(!need_a || act.has_value(), "mode ", mode, " needs the activation");
  TORCH_CHECK(!need_g || grad.has_value(), "mode ", mode, " needs the gradient");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ref.device());
  auto out = at::empty({s.B, s.C}, ref.options());
  if (out.numel() == 0) return out;
  const int64_t lim = int64_t(1) << 31;
  TORCH_CHECK(s.B < lim && s.C < lim && s.S > 0 && s.S < lim, "channel_reduce: empty or oversized (B, C, S)");
  if (act.has_value() && grad.has_value()) TORCH_CHECK(act->device() == grad->device(), "act/grad device mismatch");
  const int wse = tp_channel_reduce_ws_elems((int)s.B, (int)s.C, (int)s.S, s.cl ? 1 : 0);
  TORCH_CHECK(wse >= 0, "channel_reduce: workspace of 2^31 elements or more");
  at::Tensor ws;
  if (wse > 0) ws = at::empty({wse}, ref.options());
  TP_CHECK_HIP(tp_channel_reduce(need_a ? act->data_ptr<float>() : nullptr,
                                 need_g ? grad->data_ptr<float>() : nullptr, out.data_ptr<float>(),
                                 wse > 0 ? ws.data_ptr<float>() : nullptr, (int)s.B, (int)s.C, (int)s.S, (int)mode,
                                 s.cl ? 1 : 0, cur_stream()));
  return out;
}

void column_accumulate(const at::Tensor& v, at::Tensor& acc_sum, const c10::optional<at::Tensor>& acc_sq) {
  need(v, "v");
  TORCH_CHECK(v.dim() == 2 && v.is_contiguous(), "v must be contiguous (B, C)");
  TORCH_CHECK(acc_sum.device() == v.device() && acc_sum.scalar_type() == at::kDouble &&
                  acc_sum.numel() == v.size(1) && acc_sum.is_contiguous(),
              "acc_sum must be a contiguous float64 (C,) tensor on v's device");
  double* sq = nullptr;
  if (present(acc_sq)) {
    TORCH_CHECK(acc_sq->device() == v.device() && acc_sq->scalar_type() == at::kDouble &&
                    acc_sq->numel() == v.size(1) && acc_sq->is_contiguous(),
                "acc_sq must be a contiguous float64 (C,) tensor on v's device");
    sq = acc_sq->data_ptr<double>();
  }
  if (v.numel() == 0) return;
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  TP_CHECK_HIP(tp_column_accumulate(v.data_ptr<float>(), acc_sum.data_ptr<double>(), sq, (int)v.size(0),
                                    (int)v.size(1), cur_stream()));
}

// For every i: T[i] is (B, C) or (R, B, C) partial slots summed in slot order;
// v = |sum| (or sum); acc[i] += v.sum(0) (acc[i] may be empty = skip);
// after: 0 leave T, 1 write v back (slot 0; other slots zeroed), 2 zero T. One launch per 16 tensors.
void score_fold_(at::TensorList T, at::TensorList acc, bool take_abs, int64_t after) {
  TORCH_CHECK(T.size() == acc.size(), "one accumulator per score tensor");
  if (T.empty()) return;
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(T[0].device());
  std::vector<float*> tp;
  std::vector<double*> ap;
  std::vector<int> bs, cs, rs;
  auto flush = [&]() {
    if (tp.empty()) return;
    const int n_ws = tp_score_fold_ws_elems(bs.data(), cs.data(), (int)tp.size());
    TORCH_CHECK(n_ws >= 0, "score_fold_: empty slab or a workspace of 2^31 elements or more");
    at::Tensor ws = at::empty({std::max(n_ws, 1)}, T[0].options().dtype(at::kDouble));
    TP_CHECK_HIP(tp_score_fold_multi(tp.data(), ap.data(), bs.data(), cs.data(), rs.data(), (int)tp.size(),
                                     take_abs ? 1 : 0, (int)after, ws.data_ptr<double>(), cur_stream()));
    tp.clear(); ap.clear(); bs.clear(); cs.clear(); rs.clear();
  };
  for (size_t i = 0; i < T.size(); ++i) {
    need(T[i], "T");
    TORCH_CHECK(T[i].device() == T[0].device(), "score tensors must share a device");
    TORCH_CHECK((T[i].dim() == 2 || T[i].dim() == 3) && T[i].is_contiguous(),
                "T must be contiguous (B, C) or (R, B, C) partial slots");
    const int64_t nb = T[i].size(-2), nc = T[i].size(-1), nr = T[i].dim() == 3 ? T[i].size(0) : 1;
    double* a = nullptr;
    if (acc[i].defined() && acc[i].numel() > 0) {
      TORCH_CHECK(acc[i].device() == T[i].device() && acc[i].scalar_type() == at::kDouble &&
                      acc[i].is_contiguous() && acc[i].numel() == nc,
                  "acc must be a contiguous float64 (C,) tensor on T's device");
      a = acc[i].data_ptr<double>();
    }
    tp.push_back(T[i].data_ptr<float>());
    ap.push_back(a);
    bs.push_back((int)nb);
    cs.push_back((int)nc);
    rs.push_back((int)nr);
    if (tp.size() == 16) flush();
  }
  flush();
}

void channel_fill_(at::Tensor& x, const at::Tensor& idx, double value) {
  need(x, "x");
  TORCH_CHECK(x.is_contiguous(), "channel_fill_ needs a contiguous NC* tensor");
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.device() == x.device() && idx.dim() == 1,
              "idx must be int64 (n,) on x's device");
  BCS s = bcs_of(x);
  if (x.numel() == 0 || idx.numel() == 0) return;
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto ic = idx.contiguous();
  TP_CHECK_HIP(tp_channel_fill(x.data_ptr<float>(), s.B, (int)s.C, s.S, ic.data_ptr<int64_t>(), (int)ic.numel(),
                               (float)value, cur_stream()));
}

at::Tensor nan_channels(const at::Tensor& x_) {
  need(x_, "x");
  auto x = x_.contiguous();
  BCS s = bcs_of(x);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  if (x.numel() == 0) return at::zeros({s.C}, x.options().dtype(at::kByte));
  auto flags = at::empty({s.C}, x.options().dtype(at::kByte));
  TP_CHECK_HIP(tp_nan_channels(x.data_ptr<float>(), s.B, (int)s.C, s.S, flags.data_ptr<uint8_t>(), cur_stream()));
  return flags;
}

std::vector<at::Tensor> gather_multi(at::TensorList srcs, at::IntArrayRef axes, const at::Tensor& keep_) {
  TORCH_CHECK(srcs.size() == axes.size(), "one axis per tensor");
  TORCH_CHECK(keep_.scalar_type() == at::kLong && keep_.dim() == 1, "keep must be int64 (k,)");
  std::vector<at::Tensor> outs;
  outs.reserve(srcs.size());
  if (srcs.empty()) return outs;
  auto keep = keep_.to(srcs[0].device()).contiguous();
  const int64_t nkeep = keep.numel();
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(srcs[0].device());
  // Group tensors with equal element size into launches of up to 8 descriptors.
  std::vector<at::Tensor> csrc;
  for (size_t i = 0; i < srcs.size(); ++i) {
    TORCH_CHECK(srcs[i].is_cuda() && srcs[i].device() == srcs[0].device(),
                "gather_multi inputs must be GPU tensors on one device");
    auto c = srcs[i].contiguous();
    int64_t ax = axes[i] < 0 ? axes[i] + c.dim() : axes[i];
    TORCH_CHECK(ax >= 0 && ax < c.dim(), "bad axis");
    auto sz = c.sizes().vec();
    sz[ax] = nkeep;
    outs.push_back(at::empty(sz, c.options()));
    csrc.push_back(c);
  }
  for (int es : {1, 2, 4, 8}) {
    std::vector<const void*> s;
    std::vector<void*> d;
    std::vector<long long> outer, n, inner;
    auto flush = [&]() {
      if (s.empty()) return;
      TP_CHECK_HIP(tp_gather_multi(s.data(), d.data(), outer.data(), n.data(), inner.data(), (int)s.size(), es,
                                   keep.data_ptr<int64_t>(), nkeep, cur_stream()));
      s.clear(); d.clear(); outer.clear(); n.clear(); inner.clear();
    };
    for (size_t i = 0; i < csrc.size(); ++i) {
      if ((int)csrc[i].element_size() != es || outs[i].numel() == 0) continue;
      const auto& c = csrc[i];
      int64_t ax = axes[i] < 0 ? axes[i] + c.dim() : axes[i];
      long long o = 1, in = 1;
      for (int64_t k = 0; k < ax; ++k) o *= c.size(k);
      for (int64_t k = ax + 1; k < c.dim(); ++k) in *= c.size(k);
      s.push_back(c.data_ptr());
      d.push_back(outs[i].data_ptr());
      outer.push_back(o);
      n.push_back(c.size(ax));
      inner.push_back(in);
      if (s.size() == 8) flush();
    }
    flush();
  }
  return outs;
}

at::Tensor prefix_mask(const at::Tensor& z, const at::Tensor& rank, int64_t p0, int64_t K) {
  need(z, "z");
  TORCH_CHECK(rank.scalar_type() == at::kInt && rank.device() == z.device() && rank.dim() == 1 && rank.is_contiguous(),
              "rank must be a contiguous int32 (C,) tensor on z's device");
  BCS s = bcs_of(z);
  TORCH_CHECK(rank.numel() == s.C, "rank length must equal channel count");
  TORCH_CHECK(p0 >= 0 && K >= 0 && p0 + K < (int64_t(1) << 31) && s.C < (int64_t(1) << 31) && s.S < (int64_t(1) << 31),
              "bad prefix range (p0 ", p0, ", K ", K, ")");
  auto sz = z.sizes().vec();
  sz[0] = sz[0] * K;
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(z.device());
  auto out = at::empty(sz, z.options().memory_format(s.cl ? at::MemoryFormat::ChannelsLast
                                                            : at::MemoryFormat::Contiguous));
  if (out.numel() == 0) return out;
  TP_CHECK_HIP(tp_prefix_mask(z.data_ptr<float>(), out.data_ptr<float>(), rank.data_ptr<int>(), z.numel(), (int)s.C,
                              (int)s.S, s.cl ? 1 : 0, (int)p0, (int)K, cur_stream()));
  return out;
}

// out[0] = base, out[j] = out[j-1] - (a[:, c] - fill[c]) (x) wt[c, :], c = perm[p0 + j - 1]: the cnt stacked outputs
// of a 1x1 project conv whose input copies differ by one filled channel each (csrc/kernels/prefix_project.hip)
at::Tensor prefix_project(const at::Tensor& base, const at::Tensor& a, const at::Tensor& fill, const at::Tensor& wt,
                          const at::Tensor& perm, int64_t p0, int64_t cnt) {
  need(base, "base");
  need(a, "a");
  need(fill, "fill");
  need(wt, "wt");
  TORCH_CHECK(base.dim() == 2 && base.is_contiguous() && base.numel() > 0, "base must be a non-empty contiguous (N, Co)");
  const int64_t N = base.size(0), Co = base.size(1);
  TORCH_CHECK(a.dim() == 2 && a.is_contiguous() && a.size(0) == N && a.size(1) > 0, "a must be a contiguous (N, C)");
  const int64_t C = a.size(1);
  TORCH_CHECK(fill.dim() == 1 && fill.is_contiguous() && fill.numel() == C, "fill must be a contiguous (C,)");
  TORCH_CHECK(wt.dim() == 2 && wt.is_contiguous() && wt.size(0) == C && wt.size(1) == Co,
              "wt must be a contiguous (C, Co)");
  TORCH_CHECK(perm.scalar_type() == at::kInt && perm.is_cuda() && perm.dim() == 1 && perm.is_contiguous(),
              "perm must be a contiguous int32 (n,) GPU tensor");
  TORCH_CHECK(a.device() == base.device() && fill.device() == base.device() && wt.device() == base.device() &&
                  perm.device() == base.device(), "operands must share a device");
  const int64_t n = perm.numel(), lim = int64_t(1) << 31;
  TORCH_CHECK(Co % 4 == 0, "prefix_project needs Co % 4 == 0");
  TORCH_CHECK(n <= C && cnt >= 1 && p0 >= 0 && p0 + cnt - 1 <= n, "bad prefix range (p0 ", p0, ", cnt ", cnt, ", n ", n,
              ", C ", C, ")");
  TORCH_CHECK(N < lim && C < lim && Co < lim && cnt < lim && N * Co * 4 < lim && N * Co * 4 * cnt < lim,
              "prefix_project operands must stay below 2^31 bytes");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(base.device());
  auto out = at::empty({cnt, N, Co}, base.options());
  TP_CHECK_HIP(tp_prefix_project(base.data_ptr<float>(), a.data_ptr<float>(), fill.data_ptr<float>(),
                                 wt.data_ptr<float>(), perm.data_ptr<int>(), out.data_ptr<float>(), (int)N, (int)C,
                                 (int)Co, (int)n, (int)p0, (int)cnt, cur_stream()));
  return out;
}

void shapley_scatter(const at::Tensor& L, const at::Tensor& perm, at::Tensor& sv, int64_t row0, int64_t k0,
                     double scale) {
  need(L, "losses");
  TORCH_CHECK(L.dim() == 2 && L.is_contiguous(), "losses must be contiguous (K+1, B)");
  TORCH_CHECK(perm.scalar_type() == at::kInt && perm.is_contiguous() && perm.device() == L.device(),
              "perm must be int32 on the losses' device");
  TORCH_CHECK(sv.scalar_type() == at::kDouble && sv.dim() == 2 && sv.is_contiguous() && sv.device() == L.device(),
              "sv must be float64 (d, n) on the losses' device");
  const int64_t K = L.size(0) - 1, B = L.size(1);
  TORCH_CHECK(K >= 0 && row0 >= 0 && k0 >= 0 && row0 + B <= sv.size(0) && k0 + K <= perm.numel() &&
                  perm.numel() == sv.size(1), "shape mismatch");
  TORCH_CHECK(L.numel() < (int64_t(1) << 31) && sv.size(0) < (int64_t(1) << 31) && sv.size(1) < (int64_t(1) << 31),
              "shapley_scatter operands must stay below 2^31 elements per dimension");
  if (K == 0 || B == 0) return;
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(L.device());
  TP_CHECK_HIP(tp_shapley_scatter(L.data_ptr<float>(), perm.data_ptr<int>(), sv.data_ptr<double>(), (int)row0,
                                  (int)B, (int)sv.size(1), (int)k0, (int)K, scale, cur_stream()));
}

void shapley_column(const at::Tensor& L, const at::Tensor& perm, at::Tensor& sv_col, int64_t k0, double scale) {
  need(L, "losses");
  TORCH_CHECK(L.dim() == 2 && L.is_contiguous(), "losses must be contiguous (K+1, B)");
  TORCH_CHECK(perm.scalar_type() == at::kInt && perm.is_contiguous() && perm.device() == L.device(),
              "perm must be int32 on the losses' device");
  TORCH_CHECK(sv_col.scalar_type() == at::kDouble && sv_col.is_contiguous() && sv_col.device() == L.device(),
              "sv_col must be float64 (n,) on the losses' device");
  const int64_t K = L.size(0) - 1;
  TORCH_CHECK(K >= 0 && k0 >= 0 && k0 + K <= perm.numel() && perm.numel() == sv_col.numel(), "shape mismatch");
  TORCH_CHECK(L.numel() < (int64_t(1) << 31) && perm.numel() < (int64_t(1) << 31),
              "shapley_column operands must stay below 2^31 elements");
  if (K == 0 || L.size(1) == 0) return;
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(L.device());
  TP_CHECK_HIP(tp_shapley_column(L.data_ptr<float>(), perm.data_ptr<int>(), sv_col.data_ptr<double>(),
                                 (int)L.size(1), (int)k0, (int)K, scale, cur_stream()));
}

std::tuple<at::Tensor, at::Tensor> cross_entropy(const at::Tensor& logits_, const at::Tensor& target_,
                                                 double gscale, bool want_grad) {
  need(logits_, "logits");
  TORCH_CHECK(logits_.dim() == 2, "logits must be (B, classes)");
  auto logits = logits_.contiguous();
  TORCH_CHECK(target_.device() == logits_.device(), "target must be on the logits' device");
  auto target = target_.to(at::kLong).contiguous();
  TORCH_CHECK(target.numel() == logits.size(0), "target length mismatch");
  TORCH_CHECK(logits.size(1) > 0 && logits.size(1) < (int64_t(1) << 31), "logits need at least one class");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  auto loss = at::empty({logits.size(0)}, logits.options());
  at::Tensor grad = want_grad ? at::empty_like(logits) : at::Tensor();
  if (logits.size(0) == 0) return {loss, grad};
  TP_CHECK_HIP(tp_cross_entropy(logits.data_ptr<float>(), target.data_ptr<int64_t>(), loss.data_ptr<float>(),
                                want_grad ? grad.data_ptr<float>() : nullptr, (int)logits.size(0),
                                (int)logits.size(1), (float)gscale, cur_stream()));
  return {loss, grad};
}

// Batch of a device-resident uint8 dataset: gather rows ``idx`` of src (N, C, H, W), optional
// per-image (dy, dx, flip) augmentation ``aug`` (B, 3) int32 with zero padding ``pad``, then
// ToTensor + Normalize -> fp32 (B, C, H, W).
at::Tensor augment_u8(const at::Tensor& src, const at::Tensor& idx, const c10::optional<at::Tensor>& aug, int64_t pad,
                      const at::Tensor& mean, const at::Tensor& inv_std) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kByte && src.dim() == 4 && src.is_contiguous(),
              "src must be a contiguous uint8 (N, C, H, W) GPU tensor");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kLong && idx.dim() == 1 && idx.is_contiguous(),
              "idx must be a contiguous int64 GPU vector");
  const int64_t B = idx.size(0), C = src.size(1), H = src.size(2), W = src.size(3);
  const int* ap = nullptr;
  if (present(aug)) {
    TORCH_CHECK(aug->is_cuda() && aug->scalar_type() == at::kInt && aug->is_contiguous() && aug->numel() == 3 * B,
                "aug must be a contiguous int32 (B, 3) GPU tensor");
    ap = aug->data_ptr<int>();
  }
  need(mean, "mean");
  need(inv_std, "inv_std");
  TORCH_CHECK(mean.numel() == C && inv_std.numel() == C && mean.is_contiguous() && inv_std.is_contiguous(),
              "mean / inv_std must have C elements");
  TORCH_CHECK(pad >= 0, "pad must be >= 0");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
  TORCH_CHECK(idx.device() == src.device() && mean.device() == src.device() && inv_std.device() == src.device() &&
                  (!ap || aug->device() == src.device()), "augment_u8 operands must share a device");
  auto out = at::empty({B, C, H, W}, src.options().dtype(at::kFloat));
  if (out.numel() == 0) return out;
  TP_CHECK_HIP(tp_augment_u8(src.data_ptr<uint8_t>(), idx.data_ptr<int64_t>(), ap, (int)B, (int)C, (int)H, (int)W,
                             (int)pad, mean.data_ptr<float>(), inv_std.data_ptr<float>(), out.data_ptr<float>(),
                             cur_stream()));
  return out;
}

// Inverted dropout with a counter-based Philox mask (forward and, with the same seed, backward).
at::Tensor dropout(const at::Tensor& x_, int64_t seed, double p) {
  need(x_, "x");
  auto x = x_.contiguous();
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1)");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  // the kernel loads float4: a contiguous view into the middle of a storage (x[1:] of an odd-width
  // matrix) is copied to storage of its own; the mask depends on the element index only
  if (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0) x = x.clone(at::MemoryFormat::Contiguous);
  auto y = at::empty(x.sizes(), x.options());
  if (x.numel() == 0) return y;
  TP_CHECK_HIP(tp_dropout(x.data_ptr<float>(), y.data_ptr<float>(), x.numel(), (unsigned long long)seed, p,
                          cur_stream()));
  return y;
}

// Training max-pool on NHWC (B, H, W, C), C % 4 == 0: (y, window-local argmax bytes); the
// backward gathers (deterministic). avgpool_bwd: global average pool gradient (B, C) -> (B, H, W, C).
std::tuple<at::Tensor, at::Tensor> maxpool_train_fwd(const at::Tensor& x, int64_t k, int64_t s, int64_t pad) {
  need(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && x.size(3) % 4 == 0, "x must be contiguous NHWC with C % 4 == 0");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int64_t Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  TORCH_CHECK(k >= 1 && k * k <= 255 && s >= 1 && pad >= 0 && 2 * pad <= k && Ho > 0 && Wo > 0, "bad pool geometry");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({B, Ho, Wo, C}, x.options());
  auto am = at::empty({B, Ho, Wo, C}, x.options().dtype(at::kByte));
  TP_CHECK_HIP(tp_maxpool_fwd_arg(x.data_ptr<float>(), y.data_ptr<float>(), am.data_ptr<uint8_t>(), (int)B, (int)H,
                                  (int)W, (int)C, (int)k, (int)s, (int)pad, cur_stream()));
  return {y, am};
}

at::Tensor maxpool_train_bwd(const at::Tensor& g_, const at::Tensor& am, int64_t H, int64_t W, int64_t k, int64_t s,
                             int64_t pad) {
  need(g_, "g");
  auto g = g_.contiguous();
  TORCH_CHECK(g.dim() == 4, "g must be (B, Ho, Wo, C)");
  const uint8_t* amp = argmax_ptr(am, "am", g);  // the forward's window-local argmax
  const int64_t B = g.size(0), C = g.size(3);
  TORCH_CHECK(g.size(1) == (H + 2 * pad - k) / s + 1 && g.size(2) == (W + 2 * pad - k) / s + 1, "g shape mismatch");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  auto dx = at::empty({B, H, W, C}, g.options());
  TP_CHECK_HIP(tp_maxpool_bwd(g.data_ptr<float>(), amp, dx.data_ptr<float>(), (int)B, (int)H, (int)W, (int)C, (int)k,
                              (int)s, (int)pad, cur_stream()));
  return dx;
}

// Depthwise convolution (depth multiplier 1) on NHWC: x (B, H, W, C), w the (C, 1, k, k) parameter
// read in place, k in {3, 5}, stride in {1, 2}, zero padding 0..k-1, any C. The activations may carry
// more channels than the parameter (a pruned width at the kernels' granule): Cp = x.size(3) >
// Cw = w.size(0) needs Cp % 4 == 0; the outputs' channels past Cw are exact zeros.
void check_dw_geometry(int64_t H, int64_t W, int64_t k, int64_t s, int64_t pad) {
  TORCH_CHECK((k == 3 || k == 5) && (s == 1 || s == 2) && pad >= 0 && pad <= k - 1 && H + 2 * pad >= k &&
                  W + 2 * pad >= k, "bad depthwise conv geometry: k ", k, " stride ", s, " pad ", pad, " on ", H, "x", W);
}

void check_dw_weight(const at::Tensor& w, int64_t C, const at::Tensor& like) {
  need(w, "w");
  TORCH_CHECK(w.dim() == 4 && w.size(0) >= 1 && w.size(0) <= C && w.size(1) == 1 && w.size(2) == w.size(3) &&
                  w.is_contiguous() && w.device() == like.device(),
              "w must be a contiguous (Cw, 1, k, k) depthwise weight with Cw <= the activation's channels");
  TORCH_CHECK(w.size(0) == C || C % 4 == 0, "a carried width (more channels than the weight) must be a multiple of 4");
}

at::Tensor dwconv_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, int64_t s,
                      int64_t pad) {
  need(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && x.numel() > 0, "x must be a non-empty contiguous NHWC tensor");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  check_dw_weight(w, C, x);
  const int64_t k = w.size(2);
  check_dw_geometry(H, W, k, s, pad);
  TORCH_CHECK(x.numel() < (int64_t(1) << 29), "x exceeds the kernels' 2 GiB operand range");
  const float* bp = nullptr;
  if (present(bias)) {
    need(*bias, "bias", kAnyLayout, &x);
    TORCH_CHECK(bias->dim() == 1 && bias->size(0) == w.size(0) && bias->is_contiguous(),
                "bias must be a contiguous (Cw,) tensor");
    bp = bias->data_ptr<float>();
  }
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({B, (H + 2 * pad - k) / s + 1, (W + 2 * pad - k) / s + 1, C}, x.options());
  TP_CHECK_HIP(tp_dwconv_fwd(x.data_ptr<float>(), w.data_ptr<float>(), bp, y.data_ptr<float>(), (int)B, (int)H,
                             (int)W, (int)C, (int)w.size(0), (int)k, (int)s, (int)pad, cur_stream()));
  return y;
}

at::Tensor dwconv_dgrad(const at::Tensor& g_, const at::Tensor& w, int64_t H, int64_t W, int64_t s, int64_t pad) {
  need(g_, "g");
  auto g = g_.contiguous();
  TORCH_CHECK(g.dim() == 4 && g.numel() > 0 && H > 0 && W > 0, "g must be a non-empty (B, Ho, Wo, C) tensor");
  const int64_t B = g.size(0), C = g.size(3);
  check_dw_weight(w, C, g);
  const int64_t k = w.size(2);
  check_dw_geometry(H, W, k, s, pad);
  TORCH_CHECK(g.size(1) == (H + 2 * pad - k) / s + 1 && g.size(2) == (W + 2 * pad - k) / s + 1, "g shape mismatch");
  TORCH_CHECK(H < (int64_t(1) << 29) && W < (int64_t(1) << 29) && B * H * W * C < (int64_t(1) << 29),
              "dx exceeds the kernels' 2 GiB operand range");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  auto dx = at::empty({B, H, W, C}, g.options());
  TP_CHECK_HIP(tp_dwconv_dgrad(g.data_ptr<float>(), w.data_ptr<float>(), dx.data_ptr<float>(), (int)B, (int)H,
                               (int)W, (int)C, (int)w.size(0), (int)k, (int)s, (int)pad, cur_stream()));
  return dx;
}

// dW is written into ``dw`` with that tensor's own strides (the parameter's: DDP bucket views);
// returns the bias gradient when asked for. dw's channel count Cw may be smaller than g / x's (a
// carried width, a multiple of 4 then): the gradients cover the Cw channels of the parameter.
c10::optional<at::Tensor> dwconv_wgrad(const at::Tensor& g_, const at::Tensor& x, int64_t k, int64_t s, int64_t pad,
                                       at::Tensor& dw, bool want_bias) {
  need(g_, "g");
  need(x, "x");
  need(dw, "dw");
  auto g = g_.contiguous();
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && g.dim() == 4 && g.numel() > 0 && x.device() == g.device(),
              "g / x must be non-empty contiguous NHWC tensors on one device");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  check_dw_geometry(H, W, k, s, pad);
  const int64_t Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  TORCH_CHECK(g.size(0) == B && g.size(1) == Ho && g.size(2) == Wo && g.size(3) == C, "g shape mismatch");
  TORCH_CHECK(dw.dim() == 4 && dw.size(0) >= 1 && dw.size(0) <= C && dw.size(1) == 1 && dw.size(2) == k &&
                  dw.size(3) == k && dw.device() == g.device() && dw.stride(0) > 0 && dw.stride(2) > 0 &&
                  dw.stride(3) > 0,
              "dw must be a (Cw, 1, k, k) tensor with positive strides, Cw <= the activations' channels");
  const int64_t Cw = dw.size(0);
  TORCH_CHECK(Cw == C || C % 4 == 0, "a carried width (more channels than dw) must be a multiple of 4");
  TORCH_CHECK(x.numel() < (int64_t(1) << 29) && g.numel() < (int64_t(1) << 29),
              "g / x exceed the kernels' 2 GiB operand range");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  const int chunks = tp_dwconv_wgrad_chunks((int)(B * Ho * Wo), (int)C);
  auto ws = at::empty({(int64_t)chunks * (k * k + 1) * C}, g.options().dtype(at::kDouble));
  c10::optional<at::Tensor> db;
  if (want_bias) db = at::empty({Cw}, g.options());
  TP_CHECK_HIP(tp_dwconv_wgrad(g.data_ptr<float>(), x.data_ptr<float>(), dw.data_ptr<float>(),
                               want_bias ? db->data_ptr<float>() : nullptr, ws.data_ptr<double>(), chunks, (int)B,
                               (int)H, (int)W, (int)C, (int)Cw, (int)k, (int)s, (int)pad, dw.stride(0),
                               dw.stride(2), dw.stride(3), cur_stream()));
  return db;
}

void check_dwa_params(const at::Tensor& w, const at::Tensor& scale, const at::Tensor* shift, int64_t C,
                      const at::Tensor& like) {
  need(w, "w");
  need(scale, "scale");
  TORCH_CHECK(C % 4 == 0, "dwconv_act needs a channel count that is a multiple of 4 (pad the channels), got ", C);
  TORCH_CHECK(w.dim() == 4 && w.size(0) == C && w.size(1) == 1 && w.size(2) == w.size(3) && w.is_contiguous() &&
                  w.device() == like.device(), "w must be a contiguous (C, 1, k, k) depthwise weight");
  TORCH_CHECK(scale.dim() == 1 && scale.size(0) == C && scale.is_contiguous() && scale.device() == like.device(),
              "scale must be a contiguous (C,) tensor");
  if (shift != nullptr) {
    need(*shift, "shift");
    TORCH_CHECK(shift->dim() == 1 && shift->size(0) == C && shift->is_contiguous() && shift->device() == like.device(),
                "shift must be a contiguous (C,) tensor");
  }
}

void check_dwa_acts(int64_t in_act, int64_t out_act) {
  TORCH_CHECK(in_act >= 0 && in_act <= 2 && out_act >= 0 && out_act <= 2,
              "activation codes are 0 (none), 1 (ReLU), 2 (ReLU6), got ", in_act, " / ", out_act);
}

// y = out_act(scale * dwconv(in_act(x)) + shift) on NHWC tensors; apoz (B, C) += count(y > 0)
at::Tensor dwconv_act_fwd(const at::Tensor& x, const at::Tensor& w, const at::Tensor& scale, const at::Tensor& shift,
                          int64_t s, int64_t pad, int64_t in_act, int64_t out_act,
                          const c10::optional<at::Tensor>& apoz) {
  need(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && x.numel() > 0, "x must be a non-empty contiguous NHWC tensor");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  check_dwa_params(w, scale, &shift, C, x);
  check_dwa_acts(in_act, out_act);
  const int64_t k = w.size(2);
  check_dw_geometry(H, W, k, s, pad);
  TORCH_CHECK(x.numel() < (int64_t(1) << 29), "x exceeds the kernels' 2 GiB operand range");
  float* ap = nullptr;
  if (present(apoz)) {  // (stricter than count_ptr: the (B, C) shape itself)
    need(*apoz, "apoz", 2, &x);
    TORCH_CHECK(apoz->size(0) == B && apoz->size(1) == C, "apoz must be a contiguous (B, C) tensor");
    ap = apoz->data_ptr<float>();
  }
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({B, (H + 2 * pad - k) / s + 1, (W + 2 * pad - k) / s + 1, C}, x.options());
  TP_CHECK_HIP(tp_dwconv_act_fwd(x.data_ptr<float>(), w.data_ptr<float>(), scale.data_ptr<float>(),
                                 shift.data_ptr<float>(), y.data_ptr<float>(), ap, (int)B, (int)H, (int)W, (int)C,
                                 (int)k, (int)s, (int)pad, (int)in_act, (int)out_act, cur_stream()));
  return y;
}

int64_t dwconv_act_tay_slots(int64_t H, int64_t W, int64_t C) {
  TORCH_CHECK(H > 0 && W > 0 && C > 0 && H < (int64_t(1) << 29) && W < (int64_t(1) << 29) && C < (int64_t(1) << 29),
              "bad shape");
  return tp_dwconv_act_tay_slots((int)H, (int)W, (int)C);
}

// dz = mask_in(z) * dA, dA = dwconv^T(mask_out(y) * g * scale); tay: zeroed (R, B, C) slab of the
// partial sums of -(dA * in_act(z)) (tay_mode 0) or |dA| (1), R = dwconv_act_tay_slots(H, W, C)
at::Tensor dwconv_act_dgrad(const at::Tensor& g, const at::Tensor& y, const at::Tensor& w, const at::Tensor& scale,
                            const at::Tensor& z, int64_t H, int64_t W, int64_t s, int64_t pad, int64_t in_act,
                            int64_t out_act, const c10::optional<at::Tensor>& tay, int64_t tay_mode) {
  need(g, "g");
  need(y, "y");
  need(z, "z");
  TORCH_CHECK(z.dim() == 4 && z.is_contiguous() && z.numel() > 0 && z.size(1) == H && z.size(2) == W,
              "z must be a non-empty contiguous (B, H, W, C) tensor");
  const int64_t B = z.size(0), C = z.size(3);
  check_dwa_params(w, scale, nullptr, C, z);
  check_dwa_acts(in_act, out_act);
  const int64_t k = w.size(2);
  check_dw_geometry(H, W, k, s, pad);
  const int64_t Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  TORCH_CHECK(g.dim() == 4 && g.is_contiguous() && g.size(0) == B && g.size(1) == Ho && g.size(2) == Wo &&
                  g.size(3) == C && g.device() == z.device(), "g must be a contiguous (B, Ho, Wo, C) tensor");
  TORCH_CHECK(y.sizes() == g.sizes() && y.is_contiguous() && y.device() == z.device(), "y must match g");
  TORCH_CHECK(z.numel() < (int64_t(1) << 29), "z exceeds the kernels' 2 GiB operand range");
  float* tp = nullptr;
  int R = 0;
  if (present(tay)) {
    need(*tay, "tay");
    TORCH_CHECK(tay_mode == 0 || tay_mode == 1, "tay_mode is 0 (Taylor) or 1 (Sensitivity)");
    R = tp_dwconv_act_tay_slots((int)H, (int)W, (int)C);
    TORCH_CHECK(tay->dim() == 3 && tay->size(0) == R && tay->size(1) == B && tay->size(2) == C &&
                    tay->is_contiguous() && tay->device() == z.device(),
                "tay must be a contiguous (dwconv_act_tay_slots(H, W, C), B, C) slab");
    TORCH_CHECK(tay->numel() < (int64_t(1) << 29), "tay exceeds the kernels' 2 GiB operand range");
    tp = tay->data_ptr<float>();
  }
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(z.device());
  auto dz = at::empty_like(z);
  TP_CHECK_HIP(tp_dwconv_act_dgrad(g.data_ptr<float>(), y.data_ptr<float>(), w.data_ptr<float>(),
                                   scale.data_ptr<float>(), z.data_ptr<float>(), dz.data_ptr<float>(), tp, R,
                                   (int)tay_mode, (int)B, (int)H, (int)W, (int)C, (int)k, (int)s, (int)pad,
                                   (int)in_act, (int)out_act, cur_stream()));
  return dz;
}

void check_dwhs_acts(int64_t in_act, int64_t out_act) {
  TORCH_CHECK(in_act >= 0 && in_act <= 3 && out_act >= 0 && out_act <= 3,
              "activation codes are 0 (none), 1 (ReLU), 2 (ReLU6), 3 (Hardswish), got ", in_act, " / ", out_act);
}

// dwconv_act_fwd with activation code 3 (Hardswish) on either side; pre (the shape of y) receives the
// output's pre-activation, the y operand of dwconv_hs_dgrad when out_act == 3
at::Tensor dwconv_hs_fwd(const at::Tensor& x, const at::Tensor& w, const at::Tensor& scale, const at::Tensor& shift,
                         int64_t s, int64_t pad, int64_t in_act, int64_t out_act,
                         const c10::optional<at::Tensor>& apoz, const c10::optional<at::Tensor>& pre) {
  need(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && x.numel() > 0, "x must be a non-empty contiguous NHWC tensor");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  check_dwa_params(w, scale, &shift, C, x);
  check_dwhs_acts(in_act, out_act);
  const int64_t k = w.size(2);
  check_dw_geometry(H, W, k, s, pad);
  TORCH_CHECK(x.numel() < (int64_t(1) << 29), "x exceeds the kernels' 2 GiB operand range");
  const int64_t Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  float *ap = nullptr, *pp = nullptr;
  if (present(apoz)) {
    need(*apoz, "apoz", 2, &x);
    TORCH_CHECK(apoz->size(0) == B && apoz->size(1) == C, "apoz must be a contiguous (B, C) tensor");
    ap = apoz->data_ptr<float>();
  }
  if (present(pre)) {
    need(*pre, "pre", 4, &x);
    TORCH_CHECK(pre->size(0) == B && pre->size(1) == Ho && pre->size(2) == Wo && pre->size(3) == C,
                "pre must be a contiguous (B, Ho, Wo, C) tensor");
    pp = pre->data_ptr<float>();
  }
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({B, Ho, Wo, C}, x.options());
  TP_CHECK_HIP(tp_dwconv_hs_fwd(x.data_ptr<float>(), w.data_ptr<float>(), scale.data_ptr<float>(),
                                shift.data_ptr<float>(), y.data_ptr<float>(), ap, pp, (int)B, (int)H, (int)W, (int)C,
                                (int)k, (int)s, (int)pad, (int)in_act, (int)out_act, cur_stream()));
  return y;
}

int64_t dwconv_hs_tay_slots(int64_t H, int64_t W, int64_t C) {
  TORCH_CHECK(H > 0 && W > 0 && C > 0 && H < (int64_t(1) << 29) && W < (int64_t(1) << 29) && C < (int64_t(1) << 29),
              "bad shape");
  return tp_dwconv_hs_tay_slots((int)H, (int)W, (int)C);
}

// dz = d_in(z) * dA, dA = dwconv^T(g * scale * d_out(y)): y is the stored output for out_act 1 / 2 and
// the stored pre-activation for out_act 3; tay as dwconv_act_dgrad
at::Tensor dwconv_hs_dgrad(const at::Tensor& g, const at::Tensor& y, const at::Tensor& w, const at::Tensor& scale,
                           const at::Tensor& z, int64_t H, int64_t W, int64_t s, int64_t pad, int64_t in_act,
                           int64_t out_act, const c10::optional<at::Tensor>& tay, int64_t tay_mode) {
  need(g, "g");
  need(y, "y");
  need(z, "z");
  TORCH_CHECK(z.dim() == 4 && z.is_contiguous() && z.numel() > 0 && z.size(1) == H && z.size(2) == W,
              "z must be a non-empty contiguous (B, H, W, C) tensor");
  const int64_t B = z.size(0), C = z.size(3);
  check_dwa_params(w, scale, nullptr, C, z);
  check_dwhs_acts(in_act, out_act);
  const int64_t k = w.size(2);
  check_dw_geometry(H, W, k, s, pad);
  const int64_t Ho = (H + 2 * pad - k) / s + 1, Wo = (W + 2 * pad - k) / s + 1;
  TORCH_CHECK(g.dim() == 4 && g.is_contiguous() && g.size(0) == B && g.size(1) == Ho && g.size(2) == Wo &&
                  g.size(3) == C && g.device() == z.device(), "g must be a contiguous (B, Ho, Wo, C) tensor");
  TORCH_CHECK(y.sizes() == g.sizes() && y.is_contiguous() && y.device() == z.device(), "y must match g");
  TORCH_CHECK(z.numel() < (int64_t(1) << 29), "z exceeds the kernels' 2 GiB operand range");
  float* tp = nullptr;
  int R = 0;
  if (present(tay)) {
    need(*tay, "tay");
    TORCH_CHECK(tay_mode == 0 || tay_mode == 1, "tay_mode is 0 (Taylor) or 1 (Sensitivity)");
    R = tp_dwconv_hs_tay_slots((int)H, (int)W, (int)C);
    TORCH_CHECK(tay->dim() == 3 && tay->size(0) == R && tay->size(1) == B && tay->size(2) == C &&
                    tay->is_contiguous() && tay->device() == z.device(),
                "tay must be a contiguous (dwconv_hs_tay_slots(H, W, C), B, C) slab");
    TORCH_CHECK(tay->numel() < (int64_t(1) << 29), "tay exceeds the kernels' 2 GiB operand range");
    tp = tay->data_ptr<float>();
  }
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(z.device());
  auto dz = at::empty_like(z);
  TP_CHECK_HIP(tp_dwconv_hs_dgrad(g.data_ptr<float>(), y.data_ptr<float>(), w.data_ptr<float>(),
                                  scale.data_ptr<float>(), z.data_ptr<float>(), dz.data_ptr<float>(), tp, R,
                                  (int)tay_mode, (int)B, (int)H, (int)W, (int)C, (int)k, (int)s, (int)pad,
                                  (int)in_act, (int)out_act, cur_stream()));
  return dz;
}

at::Tensor avgpool_bwd(const at::Tensor& g_, int64_t H, int64_t W) {
  need(g_, "g");
  auto g = g_.contiguous();
  TORCH_CHECK(g.dim() == 2 && g.size(1) % 4 == 0 && H > 0 && W > 0, "g must be (B, C) with C % 4 == 0");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  auto dx = at::empty({g.size(0), H, W, g.size(1)}, g.options());
  TP_CHECK_HIP(tp_avgpool_bwd(g.data_ptr<float>(), dx.data_ptr<float>(), (int)g.size(0), (int)(H * W),
                              (int)g.size(1), cur_stream()));
  return dx;
}

// ---- squeeze-and-excitation gates (squeeze_excite.hip): x / g (B, H, W, C) NHWC, rows (B, C) / (B, Cs)
void check_se_act(const at::Tensor& x, const char* name) {
  need(x, name);
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && x.numel() > 0, name, " must be a non-empty contiguous NHWC tensor");
  TORCH_CHECK(x.numel() < (int64_t(1) << 29), name, " exceeds the kernels' 2 GiB operand range");
  TORCH_CHECK(x.size(0) <= 65535, name, ": more than 65535 images per call");
}

void check_se_rows(const at::Tensor& t, int64_t B, int64_t n, const at::Tensor& like, const char* name) {
  need(t, name);
  TORCH_CHECK(t.dim() == 2 && t.size(0) == B && t.size(1) == n && t.is_contiguous() && t.device() == like.device(),
              name, " must be a contiguous (", B, ", ", n, ") tensor on the same device");
}

// fc weights in the parameter's layout: (out, in) or (out, in, 1, 1), contiguous
void check_se_weight(const at::Tensor& w, int64_t n_out, int64_t n_in, const at::Tensor& like, const char* name) {
  need(w, name);
  TORCH_CHECK((w.dim() == 2 || (w.dim() == 4 && w.size(2) == 1 && w.size(3) == 1)) && w.size(0) == n_out &&
                  w.size(1) == n_in && w.is_contiguous() && w.device() == like.device(),
              name, " must be a contiguous (", n_out, ", ", n_in, "[, 1, 1]) weight on the same device");
}

const float* se_bias(const c10::optional<at::Tensor>& b, int64_t n, const at::Tensor& like, const char* name) {
  if (!present(b)) return nullptr;
  need(*b, name);
  TORCH_CHECK(b->dim() == 1 && b->size(0) == n && b->is_contiguous() && b->device() == like.device(), name,
              " must be a contiguous (", n, ",) tensor on the same device");
  return b->data_ptr<float>();
}

void check_se_widths(int64_t C, int64_t Cs) {
  TORCH_CHECK(C >= 1 && Cs >= 1 && C + Cs <= 12288, "gate widths out of the kernels' range (C + Cs <= 12288), got ", C,
              " and ", Cs);
}

// (B, C) = scale * sum over the pixels of a (* x when given)
at::Tensor se_reduce(const at::Tensor& a, const at::Tensor* x) {
  const int64_t B = a.size(0), HW = a.size(1) * a.size(2), C = a.size(3);
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  auto out = at::empty({B, C}, a.options());
  const int splits = tp_se_splits((int)B, (int)HW, (int)C);
  at::Tensor ws;
  if (splits > 1) ws = at::empty({(int64_t)splits * B * C}, a.options());
  float* wp = splits > 1 ? ws.data_ptr<float>() : nullptr;
  if (x != nullptr)
    TP_CHECK_HIP(tp_se_bwd_reduce(a.data_ptr<float>(), x->data_ptr<float>(), out.data_ptr<float>(), wp, splits, (int)B,
                                  (int)HW, (int)C, cur_stream()));
  else
    TP_CHECK_HIP(tp_se_pool(a.data_ptr<float>(), out.data_ptr<float>(), wp, splits, (int)B, (int)HW, (int)C,
                            cur_stream()));
  return out;
}

at::Tensor se_pool(const at::Tensor& x) {
  check_se_act(x, "x");
  return se_reduce(x, nullptr);
}

at::Tensor se_bwd_reduce(const at::Tensor& g, const at::Tensor& x) {
  check_se_act(g, "g");
  check_se_act(x, "x");
  TORCH_CHECK(g.sizes() == x.sizes() && g.device() == x.device(), "g / x shape or device mismatch");
  return se_reduce(g, &x);
}

std::tuple<at::Tensor, at::Tensor> se_gate_fwd(const at::Tensor& p, const at::Tensor& w1,
                                               const c10::optional<at::Tensor>& b1, const at::Tensor& w2,
                                               const c10::optional<at::Tensor>& b2, int64_t gate) {
  need(p, "p");
  TORCH_CHECK(p.dim() == 2 && p.is_contiguous() && p.numel() > 0, "p must be a non-empty contiguous (B, C) tensor");
  TORCH_CHECK(gate == 0 || gate == 1, "gate must be 0 (Hardsigmoid) or 1 (Sigmoid)");
  const int64_t B = p.size(0), C = p.size(1);
  TORCH_CHECK(w1.dim() >= 2, "w1 must be a (Cs, C[, 1, 1]) weight");
  const int64_t Cs = w1.size(0);
  check_se_widths(C, Cs);
  check_se_weight(w1, Cs, C, p, "w1");
  check_se_weight(w2, C, Cs, p, "w2");
  const float* b1p = se_bias(b1, Cs, p, "b1");
  const float* b2p = se_bias(b2, C, p, "b2");
  TORCH_CHECK(B * std::max(C, Cs) < (int64_t(1) << 24), "too many rows");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  auto h = at::empty({B, Cs}, p.options());
  auto s = at::empty({B, C}, p.options());
  TP_CHECK_HIP(tp_se_gate_fwd(p.data_ptr<float>(), w1.data_ptr<float>(), b1p, w2.data_ptr<float>(), b2p,
                              h.data_ptr<float>(), s.data_ptr<float>(), (int)B, (int)C, (int)Cs, (int)gate,
                              cur_stream()));
  return {h, s};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> se_gate_bwd(const at::Tensor& ds, const at::Tensor& s,
                                                           const at::Tensor& h, const at::Tensor& w1,
                                                           const at::Tensor& w2, int64_t gate) {
  need(ds, "ds");
  TORCH_CHECK(ds.dim() == 2 && ds.is_contiguous() && ds.numel() > 0, "ds must be a non-empty contiguous (B, C) tensor");
  TORCH_CHECK(gate == 0 || gate == 1, "gate must be 0 (Hardsigmoid) or 1 (Sigmoid)");
  TORCH_CHECK(h.dim() == 2, "h must be (B, Cs)");
  const int64_t B = ds.size(0), C = ds.size(1), Cs = h.size(1);
  check_se_widths(C, Cs);
  check_se_rows(s, B, C, ds, "s");
  check_se_rows(h, B, Cs, ds, "h");
  check_se_weight(w1, Cs, C, ds, "w1");
  check_se_weight(w2, C, Cs, ds, "w2");
  TORCH_CHECK(B * std::max(C, Cs) < (int64_t(1) << 24), "too many rows");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ds.device());
  auto dz2 = at::empty({B, C}, ds.options());
  auto dz1 = at::empty({B, Cs}, ds.options());
  auto dp = at::empty({B, C}, ds.options());
  TP_CHECK_HIP(tp_se_gate_bwd(ds.data_ptr<float>(), s.data_ptr<float>(), h.data_ptr<float>(), w1.data_ptr<float>(),
                              w2.data_ptr<float>(), dz2.data_ptr<float>(), dz1.data_ptr<float>(), dp.data_ptr<float>(),
                              (int)B, (int)C, (int)Cs, (int)gate, cur_stream()));
  return {dz2, dz1, dp};
}

at::Tensor se_scale(const at::Tensor& x, const at::Tensor& s) {
  check_se_act(x, "x");
  const int64_t B = x.size(0), C = x.size(3);
  check_se_rows(s, B, C, x, "s");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto out = at::empty_like(x);
  TP_CHECK_HIP(tp_se_scale(x.data_ptr<float>(), s.data_ptr<float>(), out.data_ptr<float>(), (int)B,
                           (int)(x.size(1) * x.size(2)), (int)C, cur_stream()));
  return out;
}

at::Tensor se_bwd_dx(const at::Tensor& g, const at::Tensor& s, const at::Tensor& dp) {
  check_se_act(g, "g");
  const int64_t B = g.size(0), C = g.size(3);
  check_se_rows(s, B, C, g, "s");
  check_se_rows(dp, B, C, g, "dp");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  auto dx = at::empty_like(g);
  TP_CHECK_HIP(tp_se_bwd_dx(g.data_ptr<float>(), s.data_ptr<float>(), dp.data_ptr<float>(), dx.data_ptr<float>(),
                            (int)B, (int)(g.size(1) * g.size(2)), (int)C, cur_stream()));
  return dx;
}

// dW[r, k] = sum_b a[b, r] * m[b, k] written into ``dw`` ((R, K) or (R, K, 1, 1)) with that tensor's own
// strides (the parameter's: DDP bucket views); returns db[r] = sum_b a[b, r] when asked for
c10::optional<at::Tensor> se_wgrad(const at::Tensor& a, const at::Tensor& m, at::Tensor& dw, bool want_bias) {
  need(a, "a");
  need(dw, "dw");
  TORCH_CHECK(a.dim() == 2 && a.is_contiguous() && a.numel() > 0 && m.dim() == 2, "a / m must be (B, R) / (B, K) rows");
  const int64_t B = a.size(0), R = a.size(1), K = m.size(1);
  check_se_rows(m, B, K, a, "m");
  TORCH_CHECK((dw.dim() == 2 || (dw.dim() == 4 && dw.size(2) == 1 && dw.size(3) == 1)) && dw.size(0) == R &&
                  dw.size(1) == K && dw.device() == a.device() && dw.stride(0) > 0 && dw.stride(1) > 0,
              "dw must be a (R, K[, 1, 1]) tensor with positive strides on the same device");
  TORCH_CHECK(R * K < (int64_t(1) << 29) && B * std::max(R, K) < (int64_t(1) << 29), "operands exceed the 2 GiB range");
  at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  c10::optional<at::Tensor> db;
  if (want_bias) db = at::empty({R}, a.options());
  TP_CHECK_HIP(tp_se_wgrad(a.data_ptr<float>(), m.data_ptr<float>(), dw.data_ptr<float>(),
                           want_bias ? db->data_ptr<float>() : nullptr, (int)B, (int)R, (int)K, dw.stride(0),
                           dw.stride(1), cur_stream()));
  return db;
}

}  // namespace

TORCH_LIBRARY(tpamd, m) {
  m.def("se_pool(Tensor x) -> Tensor");
  m.def("se_gate_fwd(Tensor p, Tensor w1, Tensor? b1, Tensor w2, Tensor? b2, int gate) -> (Tensor, Tensor)");
  m.def("se_scale(Tensor x, Tensor s) -> Tensor");
  m.def("se_bwd_reduce(Tensor g, Tensor x) -> Tensor");
  m.def("se_gate_bwd(Tensor ds, Tensor s, Tensor h, Tensor w1, Tensor w2, int gate) -> (Tensor, Tensor, Tensor)");
  m.def("se_bwd_dx(Tensor g, Tensor s, Tensor dp) -> Tensor");
  m.def("se_wgrad(Tensor a, Tensor m, Tensor(a!) dw, bool want_bias) -> Tensor?");
  m.def("channel_reduce(Tensor? act, Tensor? grad, int mode) -> Tensor");
  m.def("column_accumulate(Tensor v, Tensor(a!) acc_sum, Tensor(b!)? acc_sq) -> ()");
  m.def("channel_fill_(Tensor(a!) x, Tensor idx, float value) -> ()");
  m.def("score_fold_(Tensor(a!)[] T, Tensor(b!)[] acc, bool take_abs, int after) -> ()");
  m.def("nan_channels(Tensor x) -> Tensor");
  m.def("gather_multi(Tensor[] srcs, int[] axes, Tensor keep) -> Tensor[]");
  m.def("prefix_mask(Tensor z, Tensor rank, int p0, int K) -> Tensor");
  m.def("prefix_project(Tensor base, Tensor a, Tensor fill, Tensor wt, Tensor perm, int p0, int cnt) -> Tensor");
  m.def("shapley_scatter(Tensor L, Tensor perm, Tensor(a!) sv, int row0, int k0, float scale) -> ()");
  m.def("shapley_column(Tensor L, Tensor perm, Tensor(a!) sv_col, int k0, float scale) -> ()");
  m.def("cross_entropy(Tensor logits, Tensor target, float gscale, bool want_grad) -> (Tensor, Tensor)");
  m.def("augment_u8(Tensor src, Tensor idx, Tensor? aug, int pad, Tensor mean, Tensor inv_std) -> Tensor");
  m.def("dropout(Tensor x, int seed, float p) -> Tensor");
  m.def("maxpool_train_fwd(Tensor x, int k, int s, int pad) -> (Tensor, Tensor)");
  m.def("maxpool_train_bwd(Tensor g, Tensor am, int H, int W, int k, int s, int pad) -> Tensor");
  m.def("avgpool_bwd(Tensor g, int H, int W) -> Tensor");
  m.def("dwconv_fwd(Tensor x, Tensor w, Tensor? bias, int stride, int pad) -> Tensor");
  m.def("dwconv_dgrad(Tensor g, Tensor w, int H, int W, int stride, int pad) -> Tensor");
  m.def("dwconv_wgrad(Tensor g, Tensor x, int k, int stride, int pad, Tensor(a!) dw, bool want_bias) -> Tensor?");
  m.def("dwconv_act_fwd(Tensor x, Tensor w, Tensor scale, Tensor shift, int stride, int pad, int in_act, int out_act, "
        "Tensor(a!)? apoz=None) -> Tensor");
  m.def("dwconv_act_dgrad(Tensor g, Tensor y, Tensor w, Tensor scale, Tensor z, int H, int W, int stride, int pad, "
        "int in_act, int out_act, Tensor(a!)? tay=None, int tay_mode=0) -> Tensor");
  m.def("dwconv_act_tay_slots(int H, int W, int C) -> int", &dwconv_act_tay_slots);
  m.def("dwconv_hs_fwd(Tensor x, Tensor w, Tensor scale, Tensor shift, int stride, int pad, int in_act, int out_act, "
        "Tensor(a!)? apoz=None, Tensor(b!)? pre=None) -> Tensor");
  m.def("dwconv_hs_dgrad(Tensor g, Tensor y, Tensor w, Tensor scale, Tensor z, int H, int W, int stride, int pad, "
        "int in_act, int out_act, Tensor(a!)? tay=None, int tay_mode=0) -> Tensor");
  m.def("dwconv_hs_tay_slots(int H, int W, int C) -> int", &dwconv_hs_tay_slots);
  register_engine_ops_def(m);
}

TORCH_LIBRARY_IMPL(tpamd, CUDA, m) {
  m.impl("channel_reduce", &channel_reduce);
  m.impl("column_accumulate", &column_accumulate);
  m.impl("channel_fill_", &channel_fill_);
  m.impl("score_fold_", &score_fold_);
  m.impl("nan_channels", &nan_channels);
  m.impl("gather_multi", &gather_multi);
  m.impl("prefix_mask", &prefix_mask);
  m.impl("prefix_project", &prefix_project);
  m.impl("shapley_scatter", &shapley_scatter);
  m.impl("shapley_column", &shapley_column);
  m.impl("cross_entropy", &cross_entropy);
  m.impl("augment_u8", &augment_u8);
  m.impl("dropout", &dropout);
  m.impl("maxpool_train_fwd", &maxpool_train_fwd);
  m.impl("maxpool_train_bwd", &maxpool_train_bwd);
  m.impl("avgpool_bwd", &avgpool_bwd);
  m.impl("dwconv_fwd", &dwconv_fwd);
  m.impl("dwconv_dgrad", &dwconv_dgrad);
  m.impl("dwconv_wgrad", &dwconv_wgrad);
  m.impl("dwconv_act_fwd", &dwconv_act_fwd);
  m.impl("dwconv_act_dgrad", &dwconv_act_dgrad);
  m.impl("dwconv_hs_fwd", &dwconv_hs_fwd);
  m.impl("dwconv_hs_dgrad", &dwconv_hs_dgrad);
  m.impl("se_pool", &se_pool);
  m.impl("se_gate_fwd", &se_gate_fwd);
  m.impl("se_scale", &se_scale);
  m.impl("se_bwd_reduce", &se_bwd_reduce);
  m.impl("se_gate_bwd", &se_gate_bwd);
  m.impl("se_bwd_dx", &se_bwd_dx);
  m.impl("se_wgrad", &se_wgrad);
  register_engine_ops_impl(m);
}
