// Bindings of the loss kernels (loss.hip, the fused LM head) and of the auxiliary ops (aux_ops.hip,
// gram.hip): small fused losses, activations, reflect pad / nearest upsampling, the Gram matrix.
#include "bind_common.h"

namespace {
using namespace tbbind;

// ----------------------------------------------------------- cross entropy
std::vector<Tensor> ce_forward(const Tensor& logits_, const Tensor& labels_, double smoothing,
                               int64_t ignore_index) {
  const at::DeviceGuard guard = on_device_of(logits_, "logits");
  TORCH_CHECK(logits_.dim() == 2, "ce_forward expects [N, K] logits");
  Tensor logits = logits_.contiguous();
  Tensor labels = labels_.to(at::kLong).contiguous();
  const int64_t N = logits.size(0);
  const int K = (int)logits.size(1);
  auto fopt = logits.options().dtype(at::kFloat);
  Tensor rows = at::empty({3, N}, fopt);
  Tensor out = at::empty({3}, fopt);
  tbamd::ce_forward(dt_code(logits), logits.data_ptr(), labels.data_ptr<int64_t>(), N, K, (float)smoothing,
                    ignore_index, rows[0].data_ptr<float>(), rows[1].data_ptr<float>(),
                    rows[2].data_ptr<float>(), out.data_ptr<float>(), cur_stream());
  return {out, rows[1]};
}

Tensor ce_backward(const Tensor& logits_, const Tensor& labels_, const Tensor& row_lse, const Tensor& gout,
                   const Tensor& stats, double smoothing, int64_t ignore_index) {
  const at::DeviceGuard guard(logits_.device());
  Tensor logits = logits_.contiguous();
  Tensor labels = labels_.to(at::kLong).contiguous();
  Tensor g = gout.to(at::kFloat).contiguous();
  Tensor dl = at::empty_like(logits);
  tbamd::ce_backward(dt_code(logits), logits.data_ptr(), labels.data_ptr<int64_t>(),
                     row_lse.data_ptr<float>(), g.data_ptr<float>(), stats.data_ptr<float>(),
                     logits.size(0), (int)logits.size(1), (float)smoothing, ignore_index, dl.data_ptr(),
                     cur_stream());
  return dl;
}

// ------------------------------------- fused vocabulary projection + cross entropy
void check_lm_operands(const Tensor& x, const Tensor& w, const Tensor& labels, const char* op) {
  check_cuda(x, "x");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16,
              op, ": x [M, D] and weight [V, D] must be bf16");
  TORCH_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && w.is_contiguous() && x.size(1) == w.size(1) &&
                  x.size(1) % 8 == 0,
              op, ": D must be a multiple of 8, x row-major, weight contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              op, ": operands must be 16-B aligned");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.is_contiguous() &&
                  labels.numel() == x.size(0),
              op, ": labels must be a contiguous int64 [M] tensor on the device");
  TORCH_CHECK(x.size(0) < (1ll << 31) && w.size(0) < (1ll << 31), op, ": dims too large");
}

int64_t lm_loss_tile_q() { return tbamd::lm_loss_tile_q(); }

// -> {stats3 = (mean loss over valid rows, 0, n_valid), lse [M]}; no [M, V] tensor exists
std::vector<Tensor> lm_loss_forward(const Tensor& x, const Tensor& w, const Tensor& labels, int64_t ignore_index) {
  check_lm_operands(x, w, labels, "lm_loss_forward");
  const at::DeviceGuard guard(x.device());
  const int64_t M = x.size(0), V = w.size(0), K = x.size(1);
  TORCH_CHECK(V > 0, "lm_loss_forward: empty vocabulary");
  const int64_t nt = (V + tbamd::lm_loss_tile_q() - 1) / tbamd::lm_loss_tile_q();
  auto fopt = x.options().dtype(at::kFloat);
  Tensor part = at::empty({nt, M, 2}, fopt);
  Tensor rows = at::empty({4, M}, fopt);  // xy, row loss, lse, row ok
  Tensor stats = at::empty({3}, fopt);
  tbamd::lm_loss_partials(x.data_ptr(), x.stride(0), w.data_ptr(), labels.data_ptr<int64_t>(), part.data_ptr<float>(),
                          rows[0].data_ptr<float>(), (int)M, (int)V, (int)K, cur_stream());
  tbamd::lm_loss_merge(part.data_ptr<float>(), rows[0].data_ptr<float>(), labels.data_ptr<int64_t>(), (int)M, (int)nt,
                       (int)V, ignore_index, rows[1].data_ptr<float>(), rows[2].data_ptr<float>(),
                       rows[3].data_ptr<float>(), stats.data_ptr<float>(), cur_stream());
  return {stats, rows[2]};
}

// buf [M, ld] (bf16, contiguous, ld = v1 - v0 rounded up to 8) = d loss / d logits[:, v0:v1], pad columns zero
void lm_loss_dlogits(const Tensor& x, const Tensor& w, const Tensor& labels, const Tensor& lse, const Tensor& stats,
                     const Tensor& gout, int64_t v0, int64_t v1, int64_t ignore_index, const Tensor& buf) {
  check_lm_operands(x, w, labels, "lm_loss_dlogits");
  const at::DeviceGuard guard(x.device());
  const int64_t M = x.size(0), V = w.size(0), K = x.size(1);
  TORCH_CHECK(0 <= v0 && v0 < v1 && v1 <= V, "lm_loss_dlogits: bad column range");
  const int64_t ld = (v1 - v0 + 7) / 8 * 8;
  TORCH_CHECK(buf.is_cuda() && buf.scalar_type() == at::kBFloat16 && buf.dim() == 2 && buf.is_contiguous() &&
                  buf.size(0) == M && buf.size(1) == ld && reinterpret_cast<uintptr_t>(buf.data_ptr()) % 16 == 0,
              "lm_loss_dlogits: buf must be a contiguous bf16 [M, round8(v1 - v0)] tensor");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.numel() == M &&
                  stats.scalar_type() == at::kFloat && stats.is_contiguous() && stats.numel() == 3 &&
                  gout.scalar_type() == at::kFloat && gout.numel() == 1 && gout.is_cuda(),
              "lm_loss_dlogits: lse [M], stats [3], gout [1] must be f32 device tensors");
  tbamd::lm_loss_dlogits(x.data_ptr(), x.stride(0), w.data_ptr(), labels.data_ptr<int64_t>(), lse.data_ptr<float>(),
                         stats.data_ptr<float>(), gout.data_ptr<float>(), buf.data_ptr(), ld, (int)M, (int)V, (int)K,
                         (int)v0, (int)v1, ignore_index, cur_stream());
}

// ------------------------------------------- small fused losses / resampling
Tensor aux_part(const Tensor& like) { return at::empty({tbamd::aux_partials()}, like.options().dtype(at::kFloat)); }
Tensor f32_scalar(const Tensor& g) { return g.to(at::kFloat).reshape({1}).contiguous(); }
// a 4-D tensor that is channels_last and not also NCHW-contiguous: read in place
bool is_cl(const Tensor& x) { return !x.is_contiguous() && x.is_contiguous(at::MemoryFormat::ChannelsLast); }

// x: 4-D, NCHW-contiguous or channels_last
Tensor tv_forward(const Tensor& x_) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.dim() == 4, "total_variation expects [N, C, H, W]");
  const bool cl = is_cl(x_);
  Tensor x = cl ? x_ : x_.contiguous();
  Tensor out = at::empty({}, x.options().dtype(at::kFloat));
  tbamd::tv_forward(dt_code(x), x.data_ptr(), x.numel(), (int)x.size(2), (int)x.size(3), cl ? (int)x.size(1) : 1,
                    aux_part(x).data_ptr<float>(), out.data_ptr<float>(), cur_stream());
  return out;
}

Tensor tv_backward(const Tensor& x_, const Tensor& gout) {
  const at::DeviceGuard guard(x_.device());
  const bool cl = is_cl(x_);
  Tensor x = cl ? x_ : x_.contiguous();
  Tensor dx = at::empty_like(x);
  Tensor g = f32_scalar(gout);
  tbamd::tv_backward(dt_code(x), x.data_ptr(), g.data_ptr<float>(), x.numel(), (int)x.size(2), (int)x.size(3),
                     cl ? (int)x.size(1) : 1, dx.data_ptr(), cur_stream());
  return dx;
}

// y = act(x) / dx = dy * act'(x) on the storage of x (any layout the two share; numel % 8 == 0)
Tensor act_fwd(const Tensor& x_, int64_t act, double slope) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const bool cl = x_.dim() == 4 && is_cl(x_);
  Tensor x = cl ? x_ : x_.contiguous();
  TORCH_CHECK(x.numel() % 8 == 0, "act_fwd: numel must be a multiple of 8");
  Tensor y = at::empty_like(x);
  tbamd::act_forward(dt_code(x), (int)act, x.data_ptr(), y.data_ptr(), x.numel(), (float)slope, cur_stream());
  return y;
}

Tensor act_bwd(const Tensor& x_, const Tensor& dy_, int64_t act, double slope) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const bool cl = x_.dim() == 4 && is_cl(x_);
  Tensor x = cl ? x_ : x_.contiguous();
  Tensor dy = cl ? nhwc(dy_) : dy_.contiguous();
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides() && dy.scalar_type() == x.scalar_type(),
              "act_bwd: dy must match x");
  Tensor dx = at::empty_like(x);
  tbamd::act_backward(dt_code(x), (int)act, x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), (float)slope,
                      cur_stream());
  return dx;
}

// ---- SwiGLU gate (csrc/swiglu.hip).  gu: [M, 2F] packed gate | up rows, bf16 or f32, unit column
// stride, 16-B aligned rows (any row stride that keeps them so), F % 8 == 0 -> y [M, F] contiguous.
static int64_t swiglu_rows(const Tensor& gu, const char* what) {
  check_cuda(gu, "gu");
  TORCH_CHECK(gu.scalar_type() == at::kBFloat16 || gu.scalar_type() == at::kFloat, what, ": bf16 or f32 only");
  TORCH_CHECK(gu.dim() == 2 && gu.size(1) % 16 == 0 && gu.size(1) >= 16 && gu.size(1) < (int64_t)INT32_MAX,
              what, ": gu must be [M, 2F] with F % 8 == 0");
  const int64_t es = gu.element_size();
  TORCH_CHECK(gu.stride(1) == 1 && (gu.size(0) <= 1 || (gu.stride(0) >= gu.size(1) && gu.stride(0) * es % 16 == 0)) &&
                  reinterpret_cast<uintptr_t>(gu.data_ptr()) % 16 == 0,
              what, ": rows must be 16-B aligned with a unit column stride");
  return gu.size(0) <= 1 ? gu.size(1) : gu.stride(0);
}

Tensor swiglu_fwd(const Tensor& gu) {
  const at::DeviceGuard guard = on_device_of(gu, "gu");
  const int64_t sgu = swiglu_rows(gu, "swiglu_fwd");
  const int64_t M = gu.size(0), F = gu.size(1) / 2;
  Tensor y = at::empty({M, F}, gu.options().memory_format(at::MemoryFormat::Contiguous));
  tbamd::swiglu_forward(dt_code(gu), gu.data_ptr(), sgu, M, (int)F, y.data_ptr(), cur_stream());
  return y;
}

// dy [M, F] contiguous, the dtype of gu -> dgu [M, 2F] contiguous (dgate | dup), recomputed from gu
Tensor swiglu_bwd(const Tensor& gu, const Tensor& dy) {
  const at::DeviceGuard guard = on_device_of(gu, "gu");
  const int64_t sgu = swiglu_rows(gu, "swiglu_bwd");
  const int64_t M = gu.size(0), F = gu.size(1) / 2;
  check_cuda(dy, "dy");
  TORCH_CHECK(dy.scalar_type() == gu.scalar_type() && dy.dim() == 2 && dy.size(0) == M && dy.size(1) == F &&
                  dy.is_contiguous() && dy.device() == gu.device() &&
                  reinterpret_cast<uintptr_t>(dy.data_ptr()) % 16 == 0,
              "swiglu_bwd: dy must be contiguous, 16-B aligned [M, F] in the dtype and on the device of gu");
  Tensor dgu = at::empty({M, 2 * F}, gu.options().memory_format(at::MemoryFormat::Contiguous));
  tbamd::swiglu_backward(dt_code(gu), gu.data_ptr(), sgu, dy.data_ptr(), M, (int)F, dgu.data_ptr(), cur_stream());
  return dgu;
}

Tensor hinge_forward(const Tensor& x_, double margin, double sign) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = x_.contiguous();
  Tensor out = at::empty({}, x.options().dtype(at::kFloat));
  tbamd::hinge_forward(dt_code(x), x.data_ptr(), x.numel(), (float)margin, (float)sign,
                       aux_part(x).data_ptr<float>(), out.data_ptr<float>(), cur_stream());
  return out;
}

Tensor hinge_backward(const Tensor& x_, const Tensor& gout, double margin, double sign) {
  const at::DeviceGuard guard(x_.device());
  Tensor x = x_.contiguous();
  Tensor dx = at::empty_like(x);
  Tensor g = f32_scalar(gout);
  tbamd::hinge_backward(dt_code(x), x.data_ptr(), g.data_ptr<float>(), x.numel(), (float)margin, (float)sign,
                        dx.data_ptr(), cur_stream());
  return dx;
}

Tensor bce_logits_forward(const Tensor& x_, const Tensor& y_) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.numel() == y_.numel(), "bce_with_logits: input and target sizes differ");
  Tensor x = x_.contiguous();
  Tensor y = y_.to(x.scalar_type()).contiguous();
  Tensor out = at::empty({}, x.options().dtype(at::kFloat));
  tbamd::bce_logits_forward(dt_code(x), x.data_ptr(), y.data_ptr(), x.numel(), aux_part(x).data_ptr<float>(),
                            out.data_ptr<float>(), cur_stream());
  return out;
}

Tensor bce_logits_backward(const Tensor& x_, const Tensor& y_, const Tensor& gout) {
  const at::DeviceGuard guard(x_.device());
  Tensor x = x_.contiguous();
  Tensor y = y_.to(x.scalar_type()).contiguous();
  Tensor dx = at::empty_like(x);
  Tensor g = f32_scalar(gout);
  tbamd::bce_logits_backward(dt_code(x), x.data_ptr(), y.data_ptr(), g.data_ptr<float>(), x.numel(),
                             dx.data_ptr(), cur_stream());
  return dx;
}

Tensor kld_forward(const Tensor& mu_, const Tensor& lv_) {
  const at::DeviceGuard guard = on_device_of(mu_, "mu");
  TORCH_CHECK(mu_.sizes() == lv_.sizes() && mu_.dim() == 2, "kld expects matching [B, D] mu / log_var");
  Tensor mu = mu_.contiguous();
  Tensor lv = lv_.to(mu.scalar_type()).contiguous();
  Tensor out = at::empty({}, mu.options().dtype(at::kFloat));
  tbamd::kld_forward(dt_code(mu), mu.data_ptr(), lv.data_ptr(), mu.numel(), mu.size(0),
                     aux_part(mu).data_ptr<float>(), out.data_ptr<float>(), cur_stream());
  return out;
}

std::vector<Tensor> kld_backward(const Tensor& mu_, const Tensor& lv_, const Tensor& gout) {
  const at::DeviceGuard guard(mu_.device());
  Tensor mu = mu_.contiguous();
  Tensor lv = lv_.to(mu.scalar_type()).contiguous();
  Tensor dmu = at::empty_like(mu), dlv = at::empty_like(lv);
  Tensor g = f32_scalar(gout);
  tbamd::kld_backward(dt_code(mu), mu.data_ptr(), lv.data_ptr(), g.data_ptr<float>(), mu.numel(), mu.size(0),
                      dmu.data_ptr(), dlv.data_ptr(), cur_stream());
  return {dmu, dlv};
}

// x [N, C, H, W] (NCHW-contiguous or channels_last) -> f32 mean, unbiased std+eps: [N, C]
std::vector<Tensor> mean_std_forward(const Tensor& x_, double eps) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.dim() == 4, "mean_std expects [N, C, H, W]");
  const bool cl = is_cl(x_);
  Tensor x = cl ? x_ : x_.contiguous();
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int64_t S = x.size(2) * x.size(3);
  auto fo = x.options().dtype(at::kFloat);
  Tensor mean = at::empty({N, C}, fo), sd = at::empty({N, C}, fo);
  const int64_t wsz = tbamd::mean_std_workspace(N, C, S, cl);
  Tensor ws = wsz > 0 ? at::empty({wsz}, fo) : Tensor();
  if (x.numel() > 0)
    tbamd::mean_std_forward(dt_code(x), x.data_ptr(), N, C, S, cl, (float)eps, mean.data_ptr<float>(),
                            sd.data_ptr<float>(), cur_stream(), wsz > 0 ? ws.data_ptr<float>() : nullptr);
  return {mean, sd};
}

Tensor mean_std_backward(const Tensor& x_, const Tensor& mean, const Tensor& sd, const Tensor& dmean_,
                         const Tensor& dstd_) {
  const at::DeviceGuard guard(x_.device());
  const bool cl = is_cl(x_);
  Tensor x = cl ? x_ : x_.contiguous();
  Tensor dmean = dmean_.to(at::kFloat).contiguous(), dstd = dstd_.to(at::kFloat).contiguous();
  Tensor dx = at::empty_like(x);
  Tensor coef = at::empty({2 * x.size(0) * x.size(1)}, mean.options());
  if (x.numel() > 0)
    tbamd::mean_std_backward(dt_code(x), x.data_ptr(), mean.data_ptr<float>(), sd.data_ptr<float>(),
                             dmean.data_ptr<float>(), dstd.data_ptr<float>(), (int)x.size(0), (int)x.size(1),
                             x.size(2) * x.size(3), cl, dx.data_ptr(), cur_stream(), coef.data_ptr<float>());
  return dx;
}

// NHWC-only (channels_last) resampling; returns a channels_last [N, C, Ho, Wo] tensor
Tensor nhwc_in(const Tensor& x) {
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "expected a channels_last [N, C, H, W] tensor");
  return x;
}

Tensor reflect_pad_forward(const Tensor& x_, int64_t pl, int64_t pr, int64_t pt, int64_t pb) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = nhwc_in(x_);
  const int N = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(pt < H && pb < H && pl < W && pr < W && pl >= 0 && pr >= 0 && pt >= 0 && pb >= 0,
              "reflection padding must be smaller than the input size");
  Tensor y = at::empty({N, C, H + pt + pb, W + pl + pr}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (y.numel() > 0)
    tbamd::reflect_pad_forward(dt_code(x), x.data_ptr(), N, H, W, C, (int)pt, (int)pb, (int)pl, (int)pr,
                               y.data_ptr(), cur_stream());
  return y;
}

Tensor reflect_pad_backward(const Tensor& dy_, int64_t H, int64_t W, int64_t pl, int64_t pr, int64_t pt,
                            int64_t pb) {
  const at::DeviceGuard guard(dy_.device());
  Tensor dy = nhwc(dy_);
  const int N = (int)dy.size(0), C = (int)dy.size(1);
  Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (dx.numel() > 0)
    tbamd::reflect_pad_backward(dt_code(dy), dy.data_ptr(), N, (int)H, (int)W, C, (int)pt, (int)pb, (int)pl,
                                (int)pr, dx.data_ptr(), cur_stream());
  return dx;
}

Tensor upsample_nearest_forward(const Tensor& x_, int64_t f) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = nhwc_in(x_);
  TORCH_CHECK(f >= 1, "upsample factor must be >= 1");
  const int N = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  Tensor y = at::empty({N, C, H * f, W * f}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (y.numel() > 0)
    tbamd::upsample_nearest_forward(dt_code(x), x.data_ptr(), N, H, W, C, (int)f, y.data_ptr(), cur_stream());
  return y;
}

Tensor upsample_nearest_backward(const Tensor& dy_, int64_t f) {
  const at::DeviceGuard guard(dy_.device());
  Tensor dy = nhwc(dy_);
  const int N = (int)dy.size(0), C = (int)dy.size(1), H = (int)(dy.size(2) / f), W = (int)(dy.size(3) / f);
  Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (dx.numel() > 0)
    tbamd::upsample_nearest_backward(dt_code(dy), dy.data_ptr(), N, H, W, C, (int)f, dx.data_ptr(),
                                     cur_stream());
  return dx;
}

// ------------------------------------------------------------ Gram matrix
// f: [B, C, H, W] bf16 channels_last (NHWC memory) -> [B, C, C] f32 = F_b^T F_b * scale
Tensor gram_forward(const Tensor& f, double scale) {
  const at::DeviceGuard guard = on_device_of(f, "features");
  TORCH_CHECK(f.scalar_type() == at::kBFloat16 && f.dim() == 4 && f.is_contiguous(at::MemoryFormat::ChannelsLast),
              "gram: expected bf16 channels_last [B, C, H, W]");
  const int B = (int)f.size(0), C = (int)f.size(1);
  const int64_t HW = f.size(2) * f.size(3);
  TORCH_CHECK(tbamd::gram_tile(C) > 0, "gram: C must be a multiple of 64");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(f.data_ptr()) % 16 == 0, "gram: features not 16-B aligned");
  Tensor ws = at::empty({tbamd::gram_workspace(B, C, HW)}, f.options().dtype(at::kFloat));
  Tensor out = at::empty({B, C, C}, f.options().dtype(at::kFloat));
  tbamd::gram(f.data_ptr(), B, HW, C, (float)scale, ws.data_ptr<float>(), out.data_ptr<float>(), cur_stream());
  return out;
}

// [B][C][C] f32 gradient of the Gram -> bf16 (dG + dG^T) * scale
Tensor gram_sym(const Tensor& dg, double scale) {
  TORCH_CHECK(dg.is_cuda() && dg.dtype() == at::kFloat && dg.dim() == 3 && dg.size(1) == dg.size(2),
              "gram_sym: expected f32 [B, C, C]");
  Tensor d = dg.contiguous();
  Tensor out = at::empty(d.sizes(), d.options().dtype(at::kBFloat16));
  tbamd::gram_sym(d.data_ptr<float>(), out.data_ptr(), (int)d.size(0), (int)d.size(1), (float)scale, cur_stream());
  return out;
}

}  // namespace

void register_loss(pybind11::module& m) {
  m.def("ce_forward", &ce_forward);
  m.def("ce_backward", &ce_backward);
  m.def("lm_loss_tile_q", &lm_loss_tile_q);
  m.def("lm_loss_forward", &lm_loss_forward);
  m.def("lm_loss_dlogits", &lm_loss_dlogits);
  m.def("tv_forward", &tv_forward);
  m.def("tv_backward", &tv_backward);
  m.def("act_fwd", &act_fwd, py::arg("x"), py::arg("act"), py::arg("slope") = 0.01);
  m.def("act_bwd", &act_bwd, py::arg("x"), py::arg("dy"), py::arg("act"), py::arg("slope") = 0.01);
  m.def("swiglu_fwd", &swiglu_fwd, py::arg("gu"));
  m.def("swiglu_bwd", &swiglu_bwd, py::arg("gu"), py::arg("dy"));
  m.def("hinge_forward", &hinge_forward);
  m.def("hinge_backward", &hinge_backward);
  m.def("bce_logits_forward", &bce_logits_forward);
  m.def("bce_logits_backward", &bce_logits_backward);
  m.def("kld_forward", &kld_forward);
  m.def("kld_backward", &kld_backward);
  m.def("mean_std_forward", &mean_std_forward);
  m.def("mean_std_backward", &mean_std_backward);
  m.def("reflect_pad_forward", &reflect_pad_forward);
  m.def("reflect_pad_backward", &reflect_pad_backward);
  m.def("upsample_nearest_forward", &upsample_nearest_forward);
  m.def("upsample_nearest_backward", &upsample_nearest_backward);
  m.def("gram_forward", &gram_forward);
  m.def("gram_sym", &gram_sym);
}
