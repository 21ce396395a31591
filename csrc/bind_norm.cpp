// Bindings of the normalisation and pooling kernels (norm_bn.hip, layernorm.hip, pool.hip):
// BatchNorm in all its forms, GroupNorm, LayerNorm, the fused BN + max-pool, global average pool.
#include "bind_common.h"

namespace {
using namespace tbbind;

// ---------------------------------------------------------------- BatchNorm
// ReLU-after-residual bit mask [M, C/8] (uint8) when requested and applicable
Tensor make_mask(const Tensor& x, const Tensor& res, int64_t act, bool want) {
  if (!want || !res.defined() || act != 1 || x.size(1) % 8 != 0) return Tensor();
  return at::empty({x.size(0), x.size(1) / 8}, x.options().dtype(at::kByte));
}

Tensor rows_or_undef(const optional<Tensor>& t) { return given(t) ? as_rows(*t) : Tensor(); }

int64_t* nbt_ptr(const optional<Tensor>& t) {
  if (!given(t)) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kLong && t->numel() == 1 && t->is_cuda(), "num_batches_tracked: int64 scalar");
  return t->data_ptr<int64_t>();
}

std::vector<Tensor> bn_forward(const Tensor& x_, const optional<Tensor>& weight,
                               const optional<Tensor>& bias, const optional<Tensor>& running_mean,
                               const optional<Tensor>& running_var, bool training, double momentum,
                               double eps, const optional<Tensor>& residual, int64_t act, double slope,
                               const optional<Tensor>& num_batches_tracked, bool want_mask) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.dim() == 2, "bn_forward expects [M, C]");
  Tensor x = as_rows(x_);
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  auto fopt = x.options().dtype(at::kFloat);
  Tensor mean = at::empty({C}, fopt), invstd = at::empty({C}, fopt);
  Tensor scale = at::empty({C}, fopt), shift = at::empty({C}, fopt);
  auto st = cur_stream();
  Tensor wf = f32_or_undef(weight), bf = f32_or_undef(bias);
  const float *g = f32_or_null(wf), *b = f32_or_null(bf);
  if (training) {
    TORCH_CHECK(M > 0, "bn_forward: empty batch in training mode");
    const int nblk = tbamd::bn_partial_blocks(M, C);
    const int prows = tbamd::bn_stats_rows(dt_code(x), nblk);  // f32 input: + the rounding-remainder rows
    Tensor ws = at::empty({2, (int64_t)prows, C}, fopt);
    Tensor fws = at::empty({tbamd::colsum_workspace(prows, C)}, x.options().dtype(at::kDouble));
    tbamd::bn_forward_train(dt_code(x), x.data_ptr(), M, C, g, b, fptr_mut(running_mean),
                            fptr_mut(running_var), nbt_ptr(num_batches_tracked), (float)momentum, (float)eps,
                            ws[0].data_ptr<float>(), ws[1].data_ptr<float>(), nblk, fws.data_ptr<double>(),
                            mean.data_ptr<float>(), invstd.data_ptr<float>(), scale.data_ptr<float>(),
                            shift.data_ptr<float>(), st);
  } else {
    TORCH_CHECK(running_mean.has_value() && running_var.has_value(), "eval BN needs running stats");
    tbamd::bn_eval_coeffs(C, g, b, fptr(running_mean), fptr(running_var), (float)eps, mean.data_ptr<float>(),
                          invstd.data_ptr<float>(), scale.data_ptr<float>(), shift.data_ptr<float>(), st);
  }
  Tensor res = rows_or_undef(residual);
  TORCH_CHECK(!res.defined() || (res.sizes() == x.sizes() && res.scalar_type() == x.scalar_type()), "residual mismatch");
  Tensor y = at::empty_like(x);
  Tensor mask = make_mask(x, res, act, want_mask);
  if (M > 0)
    tbamd::bn_apply(dt_code(x), x.data_ptr(), ptr_or_null(res), scale.data_ptr<float>(), shift.data_ptr<float>(), M, C,
                    (int)act, (float)slope, y.data_ptr(), mask.defined() ? mask.data_ptr<uint8_t>() : nullptr, st);
  return {y, mean, invstd, scale, shift, mask};
}

std::vector<Tensor> bn_backward(const Tensor& dy_, const Tensor& y_, const Tensor& x_,
                                const optional<Tensor>& residual, const optional<Tensor>& weight,
                                const Tensor& mean, const Tensor& invstd, const Tensor& scale,
                                const Tensor& shift, bool training, int64_t act, double slope,
                                bool need_dres, const optional<Tensor>& dgamma_out,
                                const optional<Tensor>& dbeta_out, const optional<Tensor>& mask) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor x = as_rows(x_);
  Tensor dy = as_rows(dy_.to(x.scalar_type()));
  Tensor y = as_rows(y_);
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  auto fopt = x.options().dtype(at::kFloat);
  Tensor res = rows_or_undef(residual);
  Tensor wf = f32_or_undef(weight);
  const int nblk = tbamd::bn_partial_blocks(M, C);
  Tensor ws = at::empty({2, (int64_t)nblk, C}, fopt);
  Tensor fws = at::empty({tbamd::colsum_workspace(nblk, C)}, x.options().dtype(at::kDouble));
  Tensor coef = at::empty({3, C}, fopt);
  Tensor dgamma = slot_or_new(dgamma_out, C, fopt, "bn_backward"), dbeta = slot_or_new(dbeta_out, C, fopt, "bn_backward");
  Tensor dx = at::empty_like(x);
  const uint8_t* maskin = nullptr;
  if (given(mask)) {
    // act 1: this BN's own ReLU-after-residual mask; act 0: dy is a carrier whose mask comes from the
    // block-output BN downstream (ops/norm.py ResidualGradLink carrier: the downsample branch's BN)
    TORCH_CHECK((act == 1 || act == 0) && C % 8 == 0 && mask->numel() == M * (C / 8) &&
                    mask->scalar_type() == at::kByte,
                "bn_backward: mask needs ReLU or no activation, C % 8 == 0 and [M, C/8] bytes");
    maskin = mask->data_ptr<uint8_t>();
    need_dres = false;  // the residual's consumer applies the mask to dy itself
  }
  Tensor dres;
  if (need_dres) dres = at::empty_like(x);
  if (M > 0)
    tbamd::bn_backward(dt_code(x), dy.data_ptr(), y.data_ptr(), x.data_ptr(), ptr_or_null(res), M, C, (int)act,
                       (float)slope, f32_or_null(wf), mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       scale.data_ptr<float>(), shift.data_ptr<float>(), training ? 1 : 0, ws[0].data_ptr<float>(),
                       ws[1].data_ptr<float>(), nblk, fws.data_ptr<double>(), coef.data_ptr<float>(),
                       dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), ptr_or_null(dres), dx.data_ptr(), maskin,
                       cur_stream());
  else {
    dgamma.zero_();
    dbeta.zero_();
  }
  return {dx, dgamma, dbeta, dres};
}

// BN backward whose partial sums were emitted by the dgrad epilogue (conv2d_fwd bnb_mode)
std::vector<Tensor> bn_backward_from_partials(const Tensor& dy_, const Tensor& x_, const Tensor& part,
                                              const optional<Tensor>& weight, const Tensor& mean,
                                              const Tensor& invstd, const Tensor& scale, const Tensor& shift,
                                              bool training, int64_t act, double slope,
                                              const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out,
                                              const optional<Tensor>& mask, bool want_dres,
                                              const optional<Tensor>& ds_x, const optional<Tensor>& ds_mean) {
  // want_dres (ReLU-after-residual with saved mask bits): also returns dres = dy * mask
  // ds_x / ds_mean (the residual is a downsample branch: its BN input rows and batch mean): also
  // returns that BN's backward partials [rows][2][C] from this apply pass (ops/norm.py carrier)
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor x = as_rows(x_);
  Tensor dy = as_rows(dy_.to(x.scalar_type()));
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(part.dim() == 3 && part.size(1) == 2 && part.size(2) == C, "bn_backward_from_partials: part");
  auto fopt = x.options().dtype(at::kFloat);
  Tensor wf = f32_or_undef(weight);
  Tensor dgamma = slot_or_new(dgamma_out, C, fopt, "bn_backward_from_partials");
  Tensor dbeta = slot_or_new(dbeta_out, C, fopt, "bn_backward_from_partials");
  Tensor coef = at::empty({3, C}, fopt);
  Tensor fws = at::empty({tbamd::colsum_workspace((int)part.size(0), C)}, x.options().dtype(at::kDouble));
  const uint8_t* maskin = nullptr;
  if (given(mask)) maskin = mask->data_ptr<uint8_t>();
  Tensor dx = at::empty_like(x);
  Tensor dres;
  if (want_dres) {
    TORCH_CHECK(maskin != nullptr && act == 1 && C % 8 == 0, "bn_backward_from_partials: dres needs the ReLU mask");
    dres = at::empty_like(x);
  }
  Tensor dsx, dsp;
  if (given(ds_x)) {
    dsx = as_rows(*ds_x);
    TORCH_CHECK(dsx.scalar_type() == x.scalar_type() && dsx.size(0) == M && dsx.size(1) == C && maskin &&
                    act == 1 && C % 8 == 0 && !want_dres && given(ds_mean) &&
                    ds_mean->scalar_type() == at::kFloat && ds_mean->numel() == C && ds_mean->is_contiguous(),
                "bn_backward_from_partials: downsample partials need rows like x, f32 [C] mean, the ReLU mask");
    dsp = at::empty({tbamd::bn_bwd_dsp_rows(M, C), 2, C}, fopt);
  }
  tbamd::bn_backward_from_partials(dt_code(x), dy.data_ptr(), x.data_ptr(), x.data_ptr(), M, C, (int)act,
                                   (float)slope, f32_or_null(wf),
                                   mean.data_ptr<float>(), invstd.data_ptr<float>(), scale.data_ptr<float>(),
                                   shift.data_ptr<float>(), training ? 1 : 0, part.data_ptr<float>(),
                                   (int)part.size(0), fws.data_ptr<double>(), coef.data_ptr<float>(),
                                   dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), dx.data_ptr(), maskin,
                                   cur_stream(), ptr_or_null(dres), ptr_or_null(dsx),
                                   dsx.defined() ? ds_mean->data_ptr<float>() : nullptr, f32_or_null(dsp));
  return {dx, dgamma, dbeta, dres, dsp};
}

// deferred BN backward: the finalize only (coef [3, C], dgamma, dbeta) from the dgrad partials
std::vector<Tensor> bn_backward_coef(const Tensor& part, const optional<Tensor>& weight, const Tensor& mean,
                                     const Tensor& invstd, int64_t M, bool training,
                                     const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out) {
  const at::DeviceGuard guard = on_device_of(part, "part");
  TORCH_CHECK(part.dim() == 3 && part.size(1) == 2 && part.scalar_type() == at::kFloat && part.is_contiguous(),
              "bn_backward_coef: part [rows, 2, C] f32");
  const int C = (int)part.size(2);
  auto fopt = part.options();
  Tensor wf = f32_or_undef(weight);
  Tensor dgamma = slot_or_new(dgamma_out, C, fopt, "bn_backward_coef");
  Tensor dbeta = slot_or_new(dbeta_out, C, fopt, "bn_backward_coef");
  Tensor coef = at::empty({3, C}, fopt);
  Tensor fws = at::empty({tbamd::colsum_workspace((int)part.size(0), C)}, fopt.dtype(at::kDouble));
  tbamd::bn_backward_coef(part.data_ptr<float>(), (int)part.size(0), M, C, f32_or_null(wf),
                          mean.data_ptr<float>(), invstd.data_ptr<float>(), training ? 1 : 0, fws.data_ptr<double>(),
                          coef.data_ptr<float>(), dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), cur_stream());
  return {coef, dgamma, dbeta};
}

// the deferred apply when the consumer conv cannot take it: dx = ka * act'(z) * dy + c0 + c1 * x
Tensor bn_backward_apply_coef(const Tensor& dy_, const Tensor& x_, const Tensor& coef, const Tensor& scale,
                              const Tensor& shift, int64_t act, double slope, const optional<Tensor>& mask) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  TORCH_CHECK(dy_.dim() == 2 && x_.dim() == 2, "bn_backward_apply_coef: [M, C] rows");
  Tensor x = as_rows(x_);
  Tensor dy = as_rows(dy_.to(x.scalar_type()));
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(dy.size(0) == M && dy.size(1) == C && coef.numel() == 3 * C && coef.scalar_type() == at::kFloat &&
                  coef.is_contiguous(), "bn_backward_apply_coef: shapes");
  const uint8_t* maskin = nullptr;
  if (given(mask)) {
    TORCH_CHECK(mask->numel() == M * (C / 8) && C % 8 == 0, "bn_backward_apply_coef: mask");
    maskin = mask->data_ptr<uint8_t>();
  }
  Tensor dx = at::empty_like(x);
  tbamd::bn_backward_apply_coef(dt_code(x), dy.data_ptr(), x.data_ptr(), M, C, (int)act, (float)slope,
                                scale.data_ptr<float>(), shift.data_ptr<float>(), coef.data_ptr<float>(),
                                dx.data_ptr(), maskin, cur_stream());
  return dx;
}

// BN apply (+ residual, activation, optional 1-bit ReLU mask) with coefficients computed
// elsewhere: coeff [4, C] = mean, invstd, scale, shift.  Returns [y, mask].
std::vector<Tensor> bn_apply_coeff(const Tensor& x_, const Tensor& coeff, const optional<Tensor>& residual,
                                   int64_t act, double slope, bool want_mask) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = as_rows(x_);
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(coeff.dim() == 2 && coeff.size(0) == 4 && coeff.size(1) == C && coeff.scalar_type() == at::kFloat &&
                  coeff.is_contiguous(),
              "bn_apply_coeff: coeff [4, C] f32");
  Tensor res = rows_or_undef(residual);
  Tensor y = at::empty_like(x);
  Tensor mask = make_mask(x, res, act, want_mask);
  tbamd::bn_apply(dt_code(x), x.data_ptr(), ptr_or_null(res), coeff[2].data_ptr<float>(),
                  coeff[3].data_ptr<float>(), M, C, (int)act, (float)slope, y.data_ptr(),
                  mask.defined() ? mask.data_ptr<uint8_t>() : nullptr, cur_stream());
  return {y, mask};
}

// BN forward when the statistics come from the conv epilogue
std::vector<Tensor> bn_forward_from_stats(const Tensor& x_, const Tensor& stats, const optional<Tensor>& weight,
                                          const optional<Tensor>& bias, const optional<Tensor>& running_mean,
                                          const optional<Tensor>& running_var, double momentum, double eps,
                                          const optional<Tensor>& residual, int64_t act, double slope,
                                          const optional<Tensor>& num_batches_tracked, bool want_mask,
                                          const optional<Tensor>& res_scale, const optional<Tensor>& res_shift) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = as_rows(x_);
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(stats.dim() == 3 && stats.size(1) == 2 && stats.size(2) == C, "bn_forward_from_stats: stats shape");
  // res_scale / res_shift: the residual is the input of a BN without activation (its coefficients),
  // added as res * res_scale + res_shift (the bottleneck downsample branch, ops/norm.py)
  const bool resaff = given(res_scale);
  if (resaff)
    TORCH_CHECK(given(res_shift) && res_scale->scalar_type() == at::kFloat &&
                    res_shift->scalar_type() == at::kFloat && res_scale->is_contiguous() && res_shift->is_contiguous() &&
                    res_scale->numel() == C && res_shift->numel() == C && want_mask && act == 1 && C % 8 == 0 &&
                    given(residual),
                "bn_forward_from_stats: an affine residual needs f32 [C] scale / shift, ReLU, a mask, C % 8 == 0");
  auto fopt = x.options().dtype(at::kFloat);
  Tensor coeff = at::empty({4, C}, fopt);
  Tensor fws = at::empty({tbamd::colsum_workspace((int)stats.size(0), C)}, x.options().dtype(at::kDouble));
  Tensor wf = f32_or_undef(weight), bf = f32_or_undef(bias);
  auto st = cur_stream();
  tbamd::bn_finalize_from_conv(stats.data_ptr<float>(), (int)stats.size(0), M, C, f32_or_null(wf), f32_or_null(bf),
                               fptr_mut(running_mean), fptr_mut(running_var), nbt_ptr(num_batches_tracked),
                               (float)momentum, (float)eps, fws.data_ptr<double>(), coeff[0].data_ptr<float>(),
                               coeff[1].data_ptr<float>(), coeff[2].data_ptr<float>(), coeff[3].data_ptr<float>(), st);
  Tensor res = rows_or_undef(residual);
  Tensor y = at::empty_like(x);
  Tensor mask = make_mask(x, res, act, want_mask);
  tbamd::bn_apply(dt_code(x), x.data_ptr(), ptr_or_null(res), coeff[2].data_ptr<float>(),
                  coeff[3].data_ptr<float>(), M, C, (int)act, (float)slope, y.data_ptr(),
                  mask.defined() ? mask.data_ptr<uint8_t>() : nullptr, st,
                  resaff ? res_scale->data_ptr<float>() : nullptr, resaff ? res_shift->data_ptr<float>() : nullptr);
  return {y, coeff[0], coeff[1], coeff[2], coeff[3], mask};
}

// ------------------------------------------------ BN statistics + fused max-pool
// Statistics only (training: from the conv-epilogue partials `stats` when
// given, else a partial pass over x; eval: running stats) -> [mean, invstd,
// scale, shift].  x: [M, C] rows.
std::vector<Tensor> bn_stats(const Tensor& x_, const optional<Tensor>& stats, const optional<Tensor>& weight,
                             const optional<Tensor>& bias, const optional<Tensor>& running_mean,
                             const optional<Tensor>& running_var, bool training, double momentum, double eps,
                             const optional<Tensor>& num_batches_tracked) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.dim() == 2, "bn_stats expects [M, C]");
  Tensor x = as_rows(x_);
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  auto fopt = x.options().dtype(at::kFloat);
  Tensor coeff = at::empty({4, C}, fopt);
  Tensor wf = f32_or_undef(weight), bf = f32_or_undef(bias);
  const float *g = f32_or_null(wf), *b = f32_or_null(bf);
  float *mean = coeff[0].data_ptr<float>(), *invstd = coeff[1].data_ptr<float>();
  float *scale = coeff[2].data_ptr<float>(), *shift = coeff[3].data_ptr<float>();
  auto st = cur_stream();
  if (!training) {
    TORCH_CHECK(running_mean.has_value() && running_var.has_value(), "eval BN needs running stats");
    tbamd::bn_eval_coeffs(C, g, b, fptr(running_mean), fptr(running_var), (float)eps, mean, invstd, scale, shift,
                          st);
  } else if (given(stats)) {
    TORCH_CHECK(stats->dim() == 3 && stats->size(1) == 2 && stats->size(2) == C, "bn_stats: stats shape");
    Tensor fws = at::empty({tbamd::colsum_workspace((int)stats->size(0), C)}, x.options().dtype(at::kDouble));
    tbamd::bn_finalize_from_conv(stats->data_ptr<float>(), (int)stats->size(0), M, C, g, b, fptr_mut(running_mean),
                                 fptr_mut(running_var), nbt_ptr(num_batches_tracked), (float)momentum, (float)eps,
                                 fws.data_ptr<double>(), mean, invstd, scale, shift, st);
  } else {
    TORCH_CHECK(M > 0, "bn_stats: empty batch in training mode");
    const int nblk = tbamd::bn_partial_blocks(M, C);
    const int prows = tbamd::bn_stats_rows(dt_code(x), nblk);  // f32 input: + the rounding-remainder rows
    Tensor ws = at::empty({2, (int64_t)prows, C}, fopt);
    Tensor fws = at::empty({tbamd::colsum_workspace(prows, C)}, x.options().dtype(at::kDouble));
    tbamd::bn_forward_train(dt_code(x), x.data_ptr(), M, C, g, b, fptr_mut(running_mean), fptr_mut(running_var),
                            nbt_ptr(num_batches_tracked), (float)momentum, (float)eps, ws[0].data_ptr<float>(),
                            ws[1].data_ptr<float>(), nblk, fws.data_ptr<double>(), mean, invstd, scale, shift, st);
  }
  return {coeff[0], coeff[1], coeff[2], coeff[3]};
}

// y = maxpool(act(x * scale + shift)) for NHWC x [N, C, H, W] (channels_last);
// returns [y, argmax uint8 (same shape as y)]
std::vector<Tensor> bn_act_maxpool(const Tensor& x_, const Tensor& scale, const Tensor& shift, int64_t act,
                                   double slope, int64_t k, int64_t s, int64_t pad) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.dim() == 4 && x_.size(1) % 8 == 0, "bn_act_maxpool: NCHW with C % 8 == 0");
  Tensor x = nhwc(x_);
  const int N = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  const int P = (H + 2 * (int)pad - (int)k) / (int)s + 1, Q = (W + 2 * (int)pad - (int)k) / (int)s + 1;
  TORCH_CHECK(P > 0 && Q > 0 && k <= 16 && pad < k, "bn_act_maxpool: bad window");
  Tensor y = at::empty({N, C, P, Q}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  Tensor idx = at::empty({N, C, P, Q}, x.options().dtype(at::kByte).memory_format(at::MemoryFormat::ChannelsLast));
  tbamd::bn_act_maxpool_fwd(dt_code(x), x.data_ptr(), scale.data_ptr<float>(), shift.data_ptr<float>(), (int)act,
                            (float)slope, N, H, W, C, (int)k, (int)s, (int)pad, y.data_ptr(),
                            idx.data_ptr<uint8_t>(), cur_stream());
  return {y, idx};
}

// input gradient of the max-pool from the saved argmax (gather, no atomics)
Tensor maxpool_backward(const Tensor& dy_, const Tensor& idx, int64_t H, int64_t W, int64_t k, int64_t s,
                        int64_t pad) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor dy = nhwc(dy_);
  TORCH_CHECK(idx.sizes() == dy.sizes() && idx.is_contiguous(at::MemoryFormat::ChannelsLast), "maxpool_backward: idx");
  const int N = (int)dy.size(0), C = (int)dy.size(1);
  Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  tbamd::maxpool_bwd(dt_code(dy), dy.data_ptr(), idx.data_ptr<uint8_t>(), N, (int)H, (int)W, C, (int)k, (int)s,
                     (int)pad, dx.data_ptr(), cur_stream());
  return dx;
}

// BN backward of maxpool(act(BN(x))) from the POOLED gradient (csrc/pool_gather.h): the pool
// input's gradient is gathered inside the BN partial / apply passes, never materialised.
// x: the BN input rows [N*H*W, C]; returns (dx rows, dgamma, dbeta)
std::vector<Tensor> bn_backward_pool(const Tensor& dy_, const Tensor& idx, const Tensor& x_, int64_t N, int64_t H,
                                     int64_t W, int64_t k, int64_t s, int64_t pad, const optional<Tensor>& weight,
                                     const Tensor& mean, const Tensor& invstd, const Tensor& scale,
                                     const Tensor& shift, bool training, int64_t act, double slope,
                                     const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor x = as_rows(x_);
  Tensor dy = nhwc(dy_.to(x.scalar_type()));
  const int C = (int)x.size(1);
  const int64_t M = x.size(0);
  const int P = (int)((H + 2 * pad - k) / s + 1), Q = (int)((W + 2 * pad - k) / s + 1);
  TORCH_CHECK(C % 8 == 0 && M == N * H * W && dy.dim() == 4 && dy.size(0) == N && dy.size(1) == C &&
                  dy.size(2) == P && dy.size(3) == Q,
              "bn_backward_pool: shapes");
  TORCH_CHECK(idx.sizes() == dy.sizes() && idx.scalar_type() == at::kByte &&
                  idx.is_contiguous(at::MemoryFormat::ChannelsLast),
              "bn_backward_pool: idx");
  TORCH_CHECK(tbamd::bn_backward_pool_ok((int)H, (int)W, C, (int)k, (int)s, (int)pad), "bn_backward_pool: shape "
              "(3x3/2 pad 1, even H and W, C/8 channel groups dividing 256)");
  auto fopt = x.options().dtype(at::kFloat);
  Tensor wf = f32_or_undef(weight);
  const int nblk = tbamd::bn_backward_pool_blocks((int)N, (int)H, (int)W, C);
  Tensor ws = at::empty({2, (int64_t)nblk, C}, fopt);
  Tensor fws = at::empty({tbamd::colsum_workspace(nblk, C)}, x.options().dtype(at::kDouble));
  Tensor coef = at::empty({3, C}, fopt);
  Tensor dgamma = slot_or_new(dgamma_out, C, fopt, "bn_backward_pool");
  Tensor dbeta = slot_or_new(dbeta_out, C, fopt, "bn_backward_pool");
  Tensor dx = at::empty_like(x);
  if (M > 0)
    tbamd::bn_backward_pool(dt_code(x), dy.data_ptr(), idx.data_ptr<uint8_t>(), x.data_ptr(), (int)N, (int)H, (int)W,
                            C, (int)k, (int)s, (int)pad, (int)act, (float)slope, f32_or_null(wf),
                            mean.data_ptr<float>(), invstd.data_ptr<float>(), scale.data_ptr<float>(),
                            shift.data_ptr<float>(), training ? 1 : 0, ws[0].data_ptr<float>(),
                            ws[1].data_ptr<float>(), nblk, fws.data_ptr<double>(), coef.data_ptr<float>(),
                            dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), dx.data_ptr(), cur_stream());
  return {dx, dgamma, dbeta};
}

// ------------------------------------------------------ GroupNorm / InstanceNorm
// x: [N*HW, C] rows (NHWC), statistics per (sample, group)
std::vector<Tensor> gn_forward(const Tensor& x_, int64_t N, int64_t G, const optional<Tensor>& weight,
                               const optional<Tensor>& bias, double eps, const optional<Tensor>& residual,
                               int64_t act, double slope) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = as_rows(x_);
  const int C = (int)x.size(1);
  TORCH_CHECK(N > 0 && x.size(0) % N == 0, "gn_forward: rows not divisible by N");
  TORCH_CHECK(G > 0 && C % G == 0, "gn_forward: C % G != 0");
  const int64_t HW = x.size(0) / N;
  auto fopt = x.options().dtype(at::kFloat);
  Tensor wf = f32_or_undef(weight), bf = f32_or_undef(bias);
  Tensor coeff = at::empty({4, N, C}, fopt);  // mean, invstd, scale, shift (per n, c)
  const int nblk = tbamd::norm_partial_blocks(HW, C, (int)N);
  Tensor ws = at::empty({2, N, (int64_t)nblk, C}, fopt);
  Tensor row0 = at::empty({N, C}, fopt);
  auto st = cur_stream();
  tbamd::gn_forward_stats(dt_code(x), x.data_ptr(), (int)N, HW, C, (int)G, f32_or_null(wf), f32_or_null(bf),
                          (float)eps, ws[0].data_ptr<float>(),
                          ws[1].data_ptr<float>(), row0.data_ptr<float>(), nblk, coeff[0].data_ptr<float>(),
                          coeff[1].data_ptr<float>(), coeff[2].data_ptr<float>(), coeff[3].data_ptr<float>(), st);
  Tensor res = rows_or_undef(residual);
  Tensor y = at::empty_like(x);
  tbamd::norm_apply(dt_code(x), x.data_ptr(), ptr_or_null(res), coeff[2].data_ptr<float>(),
                    coeff[3].data_ptr<float>(), (int)N, HW, C, (int)act, (float)slope, y.data_ptr(), st);
  return {y, coeff};
}

std::vector<Tensor> gn_backward(const Tensor& dy_, const Tensor& y_, const Tensor& x_, const optional<Tensor>& residual,
                                const optional<Tensor>& weight, const Tensor& coeff, int64_t N, int64_t G, int64_t act,
                                double slope, bool need_dres, const optional<Tensor>& dgamma_out,
                                const optional<Tensor>& dbeta_out) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor x = as_rows(x_);
  Tensor dy = as_rows(dy_.to(x.scalar_type()));
  Tensor y = as_rows(y_);
  const int C = (int)x.size(1);
  const int64_t HW = x.size(0) / N;
  auto fopt = x.options().dtype(at::kFloat);
  Tensor res = rows_or_undef(residual);
  Tensor wf = f32_or_undef(weight);
  const int nblk = tbamd::norm_partial_blocks(HW, C, (int)N);
  Tensor ws = at::empty({2, N, (int64_t)nblk, C}, fopt);
  Tensor coef = at::empty({N, 3, C}, fopt);
  Tensor nc = at::empty({2, N, C}, fopt);
  Tensor dgamma = slot_or_new(dgamma_out, C, fopt, "gn_backward"), dbeta = slot_or_new(dbeta_out, C, fopt, "gn_backward");
  Tensor dx = at::empty_like(x);
  Tensor dres;
  if (need_dres) dres = at::empty_like(x);
  tbamd::gn_backward(dt_code(x), dy.data_ptr(), y.data_ptr(), x.data_ptr(), ptr_or_null(res),
                     (int)N, HW, C, (int)G, (int)act, (float)slope, f32_or_null(wf),
                     coeff[0].data_ptr<float>(), coeff[1].data_ptr<float>(), coeff[2].data_ptr<float>(),
                     coeff[3].data_ptr<float>(), ws[0].data_ptr<float>(), ws[1].data_ptr<float>(), nblk,
                     coef.data_ptr<float>(), nc[0].data_ptr<float>(), nc[1].data_ptr<float>(),
                     dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), need_dres ? dres.data_ptr() : nullptr,
                     dx.data_ptr(), cur_stream());
  return {dx, dgamma, dbeta, dres};
}

// --------------------------------------------------------------- LayerNorm
// returns {y, xsum (x + residual, or undefined), mean, rstd}
std::vector<Tensor> ln_forward(const Tensor& x_, const optional<Tensor>& residual, const optional<Tensor>& weight,
                               const optional<Tensor>& bias, double eps) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = as_rows(x_);
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0 && C <= 4096, "ln_forward: C % 8 == 0 and C <= 4096");
  Tensor res, xsum;
  if (given(residual)) {
    res = as_rows(residual->to(x.scalar_type()));
    xsum = at::empty_like(x);
  }
  Tensor wf = f32_or_undef(weight), bf = f32_or_undef(bias);
  auto fopt = x.options().dtype(at::kFloat);
  Tensor mean = at::empty({M}, fopt), rstd = at::empty({M}, fopt);
  Tensor y = at::empty_like(x);
  if (M > 0)
    tbamd::ln_forward(dt_code(x), x.data_ptr(), ptr_or_null(res), f32_or_null(wf), f32_or_null(bf), M,
                      C, (float)eps, y.data_ptr(), ptr_or_null(xsum), mean.data_ptr<float>(),
                      rstd.data_ptr<float>(), cur_stream());
  return {y, xsum, mean, rstd};
}

// dadd (optional, same shape as x): added to dx in the kernel (residual-stream gradient)
std::vector<Tensor> ln_backward(const Tensor& dy_, const Tensor& x_, const optional<Tensor>& weight,
                                const Tensor& mean, const Tensor& rstd, const optional<Tensor>& dadd_,
                                const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor x = as_rows(x_);
  Tensor dy = as_rows(dy_.to(x.scalar_type()));
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  Tensor wf = f32_or_undef(weight);
  auto fopt = x.options().dtype(at::kFloat);
  const int nblk = tbamd::ln_bwd_blocks(M);
  Tensor ws = at::empty({2, (int64_t)nblk, C}, fopt);
  Tensor dg = slot_or_new(dgamma_out, C, fopt, "ln_backward"), db = slot_or_new(dbeta_out, C, fopt, "ln_backward");
  Tensor dx = at::empty_like(x);
  Tensor dadd;
  if (given(dadd_)) {
    dadd = as_rows(dadd_->to(x.scalar_type()));
    TORCH_CHECK(dadd.size(0) == M && dadd.size(1) == C, "ln_backward: dadd shape");
  }
  if (M > 0)
    tbamd::ln_backward(dt_code(x), dy.data_ptr(), x.data_ptr(), ptr_or_null(dadd), f32_or_null(wf),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), M, C, dx.data_ptr(), ws[0].data_ptr<float>(),
                       ws[1].data_ptr<float>(), nblk, dg.data_ptr<float>(), db.data_ptr<float>(), cur_stream());
  else {
    dg.zero_();
    db.zero_();
  }
  return {dx, dg, db};
}

// --------------------------------------------------------------- RMSNorm (csrc/layernorm.hip, RMS = true)
// returns {y, xsum (x + residual, or undefined), rstd}
std::vector<Tensor> rms_forward(const Tensor& x_, const optional<Tensor>& residual, const optional<Tensor>& weight,
                                double eps) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = as_rows(x_);
  TORCH_CHECK(x.dim() == 2, "rms_forward: x must be [M, C]");
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= 4096, "rms_forward: C % 8 == 0 and C <= 4096");
  Tensor res, xsum;
  if (given(residual)) {
    res = as_rows(residual->to(x.scalar_type()));
    TORCH_CHECK(res.dim() == 2 && res.size(0) == M && res.size(1) == C, "rms_forward: residual shape");
    xsum = at::empty_like(x);
  }
  Tensor wf = f32_or_undef(weight);
  TORCH_CHECK(!wf.defined() || wf.numel() == C, "rms_forward: weight must be [C]");
  Tensor rstd = at::empty({M}, x.options().dtype(at::kFloat));
  Tensor y = at::empty_like(x);
  if (M > 0)
    tbamd::rms_forward(dt_code(x), x.data_ptr(), ptr_or_null(res), f32_or_null(wf), M, C, (float)eps, y.data_ptr(),
                       ptr_or_null(xsum), rstd.data_ptr<float>(), cur_stream());
  return {y, xsum, rstd};
}

// dadd (optional, same shape as x): added to dx in the kernel (residual-stream gradient)
std::vector<Tensor> rms_backward(const Tensor& dy_, const Tensor& x_, const optional<Tensor>& weight,
                                 const Tensor& rstd, const optional<Tensor>& dadd_,
                                 const optional<Tensor>& dgamma_out) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor x = as_rows(x_);
  Tensor dy = as_rows(dy_.to(x.scalar_type()));
  TORCH_CHECK(x.dim() == 2 && dy.sizes() == x.sizes(), "rms_backward: dy must match x [M, C]");
  const int64_t M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= 4096, "rms_backward: C % 8 == 0 and C <= 4096");
  check_cuda(rstd, "rstd");
  TORCH_CHECK(rstd.scalar_type() == at::kFloat && rstd.numel() == M && rstd.is_contiguous(),
              "rms_backward: rstd must be contiguous f32 [M]");
  Tensor wf = f32_or_undef(weight);
  TORCH_CHECK(!wf.defined() || wf.numel() == C, "rms_backward: weight must be [C]");
  auto fopt = x.options().dtype(at::kFloat);
  const int nblk = tbamd::ln_bwd_blocks(M);
  Tensor ws = at::empty({(int64_t)nblk, C}, fopt);
  Tensor dg = slot_or_new(dgamma_out, C, fopt, "rms_backward");
  Tensor dx = at::empty_like(x);
  Tensor dadd;
  if (given(dadd_)) {
    dadd = as_rows(dadd_->to(x.scalar_type()));
    TORCH_CHECK(dadd.dim() == 2 && dadd.size(0) == M && dadd.size(1) == C, "rms_backward: dadd shape");
  }
  if (M > 0)
    tbamd::rms_backward(dt_code(x), dy.data_ptr(), x.data_ptr(), ptr_or_null(dadd), f32_or_null(wf),
                        rstd.data_ptr<float>(), M, C, dx.data_ptr(), ws.data_ptr<float>(), nblk,
                        dg.data_ptr<float>(), cur_stream());
  else
    dg.zero_();
  return {dx, dg};
}

// ---------------------------------------------------------------- global average pool (K7)
// x [N, C, H, W] channels_last (C % 8 == 0) -> [N, C]
Tensor global_avgpool(const Tensor& x_) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = nhwc(x_);
  const int N = (int)x.size(0), C = (int)x.size(1), HW = (int)(x.size(2) * x.size(3));
  TORCH_CHECK(C % 8 == 0, "global_avgpool: C % 8 == 0");
  Tensor y = at::empty({N, C}, x.options());
  tbamd::global_avgpool_fwd(dt_code(x), x.data_ptr(), N, HW, C, y.data_ptr(), cur_stream());
  return y;
}

// dy [N, C] -> dx [N, C, H, W] channels_last = dy / (H W) broadcast
Tensor global_avgpool_backward(const Tensor& dy_, int64_t H, int64_t W) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor dy = dy_.contiguous();
  const int N = (int)dy.size(0), C = (int)dy.size(1);
  TORCH_CHECK(C % 8 == 0, "global_avgpool_backward: C % 8 == 0");
  Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  tbamd::global_avgpool_bwd(dt_code(dy), dy.data_ptr(), N, (int)(H * W), C, dx.data_ptr(), cur_stream());
  return dx;
}

}  // namespace

void register_norm(pybind11::module& m) {
  m.def("bn_forward", &bn_forward, py::arg("x"), py::arg("weight"), py::arg("bias"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("training"), py::arg("momentum"), py::arg("eps"), py::arg("residual"),
        py::arg("act"), py::arg("slope"), py::arg("num_batches_tracked") = py::none(),
        py::arg("want_mask") = false);
  m.def("bn_backward", &bn_backward, py::arg("dy"), py::arg("y"), py::arg("x"), py::arg("residual"),
        py::arg("weight"), py::arg("mean"), py::arg("invstd"), py::arg("scale"), py::arg("shift"),
        py::arg("training"), py::arg("act"), py::arg("slope"), py::arg("need_dres"),
        py::arg("dgamma_out") = py::none(), py::arg("dbeta_out") = py::none(), py::arg("mask") = py::none());
  m.def("bn_backward_from_partials", &bn_backward_from_partials, py::arg("dy"), py::arg("x"), py::arg("part"),
        py::arg("weight"), py::arg("mean"), py::arg("invstd"), py::arg("scale"), py::arg("shift"),
        py::arg("training"), py::arg("act"), py::arg("slope"), py::arg("dgamma_out") = py::none(),
        py::arg("dbeta_out") = py::none(), py::arg("mask") = py::none(), py::arg("want_dres") = false,
        py::arg("ds_x") = py::none(), py::arg("ds_mean") = py::none());
  m.def("bn_backward_coef", &bn_backward_coef, py::arg("part"), py::arg("weight"), py::arg("mean"),
        py::arg("invstd"), py::arg("M"), py::arg("training"), py::arg("dgamma_out") = py::none(),
        py::arg("dbeta_out") = py::none());
  m.def("bn_backward_apply_coef", &bn_backward_apply_coef, py::arg("dy"), py::arg("x"), py::arg("coef"),
        py::arg("scale"), py::arg("shift"), py::arg("act"), py::arg("slope"), py::arg("mask") = py::none());
  m.def("bn_apply_coeff", &bn_apply_coeff, py::arg("x"), py::arg("coeff"), py::arg("residual") = py::none(),
        py::arg("act") = 1, py::arg("slope") = 0.01, py::arg("want_mask") = false);
  m.def("bn_forward_from_stats", &bn_forward_from_stats, py::arg("x"), py::arg("stats"), py::arg("weight"),
        py::arg("bias"), py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        py::arg("residual"), py::arg("act"), py::arg("slope"), py::arg("num_batches_tracked") = py::none(),
        py::arg("want_mask") = false, py::arg("res_scale") = py::none(), py::arg("res_shift") = py::none());
  m.def("bn_stats", &bn_stats);
  m.def(
      "norm_partial_blocks",
      [](int64_t M, int64_t C, int64_t S) {
        TORCH_CHECK(M > 0 && C > 0 && S > 0, "norm_partial_blocks: M, C, S > 0");
        return (int64_t)tbamd::norm_partial_blocks(M, (int)C, (int)S);
      },
      py::arg("M"), py::arg("C"), py::arg("S") = 1,
      "Read-only: the number of partial-sum rows (row blocks, gridDim.x) the statistics and backward "
      "reduction passes write for M rows of C channels per sample and S samples (S = 1: BatchNorm; "
      "S = N: GroupNorm / InstanceNorm).  More than 32 rows puts the BatchNorm column-sum finalize "
      "on its multi-slice ticket path.");
  m.def("bn_act_maxpool", &bn_act_maxpool);
  m.def("maxpool_backward", &maxpool_backward);
  m.def("bn_backward_pool", &bn_backward_pool, py::arg("dy"), py::arg("idx"), py::arg("x"), py::arg("N"),
        py::arg("H"), py::arg("W"), py::arg("k"), py::arg("s"), py::arg("pad"), py::arg("weight"), py::arg("mean"),
        py::arg("invstd"), py::arg("scale"), py::arg("shift"), py::arg("training"), py::arg("act"),
        py::arg("slope"), py::arg("dgamma_out") = py::none(), py::arg("dbeta_out") = py::none());
  m.def("bn_backward_pool_ok", &tbamd::bn_backward_pool_ok);
  m.def("gn_forward", &gn_forward);
  m.def("gn_backward", &gn_backward, py::arg("dy"), py::arg("y"), py::arg("x"), py::arg("residual"),
        py::arg("weight"), py::arg("coeff"), py::arg("N"), py::arg("G"), py::arg("act"), py::arg("slope"),
        py::arg("need_dres"), py::arg("dgamma_out") = py::none(), py::arg("dbeta_out") = py::none());
  m.def("ln_forward", &ln_forward);
  m.def("ln_backward", &ln_backward, py::arg("dy"), py::arg("x"), py::arg("weight"), py::arg("mean"),
        py::arg("rstd"), py::arg("dadd") = py::none(), py::arg("dgamma_out") = py::none(),
        py::arg("dbeta_out") = py::none());
  m.def("rms_forward", &rms_forward, py::arg("x"), py::arg("residual"), py::arg("weight"), py::arg("eps"));
  m.def("rms_backward", &rms_backward, py::arg("dy"), py::arg("x"), py::arg("weight"), py::arg("rstd"),
        py::arg("dadd") = py::none(), py::arg("dgamma_out") = py::none());
  m.def("global_avgpool", &global_avgpool);
  m.def("global_avgpool_backward", &global_avgpool_backward);
}
