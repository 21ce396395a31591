// Bindings of the 64-channel implicit-GEMM convolutions (conv.hip, conv_big.hip, conv_wgrad.hip,
// conv_tinyin_wgrad.hip, im2col.hip): the ResNet stem, forward / input gradient / weight gradient
// with their fused BN epilogues and prologues, the virtual-input and split-bf16 fp32 forms.
// x: [N, C, H, W] logical, channels_last memory; w: [K, C, R, S] logical, channels_last memory
// ([K][R][S][C]); outputs [N, K, P, Q] channels_last.
#include "bind_common.h"

namespace {
using namespace tbbind;

const auto kNHWC = at::MemoryFormat::ChannelsLast;

// n floats of kernel workspace on like's device, or an undefined tensor when the kernel needs none
Tensor f32_work(int64_t n, const Tensor& like) {
  return n > 0 ? at::empty({n}, like.options().dtype(at::kFloat)) : Tensor();
}

// ---------------------------------------------------------------- ResNet stem
// ResNet stem on the native kernels (see tbamd.h): pad -> xp, forward from xp + packed
// weights wp [K, 256] -> {y [N, K, P, Q] channels_last, stats [tiles, 2, K] or undefined},
// weight gradient from dy + xp -> packed [K, 256]
Tensor conv2d_stem_pad(const Tensor& x_) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.scalar_type() == at::kBFloat16 && x_.dim() == 4 && x_.size(1) == 3, "conv2d_stem_pad: bf16 [N,3,H,W]");
  Tensor x = nhwc(x_);
  const int N = (int)x.size(0), H = (int)x.size(2), W = (int)x.size(3);
  int P, Q, Hp, Wp;
  tbamd::stem_geometry(H, W, &P, &Q, &Hp, &Wp);
  Tensor xp = at::empty({N, Hp, Wp, 4}, x.options());
  if (N > 0) tbamd::conv_stem_pad(x.data_ptr(), xp.data_ptr(), N, H, W, cur_stream());
  return xp;
}

std::vector<Tensor> conv2d_stem_fwd(const Tensor& xp, const Tensor& wp_, int64_t H, int64_t W, bool want_stats) {
  const at::DeviceGuard guard = on_device_of(xp, "xp");
  int P, Q, Hp, Wp;
  tbamd::stem_geometry((int)H, (int)W, &P, &Q, &Hp, &Wp);
  TORCH_CHECK(xp.scalar_type() == at::kBFloat16 && xp.dim() == 4 && xp.size(1) == Hp && xp.size(2) == Wp &&
                  xp.size(3) == 4 && xp.is_contiguous(), "conv2d_stem_fwd: xp from conv2d_stem_pad");
  TORCH_CHECK(wp_.scalar_type() == at::kBFloat16 && wp_.dim() == 2 && wp_.size(1) == 256 && wp_.size(0) % 64 == 0,
              "conv2d_stem_fwd: wp [K % 64 == 0, 256] bf16");
  Tensor wp = wp_.contiguous();
  const int N = (int)xp.size(0), K = (int)wp.size(0);
  Tensor y = at::empty({N, K, P, Q}, xp.options().memory_format(kNHWC));
  const int64_t NPQ = (int64_t)N * P * Q;
  Tensor stats;
  if (want_stats) stats = at::empty({tbamd::conv_fwd_pixel_tiles(NPQ, K), 2, K}, xp.options().dtype(at::kFloat));
  if (NPQ > 0)
    tbamd::conv_stem_fwd(xp.data_ptr(), wp.data_ptr(), y.data_ptr(), want_stats ? stats.data_ptr<float>() : nullptr,
                         N, (int)H, (int)W, K, cur_stream());
  return {y, stats};
}

Tensor conv2d_stem_wgrad(const Tensor& dy_, const Tensor& xp, int64_t H, int64_t W) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  int P, Q, Hp, Wp;
  tbamd::stem_geometry((int)H, (int)W, &P, &Q, &Hp, &Wp);
  TORCH_CHECK(xp.dim() == 4 && xp.size(1) == Hp && xp.size(2) == Wp && xp.size(3) == 4 && xp.is_contiguous(),
              "conv2d_stem_wgrad: xp from conv2d_stem_pad");
  Tensor dy = nhwc(dy_);
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && dy.size(0) == xp.size(0) && dy.size(2) == P && dy.size(3) == Q &&
                  dy.size(1) % 64 == 0, "conv2d_stem_wgrad: dy [N, K % 64, P, Q] bf16");
  const int N = (int)dy.size(0), K = (int)dy.size(1);
  Tensor dwp = at::empty({K, 256}, dy.options());
  Tensor work = f32_work(tbamd::conv_stem_wgrad_workspace(N, Hp, Wp, K, P, Q), dy);
  if ((int64_t)N * P * Q == 0) return dwp.zero_();
  tbamd::conv_stem_wgrad(dy.data_ptr(), xp.data_ptr(), dwp.data_ptr(), f32_or_null(work), N, Hp, Wp, K, P, Q,
                         cur_stream());
  return dwp;
}

// ---------------------------------------------------------------- forward and input gradient
// BN-backward partial sums fused into an input-gradient epilogue (bnb_mode 1-3): the operands of the
// BN whose output gradient the conv produces, as [pixels, ch] rows
struct Bnb {
  const void* x = nullptr;
  const float *scale = nullptr, *shift = nullptr, *mean = nullptr;
  const uint8_t* bits = nullptr;
};

Bnb bnb_operands(int64_t mode, const optional<Tensor>& x, const optional<Tensor>& scale, const optional<Tensor>& shift,
                 const optional<Tensor>& mean, const optional<Tensor>& bits, int64_t pixels, int ch, const char* op) {
  Bnb b;
  TORCH_CHECK(x.has_value() && x->numel() == pixels * ch && x->scalar_type() == at::kBFloat16 && mean.has_value() &&
                  mean->numel() == ch,
              op, ": bnb_x [pixels, channels] bf16 and bnb_mean [channels] required");
  b.x = x->data_ptr();
  b.mean = mean->data_ptr<float>();
  if (mode == 1) {
    TORCH_CHECK(scale.has_value() && shift.has_value(), op, ": bnb scale/shift");
    b.scale = scale->data_ptr<float>();
    b.shift = shift->data_ptr<float>();
  }
  if (mode == 2) {
    TORCH_CHECK(bits.has_value() && bits->numel() == pixels * (ch / 8), op, ": bnb_bits");
    b.bits = bits->data_ptr<uint8_t>();
  }
  return b;
}

// input gradient of a stride-2 conv: dy [N, Kf, P, Q], wt = conv_flip_weight(w) [Cf, R, S, Kf]
// (channels_last bf16) -> dx [N, Cf, H, W] channels_last (4 parity-class launches)
std::vector<Tensor> conv2d_dgrad_s2(const Tensor& dy_, const Tensor& wt_, int64_t R, int64_t S, int64_t pad,
                                    int64_t H, int64_t W, int64_t bnb_mode, const optional<Tensor>& bnb_x,
                                    const optional<Tensor>& bnb_scale, const optional<Tensor>& bnb_shift,
                                    const optional<Tensor>& bnb_mean, const optional<Tensor>& bnb_bits,
                                    int64_t stride) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  TORCH_CHECK(dy_.scalar_type() == at::kBFloat16 && wt_.scalar_type() == at::kBFloat16, "conv2d_dgrad_s2: bf16 only");
  const int cs = (int)stride;
  Tensor dy = nhwc(dy_);
  Tensor wt = nhwc(wt_);
  const int N = (int)dy.size(0), Kf = (int)dy.size(1), P = (int)dy.size(2), Q = (int)dy.size(3);
  const int Cf = (int)wt.size(0);
  TORCH_CHECK(wt.dim() == 4 && wt.size(1) == Kf && wt.size(2) == R && wt.size(3) == S,
              "conv2d_dgrad_s2: wt must be the flip-transposed [Cf, Kf, R, S] weight");
  TORCH_CHECK(tbamd::conv_fwd_supported(Kf, Cf) && tbamd::conv_dgrad_s2_supported((int)R, (int)S, cs),
              "conv2d_dgrad_s2: channels % 64, stride 2 or 3, <= 16 taps per phase class");
  TORCH_CHECK(pad >= 0 && P == (H + 2 * pad - R) / cs + 1 && Q == (W + 2 * pad - S) / cs + 1,
              "conv2d_dgrad_s2: geometry");
  Tensor dx = at::empty({N, Cf, H, W}, dy.options().memory_format(kNHWC));
  const int64_t NHW = (int64_t)N * H * W;
  Tensor part;
  Bnb bnb;
  if (bnb_mode != 0) {
    TORCH_CHECK(bnb_mode >= 1 && bnb_mode <= 3, "conv2d_dgrad_s2: bnb_mode");
    bnb = bnb_operands(bnb_mode, bnb_x, bnb_scale, bnb_shift, bnb_mean, bnb_bits, NHW, Cf, "conv2d_dgrad_s2");
    part = at::empty({tbamd::conv_dgrad_s2_tiles(N, (int)H, (int)W, Cf, cs), 2, Cf}, dy.options().dtype(at::kFloat));
  }
  if (NHW > 0)
    tbamd::conv_dgrad_s2(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), N, P, Q, Kf, Cf, (int)R, (int)S, (int)pad,
                         (int)H, (int)W, cur_stream(), (int)bnb_mode, bnb.x, bnb.scale, bnb.shift, bnb.mean, bnb.bits,
                         f32_or_null(part), cs);
  return {dx, part};
}

// Returns y [N, K, P, Q] channels_last and, if want_stats, per-pixel-tile (sum, sumsq) partials
// [ntiles, 2, K] (with bnb_mode: the BN-backward partials instead).
std::vector<Tensor> conv2d_fwd(const Tensor& x_, const Tensor& w_, const optional<Tensor>& bias, int64_t stride,
                               int64_t pad, bool relu, bool want_stats, const optional<Tensor>& addend,
                               const optional<Tensor>& addend_mask, int64_t bnb_mode, const optional<Tensor>& bnb_x,
                               const optional<Tensor>& bnb_scale, const optional<Tensor>& bnb_shift,
                               const optional<Tensor>& bnb_mean, const optional<Tensor>& bnb_bits, int64_t big) {
  check_cuda(x_, "x");
  // big >= 0: this call's big-tile choice (0 = the 128x128 kernels), restored on every exit
  struct BigScope {
    explicit BigScope(int64_t c) { if (c >= 0) tbamd::conv_big_set_call((int)c); }
    ~BigScope() { tbamd::conv_big_set_call(-1); }
  } big_scope(big);
  const at::DeviceGuard guard(x_.device());
  TORCH_CHECK(x_.scalar_type() == at::kBFloat16 && w_.scalar_type() == at::kBFloat16, "conv2d_fwd: bf16 only");
  TORCH_CHECK(x_.dim() == 4 && w_.dim() == 4 && x_.size(1) == w_.size(1), "conv2d_fwd: shape");
  Tensor x = nhwc(x_);
  Tensor w = nhwc(w_);
  ConvGeom g = ConvGeom::of(x, w);
  TORCH_CHECK(tbamd::conv_fwd_supported(g.C, g.K), "conv2d_fwd: needs C % 64 == 0 and K % 64 == 0");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, 1, false, 0, "conv2d_fwd");
  Tensor y = at::empty({N, K, P, Q}, x.options().memory_format(kNHWC));
  Tensor bf = f32_or_undef(bias);
  Tensor stats;
  const int64_t NPQ = g.NPQ();
  if (want_stats)
    stats = at::empty({tbamd::conv_fwd_stats_rows(NPQ, C, K, R, S, (int)stride, (int)pad), 2, K},
                      x.options().dtype(at::kFloat));
  Tensor add;
  if (given(addend)) {
    TORCH_CHECK(!want_stats && !bf.defined() && !relu, "conv2d_fwd: addend excludes bias / relu / stats");
    TORCH_CHECK(addend->sizes() == y.sizes() && addend->scalar_type() == at::kBFloat16, "conv2d_fwd: addend shape");
    add = nhwc(*addend);
  }
  const uint8_t* amask = nullptr;
  if (given(addend_mask)) {
    TORCH_CHECK(add.defined() && addend_mask->scalar_type() == at::kByte && addend_mask->numel() == NPQ * (K / 8),
                "conv2d_fwd: addend_mask must be [N*P*Q, K/8] bytes");
    amask = addend_mask->data_ptr<uint8_t>();
  }
  // BN-backward partial sums of the BN whose output gradient y is (dgrad use)
  Tensor part;
  Bnb bnb;
  if (bnb_mode != 0) {
    TORCH_CHECK(bnb_mode >= 1 && bnb_mode <= 3 && !want_stats && !bf.defined() && !relu, "conv2d_fwd: bnb_mode");
    bnb = bnb_operands(bnb_mode, bnb_x, bnb_scale, bnb_shift, bnb_mean, bnb_bits, NPQ, K, "conv2d_fwd");
    part = at::empty({tbamd::conv_fwd_bnb_rows(NPQ, C, K, R, S, (int)stride, (int)pad), 2, K},
                     x.options().dtype(at::kFloat));
  }
  if (NPQ > 0)
    tbamd::conv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), f32_or_null(bf),
                    want_stats ? stats.data_ptr<float>() : nullptr, ptr_or_null(add), amask, relu, N,
                    H, W, C, K, R, S, P, Q, (int)stride, (int)pad, cur_stream(), (int)bnb_mode, bnb.x, bnb.scale,
                    bnb.shift, bnb.mean, bnb.bits, f32_or_null(part));
  return {y, bnb_mode != 0 ? part : stats};
}

// 1x1 stride-1 input gradient whose operand is a deferred BN backward apply (conv.hip GxfArgs):
// g = the BN output gradient [N, C, H, W] (C = the conv's output channels), wt the flipped /
// transposed weight [K, C, 1, 1] (K = the conv's input channels), gx_x the BN input (the conv's
// forward output, g's shape), gx_coef [3, C] from bn_backward_coef, gxf 1 (ReLU mask recomputed
// from gx_scale / gx_shift) or 2 (gx_bits [N*H*W, C/8]).  Returns [dx, bnb partials (or empty),
// dz (the materialised BN input gradient when want_dz, else empty)].
std::vector<Tensor> conv2d_dgrad_gxf(const Tensor& g_, const Tensor& wt_, const optional<Tensor>& addend,
                                     const optional<Tensor>& addend_mask, int64_t bnb_mode,
                                     const optional<Tensor>& bnb_x, const optional<Tensor>& bnb_scale,
                                     const optional<Tensor>& bnb_shift, const optional<Tensor>& bnb_mean,
                                     const optional<Tensor>& bnb_bits, int64_t gxf, const Tensor& gx_x_,
                                     const optional<Tensor>& gx_bits, const optional<Tensor>& gx_scale,
                                     const optional<Tensor>& gx_shift, const Tensor& gx_coef, bool want_dz) {
  const at::DeviceGuard guard = on_device_of(g_, "g");
  TORCH_CHECK(g_.scalar_type() == at::kBFloat16 && wt_.scalar_type() == at::kBFloat16 &&
                  gx_x_.scalar_type() == at::kBFloat16, "conv2d_dgrad_gxf: bf16 only");
  TORCH_CHECK(g_.dim() == 4 && wt_.dim() == 4 && wt_.size(1) == g_.size(1) && wt_.size(2) == 1 && wt_.size(3) == 1,
              "conv2d_dgrad_gxf: 1x1 weight [K, C, 1, 1] over g [N, C, H, W]");
  TORCH_CHECK(gx_x_.sizes() == g_.sizes(), "conv2d_dgrad_gxf: gx_x must have g's shape");
  Tensor g = nhwc(g_);
  Tensor wt = nhwc(wt_);
  Tensor gx_x = nhwc(gx_x_);
  const int N = (int)g.size(0), C = (int)g.size(1), H = (int)g.size(2), W = (int)g.size(3);
  const int K = (int)wt.size(0);
  const int64_t NPQ = (int64_t)N * H * W;
  TORCH_CHECK(tbamd::conv_fwd_supported(C, K), "conv2d_dgrad_gxf: needs C % 64 == 0 and K % 64 == 0");
  TORCH_CHECK(gx_coef.scalar_type() == at::kFloat && gx_coef.is_contiguous() && gx_coef.numel() == 3 * C,
              "conv2d_dgrad_gxf: gx_coef [3, C] f32");
  const uint8_t* gbits = nullptr;
  const float *gsc = nullptr, *gsf = nullptr;
  if (gxf == 2) {
    TORCH_CHECK(gx_bits.has_value() && gx_bits->scalar_type() == at::kByte && gx_bits->numel() == NPQ * (C / 8),
                "conv2d_dgrad_gxf: gx_bits [N*H*W, C/8] bytes");
    gbits = gx_bits->data_ptr<uint8_t>();
  } else {
    TORCH_CHECK(gxf == 1 && gx_scale.has_value() && gx_shift.has_value() && gx_scale->numel() == C &&
                    gx_shift->numel() == C && gx_scale->scalar_type() == at::kFloat &&
                    gx_shift->scalar_type() == at::kFloat && gx_scale->is_contiguous() && gx_shift->is_contiguous(),
                "conv2d_dgrad_gxf: gxf 1 needs f32 [C] scale / shift");
    gsc = gx_scale->data_ptr<float>();
    gsf = gx_shift->data_ptr<float>();
  }
  Tensor y = at::empty({N, K, H, W}, g.options().memory_format(kNHWC));
  Tensor add;
  const uint8_t* amask = nullptr;
  if (given(addend)) {
    TORCH_CHECK(addend->sizes() == y.sizes() && addend->scalar_type() == at::kBFloat16, "conv2d_dgrad_gxf: addend");
    add = nhwc(*addend);
    if (given(addend_mask)) {
      TORCH_CHECK(addend_mask->scalar_type() == at::kByte && addend_mask->numel() == NPQ * (K / 8),
                  "conv2d_dgrad_gxf: addend_mask [N*H*W, K/8] bytes");
      amask = addend_mask->data_ptr<uint8_t>();
    }
  }
  const int add_code = add.defined() ? (amask ? 2 : 1) : 0;
  TORCH_CHECK(tbamd::conv_dgrad_gxf_supported((int)gxf, add_code, (int)bnb_mode),
              "conv2d_dgrad_gxf: unsupported (gxf, addend, bnb_mode) combination");
  Tensor part;
  Bnb bnb;
  if (bnb_mode != 0) {
    bnb = bnb_operands(bnb_mode, bnb_x, bnb_scale, bnb_shift, bnb_mean, bnb_bits, NPQ, K, "conv2d_dgrad_gxf");
    part = at::empty({tbamd::conv_gxf_bnb_rows(NPQ, K), 2, K}, g.options().dtype(at::kFloat));
  }
  Tensor dz;
  if (want_dz) dz = at::empty_like(g);
  if (NPQ > 0)
    tbamd::conv_dgrad_gxf(g.data_ptr(), wt.data_ptr(), y.data_ptr(), ptr_or_null(add), amask,
                          N, H, W, C, K, cur_stream(), (int)bnb_mode, bnb.x, bnb.scale, bnb.shift, bnb.mean, bnb.bits,
                          f32_or_null(part), (int)gxf, gx_x.data_ptr(), gbits, gsc,
                          gsf, gx_coef.data_ptr<float>(), ptr_or_null(dz));
  return {y, part, dz};
}

bool conv_dgrad_gxf_supported(int64_t gxf, int64_t add, int64_t bnb_mode) {
  return tbamd::conv_dgrad_gxf_supported((int)gxf, (int)add, (int)bnb_mode);
}

// f32 [C] scale / shift of a BN folded into a conv's operand staging (csrc/xf.h)
void check_xf_coeffs(const Tensor& scale, const Tensor& shift, int C, const char* op) {
  TORCH_CHECK(scale.scalar_type() == at::kFloat && shift.scalar_type() == at::kFloat && scale.numel() == C &&
                  shift.numel() == C && scale.is_contiguous() && shift.is_contiguous(),
              op, ": scale / shift [C] f32");
}

// y = conv(relu(x * scale + shift), w) with the BN + ReLU applied in the kernel's operand staging
// (csrc/xf.h): returns [y, stats] (stats: the BN partial rows of y, as conv2d_fwd want_stats)
std::vector<Tensor> conv2d_fwd_xf(const Tensor& x_, const Tensor& w_, const Tensor& scale, const Tensor& shift,
                                  int64_t stride, int64_t pad, bool want_stats) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.scalar_type() == at::kBFloat16 && w_.scalar_type() == at::kBFloat16, "conv2d_fwd_xf: bf16 only");
  Tensor x = nhwc(x_);
  Tensor w = nhwc(w_);
  ConvGeom g = ConvGeom::of(x, w);
  TORCH_CHECK(w.size(1) == g.C && tbamd::conv_fwd_supported(g.C, g.K), "conv2d_fwd_xf: needs C % 64 == 0 and K % 64 == 0");
  TORCH_CHECK(g.C <= tbamd::kXfMaxC, "conv2d_fwd_xf: at most ", tbamd::kXfMaxC, " input channels (coefficients in LDS)");
  check_xf_coeffs(scale, shift, g.C, "conv2d_fwd_xf");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, 1, false, 0, "conv2d_fwd_xf");
  const int64_t NPQ = g.NPQ();
  TORCH_CHECK(tbamd::conv_fwd_xf_supported(NPQ, C, K, R, S, (int)stride, (int)pad),
              "conv2d_fwd_xf: the persistent 1x1 shapes only (C = 64 / 128, 1x1 stride 1, K % 128, enough pixels)");
  Tensor y = at::empty({N, K, P, Q}, x.options().memory_format(kNHWC));
  Tensor stats;
  if (want_stats)
    stats = at::empty({tbamd::conv_fwd_stats_rows_tiled(NPQ, C, K, R, S, (int)stride, (int)pad), 2, K},
                      x.options().dtype(at::kFloat));
  if (NPQ > 0)
    tbamd::conv_fwd_xf(x.data_ptr(), w.data_ptr(), y.data_ptr(), want_stats ? stats.data_ptr<float>() : nullptr,
                       scale.data_ptr<float>(), shift.data_ptr<float>(), N, H, W, C, K, R, S, P, Q, (int)stride,
                       (int)pad, cur_stream());
  return {y, stats};
}

// w [K, C, R, S] (channels_last) -> flipped transpose [C, K, R, S] (channels_last)
Tensor conv_flip_weight(const Tensor& w_) {
  const at::DeviceGuard guard(w_.device());
  Tensor w = nhwc(w_);
  const int K = (int)w.size(0), C = (int)w.size(1), R = (int)w.size(2), S = (int)w.size(3);
  Tensor wt = at::empty({C, K, R, S}, w.options().memory_format(kNHWC));
  tbamd::conv_flip_transpose_weight(w.data_ptr(), K, R, S, C, wt.data_ptr(), cur_stream());
  return wt;
}

// ---------------------------------------------------------------- weight gradient
// the caller's channels_last bf16 [K, C, R, S] slot (e.g. a zero-copy gradient slot) or a new tensor
Tensor dw_slot_or_new(const optional<Tensor>& out, const ConvGeom& g, const Tensor& x, const char* op) {
  if (!given(out)) return at::empty({g.K, g.C, g.R, g.S}, x.options().memory_format(kNHWC));
  TORCH_CHECK(out->dim() == 4 && out->size(0) == g.K && out->size(1) == g.C && out->size(2) == g.R &&
                  out->size(3) == g.S && out->scalar_type() == at::kBFloat16 && out->is_contiguous(kNHWC),
              op, ": out must be a channels_last bf16 [K, C, R, S] tensor");
  return *out;
}

// dW [K, C, R, S] (channels_last) of y = conv(x, w): dy [N, K, P, Q] and x
// [N, C, H, W] channels_last bf16
Tensor conv2d_wgrad(const Tensor& dy_, const Tensor& x_, int64_t R_, int64_t S_, int64_t stride, int64_t pad,
                    const optional<Tensor>& out) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.scalar_type() == at::kBFloat16 && dy_.scalar_type() == at::kBFloat16, "conv2d_wgrad: bf16 only");
  Tensor x = nhwc(x_);
  Tensor dy = nhwc(dy_);
  ConvGeom g = ConvGeom::of(x, dy, R_, S_);
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, 1, false, 0, "conv2d_wgrad");
  TORCH_CHECK(g.fits(dy), "conv2d_wgrad: dy shape does not match x / kernel / stride / pad");
  const int64_t NPQ = g.NPQ();
  TORCH_CHECK(tbamd::conv_wgrad_supported(C, K, NPQ), "conv2d_wgrad: needs C % 64 == 0 and K % 64 == 0");
  Tensor dw = dw_slot_or_new(out, g, x, "conv2d_wgrad");
  if (NPQ == 0) return dw.zero_();
  Tensor work = f32_work(tbamd::conv_wgrad_workspace(N, H, W, C, K, R, S, P, Q, (int)stride, (int)pad), x);
  tbamd::conv_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), f32_or_null(work), N, H, W, C, K, R, S, P, Q,
                    (int)stride, (int)pad, cur_stream());
  return dw;
}

// dW of conv(relu(x * scale + shift), w) (the transform in the X staging); out: optional slot
Tensor conv2d_wgrad_xf(const Tensor& dy_, const Tensor& x_, const Tensor& scale, const Tensor& shift, int64_t R_,
                       int64_t S_, int64_t stride, int64_t pad, const optional<Tensor>& out) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.scalar_type() == at::kBFloat16 && dy_.scalar_type() == at::kBFloat16, "conv2d_wgrad_xf: bf16 only");
  Tensor x = nhwc(x_);
  Tensor dy = nhwc(dy_);
  ConvGeom g = ConvGeom::of(x, dy, R_, S_);
  TORCH_CHECK(tbamd::conv_wgrad_supported(g.C, g.K, (int64_t)g.N * dy.size(2) * dy.size(3)), "conv2d_wgrad_xf: shape");
  check_xf_coeffs(scale, shift, g.C, "conv2d_wgrad_xf");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, 1, false, 0, "conv2d_wgrad_xf");
  TORCH_CHECK(dy.size(2) == P && dy.size(3) == Q, "conv2d_wgrad_xf: dy shape");
  Tensor dw = dw_slot_or_new(out, g, x, "conv2d_wgrad_xf");
  Tensor work = f32_work(tbamd::conv_wgrad_workspace(N, H, W, C, K, R, S, P, Q, (int)stride, (int)pad), x);
  tbamd::conv_wgrad_xf(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), f32_or_null(work), scale.data_ptr<float>(),
                       shift.data_ptr<float>(), N, H, W, C, K, R, S, P, Q, (int)stride, (int)pad, cur_stream());
  return dw;
}

// dW [K = 64, C = 3, 4, 4] (channels_last) of a 4x4 / 2 / pad-1 conv: T = its 3-channel input
// [N, 3, H, W], G = the gradient of its 64-channel output [N, 64, H/2, W/2] (both NHWC bf16).  The
// 64 -> 3 transposed conv's weight gradient is the same call with T = dY and G = its input.
Tensor conv2d_wgrad_tinyin(const Tensor& T_, const Tensor& G_) {
  check_cuda(T_, "T");
  check_cuda(G_, "G");
  const at::DeviceGuard guard(T_.device());
  TORCH_CHECK(T_.scalar_type() == at::kBFloat16 && G_.scalar_type() == at::kBFloat16, "conv2d_wgrad_tinyin: bf16");
  TORCH_CHECK(T_.dim() == 4 && G_.dim() == 4 && T_.size(0) == G_.size(0), "conv2d_wgrad_tinyin: NCHW shapes");
  Tensor T = nhwc(T_), G = nhwc(G_);
  const int N = (int)T.size(0), C = (int)T.size(1), H = (int)T.size(2), W = (int)T.size(3);
  const int K = (int)G.size(1), P = (int)G.size(2), Q = (int)G.size(3);
  TORCH_CHECK(tbamd::wgrad_tinyin_supported(C, K, 4, 4, 2, 1, P, Q, H, W),
              "conv2d_wgrad_tinyin: needs C = 3, K = 64, Q = 64, H = 2P, W = 2Q");
  Tensor part = at::empty({(int64_t)tbamd::wgrad_tinyin_parts(N, P) * K * 48}, T.options().dtype(at::kFloat));
  Tensor dw = at::empty({K, C, 4, 4}, T.options().memory_format(kNHWC));
  tbamd::wgrad_tinyin(T.data_ptr(), G.data_ptr(), dw.data_ptr(), part.data_ptr<float>(), N, P, H, W, cur_stream());
  return dw;
}

// ---------------------------------------------------------------- virtual-input 64-channel convs
// y = conv2d(pad(upsample_nearest(x, up), pad, reflect|zero), w, bias, stride) on the implicit-GEMM
// kernels (bf16, C % 64 == K % 64 == 0, up in {1, 2, 4}): the padded / upsampled input is never
// written (StyleNet residual blocks, AdaIN decoder)
Tensor conv2d_fwd_virtual(const Tensor& x_, const Tensor& w_, const optional<Tensor>& bias, int64_t stride,
                          int64_t pad, int64_t up, bool reflect) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.scalar_type() == at::kBFloat16 && w_.scalar_type() == at::kBFloat16, "conv2d_fwd_virtual: bf16 only");
  TORCH_CHECK(x_.dim() == 4 && w_.dim() == 4 && x_.size(1) == w_.size(1), "conv2d_fwd_virtual: shape");
  TORCH_CHECK(tbamd::conv_fwd_supported((int)x_.size(1), (int)w_.size(0)),
              "conv2d_fwd_virtual: needs C % 64 == 0 and K % 64 == 0");
  TORCH_CHECK(up == 1 || up == 2 || up == 4, "conv2d_fwd_virtual: up must be 1, 2 or 4");
  Tensor x = nhwc(x_);
  Tensor w = nhwc(w_);
  const auto [N, C, H, W, K, R, S, P, Q] = ConvGeom::of(x, w).window(
      stride, pad, up, reflect, ConvGeom::kReflectFits | ConvGeom::kNonEmpty, "conv2d_fwd_virtual");
  Tensor y = at::empty({N, K, P, Q}, x.options().memory_format(kNHWC));
  Tensor bf = f32_or_undef(bias);
  tbamd::conv_fwd_virtual(x.data_ptr(), w.data_ptr(), y.data_ptr(), f32_or_null(bf), N,
                          H, W, C, K, R, S, P, Q, (int)stride, (int)pad, (int)up, reflect ? 1 : 0, cur_stream());
  return y;
}

// dW [K, C, R, S] (channels_last) of conv2d_fwd_virtual
Tensor conv2d_wgrad_virtual(const Tensor& dy_, const Tensor& x_, int64_t R_, int64_t S_, int64_t stride, int64_t pad,
                            int64_t up, bool reflect) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = nhwc(x_);
  Tensor dy = nhwc(dy_);
  ConvGeom g = ConvGeom::of(x, dy, R_, S_);
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && x.scalar_type() == at::kBFloat16, "conv2d_wgrad_virtual: bf16");
  TORCH_CHECK(g.C % 64 == 0 && g.K % 32 == 0 && (up == 1 || up == 2 || up == 4), "conv2d_wgrad_virtual: channels / up");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, up, reflect, 0, "conv2d_wgrad_virtual");
  TORCH_CHECK(g.fits(dy), "conv2d_wgrad_virtual: dy shape");
  Tensor dw = at::empty({K, C, R, S}, x.options().memory_format(kNHWC));
  Tensor work = f32_work(tbamd::conv_wgrad_workspace(N, H, W, C, K, R, S, P, Q, (int)stride, (int)pad), x);
  tbamd::conv_wgrad_virtual(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), f32_or_null(work), N, H, W, C, K, R, S, P, Q,
                            (int)stride, (int)pad, (int)up, reflect ? 1 : 0, cur_stream());
  return dw;
}

// dX [N, C, H, W] of conv2d_fwd_virtual: the gradient on the padded virtual grid from the
// 64-channel dgrad kernels (stride 1: flipped-weight forward with padding R-1; stride 2: the
// four parity classes), folded back onto x (reflect mirror images, upsampled copies)
// wt = conv_flip_weight(w) [C, K, R, S] channels_last
Tensor conv2d_dgrad_virtual(const Tensor& dy_, const Tensor& wt_, int64_t H, int64_t W, int64_t stride, int64_t pad,
                            int64_t up, bool reflect) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  Tensor dy = nhwc(dy_);
  Tensor wt = nhwc(wt_);
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && wt.scalar_type() == at::kBFloat16, "conv2d_dgrad_virtual: bf16");
  const int N = (int)dy.size(0), K = (int)dy.size(1), P = (int)dy.size(2), Q = (int)dy.size(3);
  const int C = (int)wt.size(0), R = (int)wt.size(2), S = (int)wt.size(3);
  TORCH_CHECK(wt.size(1) == K && tbamd::conv_fwd_supported(K, C), "conv2d_dgrad_virtual: wt [C, K, R, S], % 64");
  TORCH_CHECK(stride == 1 || (stride == 2 && tbamd::conv_dgrad_s2_supported(R, S, 2)),
              "conv2d_dgrad_virtual: stride 1, or 2 with <= 16 taps per phase class");
  const int Hp = (int)(H * up + 2 * pad), Wp = (int)(W * up + 2 * pad);
  TORCH_CHECK(P == (Hp - R) / (int)stride + 1 && Q == (Wp - S) / (int)stride + 1, "conv2d_dgrad_virtual: geometry");
  Tensor dxp = at::empty({N, C, Hp, Wp}, dy.options().memory_format(kNHWC));
  if (stride == 1) {
    TORCH_CHECK(R == S, "conv2d_dgrad_virtual: square taps");
    tbamd::conv_fwd(dy.data_ptr(), wt.data_ptr(), dxp.data_ptr(), nullptr, nullptr, nullptr, nullptr, false, N, P, Q, K,
                    C, R, S, Hp, Wp, 1, R - 1, cur_stream());
  } else {
    tbamd::conv_dgrad_s2(dy.data_ptr(), wt.data_ptr(), dxp.data_ptr(), N, P, Q, K, C, R, S, 0, Hp, Wp, cur_stream());
  }
  const tbamd::ConvAnyShape fwd{N, (int)H, (int)W, C, K, R, S, P, Q, (int)stride, (int)pad, (int)up, 1, reflect ? 1 : 0};
  Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(kNHWC));
  tbamd::conv_any_fold(0, dxp.data_ptr(), Hp, Wp, dx.data_ptr(), fwd, cur_stream());
  return dx;
}

// ---------------------------------------------------------------- fp32 through split bf16, split-K
// (hi, lo) bf16 pair of an f32 tensor, same sizes and strides (the layout of t is kept)
std::vector<Tensor> split_bf16(const Tensor& t_) {
  const at::DeviceGuard guard = on_device_of(t_, "t");
  TORCH_CHECK(t_.scalar_type() == at::kFloat, "split_bf16: fp32");
  const bool cl = t_.dim() == 4 && !t_.is_contiguous() && t_.is_contiguous(kNHWC);
  Tensor t = cl ? t_ : t_.contiguous();
  TORCH_CHECK(t.numel() % 4 == 0, "split_bf16: numel % 4");
  Tensor hi = at::empty_like(t, t.options().dtype(at::kBFloat16));
  Tensor lo = at::empty_like(t, t.options().dtype(at::kBFloat16));
  tbamd::split_bf16(t.data_ptr<float>(), t.numel(), (uint16_t*)hi.data_ptr(), (uint16_t*)lo.data_ptr(), cur_stream());
  return {hi, lo};
}

// the f32 contiguous [K] bias of the split kernels, or an undefined tensor
Tensor bias_k(const optional<Tensor>& bias, int K, const char* op) {
  Tensor b = f32_or_undef(bias);
  TORCH_CHECK(!b.defined() || b.numel() == K, op, ": bias");
  return b;
}

// y = conv2d(x, w) (+ bias, ReLU) in fp32 from split-bf16 operands (csrc/conv.hip conv_fwd_split_k):
// xh/xl [N, C, H, W] channels_last, wh/wl [K, C, R, S] channels_last bf16, C % 64 == K % 64 == 0
Tensor conv2d_fwd_split32(const Tensor& xh, const Tensor& xl, const Tensor& wh, const Tensor& wl,
                          const optional<Tensor>& bias, int64_t stride, int64_t pad, bool relu) {
  const at::DeviceGuard guard = on_device_of(xh, "xh");
  for (const Tensor* t : {&xh, &xl, &wh, &wl})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->is_contiguous(kNHWC),
                "conv2d_fwd_split32: bf16 channels_last operands");
  ConvGeom g = ConvGeom::of(xh, wh);
  TORCH_CHECK(wh.size(1) == g.C && g.C % 64 == 0 && g.K % 64 == 0 && xl.sizes() == xh.sizes() &&
                  wl.sizes() == wh.sizes(),
              "conv2d_fwd_split32: shapes");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, 1, false, 0, "conv2d_fwd_split32");
  Tensor y = at::empty({N, K, P, Q}, xh.options().dtype(at::kFloat).memory_format(kNHWC));
  Tensor b = bias_k(bias, K, "conv2d_fwd_split32");
  const int ns = tbamd::conv_fwd_split32_ksplit(N, C, K, R, S, P, Q);
  Tensor part;  // few output pixels: the reduction is split over workgroups (f32 partials)
  if (ns > 1) part = at::empty({(int64_t)ns * N * P * Q * K}, y.options().memory_format(at::MemoryFormat::Contiguous));
  tbamd::conv_fwd_split32(xh.data_ptr(), xl.data_ptr(), wh.data_ptr(), wl.data_ptr(), y.data_ptr<float>(),
                          f32_or_null(b), relu, N, H, W, C, K, R, S, P, Q, (int)stride,
                          (int)pad, cur_stream(), ns > 1 ? part.data_ptr<float>() : nullptr);
  return y;
}

// bf16 forward of a few-pixel conv with the reduction split over workgroups (csrc/conv.hip
// conv_fwd_splitk_bf16): VGG-19 512-channel maps at batch 1; C % 64 == 0, K % 128 == 0
Tensor conv2d_fwd_splitk(const Tensor& x_, const Tensor& w_, const optional<Tensor>& bias, int64_t stride, int64_t pad,
                         bool relu) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = nhwc(x_), w = nhwc(w_);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16, "conv2d_fwd_splitk: bf16");
  ConvGeom g = ConvGeom::of(x, w);
  TORCH_CHECK(w.size(1) == g.C && g.C % 64 == 0 && g.K % 128 == 0 && stride >= 1 && pad >= 0,
              "conv2d_fwd_splitk: shapes");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, 1, false, ConvGeom::kNonEmpty, "conv2d_fwd_splitk");
  Tensor y = at::empty({N, K, P, Q}, x.options().memory_format(kNHWC));
  Tensor b = bias_k(bias, K, "conv2d_fwd_splitk");
  const int ns = std::max(1, tbamd::conv_fwd_splitk_bf16_ksplit(N, C, K, R, S, P, Q));
  Tensor part = at::empty({(int64_t)ns * N * P * Q * K}, x.options().dtype(at::kFloat));
  tbamd::conv_fwd_splitk_bf16(x.data_ptr(), w.data_ptr(), y.data_ptr(), f32_or_null(b),
                              relu, N, H, W, C, K, R, S, P, Q, (int)stride, (int)pad, part.data_ptr<float>(), ns,
                              cur_stream());
  return y;
}

// fp32 dW [K, C, R, S] (channels_last) of a conv over pad(upsample(x)) on the bf16 MFMA weight-gradient
// kernel with split-bf16 operands (csrc/conv_wgrad.hip conv_wgrad_split32); C % 64 == K % 64 == 0
Tensor conv2d_wgrad_split32(const Tensor& dy_, const Tensor& x_, int64_t R_, int64_t S_, int64_t stride, int64_t pad,
                            int64_t up, bool reflect) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  Tensor x = nhwc(x_);
  Tensor dy = nhwc(dy_);
  ConvGeom g = ConvGeom::of(x, dy, R_, S_);
  TORCH_CHECK(dy.scalar_type() == at::kFloat && x.scalar_type() == at::kFloat, "conv2d_wgrad_split32: fp32");
  TORCH_CHECK(g.C % 64 == 0 && g.K % 64 == 0 && (up == 1 || up == 2 || up == 4), "conv2d_wgrad_split32: channels / up");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, up, reflect, 0, "conv2d_wgrad_split32");
  TORCH_CHECK(g.fits(dy), "conv2d_wgrad_split32: dy shape");
  TORCH_CHECK(g.NPQ() < (1ll << 31), "conv2d_wgrad_split32: too many output pixels");
  Tensor dw = at::empty({K, C, R, S}, x.options().memory_format(kNHWC));
  auto bf = x.options().dtype(at::kBFloat16);
  Tensor dyh = at::empty({dy.numel()}, bf), dyl = at::empty({dy.numel()}, bf);
  Tensor xh = at::empty({x.numel()}, bf), xl = at::empty({x.numel()}, bf);
  Tensor work = at::empty({tbamd::conv_wgrad_split32_workspace(N, H, W, C, K, R, S, P, Q, (int)stride, (int)pad)},
                          x.options());
  tbamd::conv_wgrad_split32(dy.data_ptr<float>(), x.data_ptr<float>(), dw.data_ptr<float>(),
                            (uint16_t*)dyh.data_ptr(), (uint16_t*)dyl.data_ptr(), (uint16_t*)xh.data_ptr(),
                            (uint16_t*)xl.data_ptr(), work.data_ptr<float>(), N, H, W, C, K, R, S, P, Q,
                            (int)stride, (int)pad, (int)up, reflect ? 1 : 0, cur_stream());
  return dw;
}

// ---------------------------------------------------------------- im2col / col2im
// x: bf16 [N, C, H, W] channels_last -> col [N*P*Q, KP] (KP = RSC rounded up to 8)
Tensor im2col(const Tensor& x, int64_t R, int64_t S, int64_t P, int64_t Q, int64_t stride, int64_t pad, int64_t up,
              bool reflect) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == at::kBFloat16 && x.dim() == 4 && x.is_contiguous(kNHWC),
              "im2col: expected bf16 channels_last [N, C, H, W]");
  TORCH_CHECK(up == 1 || up == 2 || up == 4, "im2col: upsample 1, 2 or 4");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t KP = (R * S * C + 7) / 8 * 8;
  Tensor col = at::empty({N * P * Q, KP}, x.options().memory_format(at::MemoryFormat::Contiguous));
  tbamd::im2col_nhwc(x.data_ptr(), col.data_ptr(), (int)N, (int)H, (int)W, (int)C, (int)R, (int)S, (int)P, (int)Q,
                     (int)stride, (int)pad, (int)up, reflect ? 1 : 0, (int)KP, cur_stream());
  return col;
}

// col [N*P*Q, KP] -> dx bf16 [N, C, H, W] channels_last (gather; + bias[C] when given)
Tensor col2im(const Tensor& col, int64_t N, int64_t C, int64_t H, int64_t W, int64_t R, int64_t S, int64_t P,
              int64_t Q, int64_t stride, int64_t pad, const optional<Tensor>& bias) {
  TORCH_CHECK(col.is_cuda() && col.dtype() == at::kBFloat16 && col.dim() == 2 && col.is_contiguous(),
              "col2im: expected contiguous bf16 [M, KP]");
  const int64_t KP = col.size(1);
  TORCH_CHECK(col.size(0) == N * P * Q && KP >= R * S * C, "col2im: col shape");
  Tensor b;
  if (given(bias)) {
    b = bias->to(at::kBFloat16).contiguous();
    TORCH_CHECK(b.numel() == C, "col2im: bias size");
  }
  Tensor dx = at::empty({N, C, H, W}, col.options().memory_format(kNHWC));
  tbamd::col2im_nhwc(col.data_ptr(), dx.data_ptr(), ptr_or_null(b), (int)N, (int)H, (int)W,
                     (int)C, (int)R, (int)S, (int)P, (int)Q, (int)stride, (int)pad, (int)KP, cur_stream());
  return dx;
}

}  // namespace

void register_conv(pybind11::module& m) {
  m.def("conv2d_stem_pad", &conv2d_stem_pad);
  m.def("conv2d_stem_fwd", &conv2d_stem_fwd);
  m.def("conv2d_stem_wgrad", &conv2d_stem_wgrad);
  m.def("conv2d_dgrad_s2", &conv2d_dgrad_s2, py::arg("dy"), py::arg("wt"), py::arg("R"), py::arg("S"), py::arg("pad"),
        py::arg("H"), py::arg("W"), py::arg("bnb_mode") = 0, py::arg("bnb_x") = py::none(),
        py::arg("bnb_scale") = py::none(), py::arg("bnb_shift") = py::none(), py::arg("bnb_mean") = py::none(),
        py::arg("bnb_bits") = py::none(), py::arg("stride") = 2);
  m.def("conv_dgrad_s2_supported", &tbamd::conv_dgrad_s2_supported);
  m.def("conv2d_fwd", &conv2d_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("stride"), py::arg("pad"),
        py::arg("relu"), py::arg("want_stats"), py::arg("addend") = py::none(), py::arg("addend_mask") = py::none(),
        py::arg("bnb_mode") = 0, py::arg("bnb_x") = py::none(), py::arg("bnb_scale") = py::none(),
        py::arg("bnb_shift") = py::none(), py::arg("bnb_mean") = py::none(), py::arg("bnb_bits") = py::none(),
        py::arg("big") = -1);
  m.def("conv2d_dgrad_gxf", &conv2d_dgrad_gxf, py::arg("g"), py::arg("wt"), py::arg("addend"),
        py::arg("addend_mask"), py::arg("bnb_mode"), py::arg("bnb_x"), py::arg("bnb_scale"), py::arg("bnb_shift"),
        py::arg("bnb_mean"), py::arg("bnb_bits"), py::arg("gxf"), py::arg("gx_x"), py::arg("gx_bits"),
        py::arg("gx_scale"), py::arg("gx_shift"), py::arg("gx_coef"), py::arg("want_dz"));
  m.def("conv_dgrad_gxf_supported", &conv_dgrad_gxf_supported);
  m.def("conv_fwd_xf_supported", &tbamd::conv_fwd_xf_supported);
  m.def("conv2d_fwd_xf", &conv2d_fwd_xf, py::arg("x"), py::arg("w"), py::arg("scale"), py::arg("shift"),
        py::arg("stride"), py::arg("pad"), py::arg("want_stats") = true);
  m.def("conv_flip_weight", &conv_flip_weight);
  m.def("conv2d_wgrad", &conv2d_wgrad, py::arg("dy"), py::arg("x"), py::arg("R"), py::arg("S"), py::arg("stride"),
        py::arg("pad"), py::arg("out") = py::none());
  m.def("conv2d_wgrad_xf", &conv2d_wgrad_xf, py::arg("dy"), py::arg("x"), py::arg("scale"), py::arg("shift"),
        py::arg("R"), py::arg("S"), py::arg("stride"), py::arg("pad"), py::arg("out") = py::none());
  m.def("conv2d_wgrad_tinyin", &conv2d_wgrad_tinyin, py::arg("T"), py::arg("G"));
  m.def("conv2d_fwd_virtual", &conv2d_fwd_virtual, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("stride"),
        py::arg("pad"), py::arg("up") = 1, py::arg("reflect") = false);
  m.def("conv2d_wgrad_virtual", &conv2d_wgrad_virtual, py::arg("dy"), py::arg("x"), py::arg("R"), py::arg("S"),
        py::arg("stride"), py::arg("pad"), py::arg("up") = 1, py::arg("reflect") = false);
  m.def("conv2d_dgrad_virtual", &conv2d_dgrad_virtual, py::arg("dy"), py::arg("wt"), py::arg("H"), py::arg("W"),
        py::arg("stride"), py::arg("pad"), py::arg("up") = 1, py::arg("reflect") = false);
  m.def("split_bf16", &split_bf16);
  m.def("conv2d_fwd_split32", &conv2d_fwd_split32, py::arg("xh"), py::arg("xl"), py::arg("wh"), py::arg("wl"),
        py::arg("bias") = py::none(), py::arg("stride") = 1, py::arg("pad") = 0, py::arg("relu") = false);
  m.def("conv2d_fwd_splitk", &conv2d_fwd_splitk, py::arg("x"), py::arg("w"), py::arg("bias") = py::none(),
        py::arg("stride") = 1, py::arg("pad") = 0, py::arg("relu") = false);
  m.def("conv_fwd_splitk_ksplit", [](int64_t N, int64_t C, int64_t K, int64_t R, int64_t S, int64_t P, int64_t Q) {
    return tbamd::conv_fwd_splitk_bf16_ksplit((int)N, (int)C, (int)K, (int)R, (int)S, (int)P, (int)Q);
  });
  m.def("conv2d_wgrad_split32", &conv2d_wgrad_split32);
  m.def("im2col", &im2col);
  m.def("col2im", &col2im, py::arg("col"), py::arg("N"), py::arg("C"), py::arg("H"), py::arg("W"), py::arg("R"),
        py::arg("S"), py::arg("P"), py::arg("Q"), py::arg("stride"), py::arg("pad"), py::arg("bias") = py::none());
  // tuning knobs
  m.def("conv_set_stages", &tbamd::conv_set_stages);
  m.def("conv_set_big", &tbamd::conv_set_big);
  m.def("conv_get_big", &tbamd::conv_get_big);
  m.def("conv_big_encode", &tbamd::conv_big_encode);
  m.def("conv_big_choice", &tbamd::conv_big_choice);
  m.def("conv_set_persistent_1x1", &tbamd::conv_set_persistent_1x1);
  m.def("conv_set_occupancy", &tbamd::conv_set_occupancy);
  m.def("conv_wgrad_set_occupancy", &tbamd::conv_wgrad_set_occupancy);
}
