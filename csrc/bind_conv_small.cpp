// Bindings of the convolutions outside the 64-channel family (conv_any.hip, conv_narrow.hip): the
// generic kernels, the narrow-output (K <= 16) halo-tile kernels and the tiny-input-channel kernels.
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "bind_common.h"

namespace {
using namespace tbbind;

const auto kNHWC = at::MemoryFormat::ChannelsLast;
constexpr unsigned kFitsNonEmpty = ConvGeom::kReflectFits | ConvGeom::kNonEmpty;

// ---------------------------------------------------------------- generic convolution
// x [N, C, H, W], w [K, C, R, S] (bf16 or f32, any layout), virtual input
// reflect-or-zero-pad(upsample_nearest(x, up)); NHWC (channels_last) outputs
tbamd::ConvAnyShape any_shape(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t R, int64_t S,
                              int64_t stride, int64_t pad, int64_t up, int64_t dil, bool reflect) {
  ConvGeom g{(int)N, (int)C, (int)H, (int)W, (int)K, (int)R, (int)S, 0, 0};
  g.window(stride, pad, up, reflect, ConvGeom::kReflectFits, "conv_any", dil);
  TORCH_CHECK(g.P > 0 && g.Q > 0 && stride >= 1 && up >= 1 && dil >= 1, "conv_any: bad geometry");
  return tbamd::ConvAnyShape{g.N, g.H, g.W, g.C, g.K, g.R, g.S, g.P, g.Q,
                             (int)stride, (int)pad, (int)up, (int)dil, reflect ? 1 : 0};
}

int any_f32(const Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16, "conv_any: ", name,
              " must be f32 or bf16");
  return t.scalar_type() == at::kFloat ? 1 : 0;
}

Tensor conv_any_fwd(const Tensor& x_, const Tensor& w_, const optional<Tensor>& bias, int64_t stride, int64_t pad,
                    int64_t up, bool reflect) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const int f32 = any_f32(x_, "x");
  TORCH_CHECK(w_.scalar_type() == x_.scalar_type(), "conv_any: x and w dtypes differ");
  Tensor x = nhwc(x_);
  Tensor w = w_.permute({0, 2, 3, 1}).contiguous();  // [K][R][S][C]
  const auto sh = any_shape(x.size(0), x.size(1), x.size(2), x.size(3), w_.size(0), w_.size(2), w_.size(3),
                            stride, pad, up, 1, reflect);
  TORCH_CHECK(w_.size(1) == x.size(1), "conv_any: channel mismatch");
  Tensor b;
  if (given(bias)) b = bias->to(x.scalar_type()).contiguous();
  Tensor y = at::empty({sh.N, sh.K, sh.P, sh.Q}, x.options().memory_format(kNHWC));
  tbamd::conv_any_fwd(f32, x.data_ptr(), w.data_ptr(), ptr_or_null(b), y.data_ptr(), sh, cur_stream());
  return y;
}

// dW [K, C, R, S] (channels_last) for y = conv_any_fwd(x, w, stride, pad, up, reflect)
Tensor conv_any_wgrad(const Tensor& dy_, const Tensor& x_, int64_t R, int64_t S, int64_t stride, int64_t pad,
                      int64_t up, bool reflect) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const int f32 = any_f32(x_, "x");
  TORCH_CHECK(dy_.scalar_type() == x_.scalar_type(), "conv_any: x and dy dtypes differ");
  Tensor x = nhwc(x_);
  Tensor dy = nhwc(dy_);
  const auto sh = any_shape(x.size(0), x.size(1), x.size(2), x.size(3), dy.size(1), R, S, stride, pad, up, 1,
                            reflect);
  TORCH_CHECK(dy.size(2) == sh.P && dy.size(3) == sh.Q && dy.size(0) == sh.N, "conv_any_wgrad: dy shape");
  const int splits = tbamd::conv_any_wgrad_splits(sh);
  Tensor part = at::empty({(int64_t)splits * sh.K * R * S * sh.C}, x.options().dtype(at::kFloat));
  Tensor dw = at::empty({sh.K, sh.C, R, S}, x.options().memory_format(kNHWC));
  tbamd::conv_any_wgrad(f32, x.data_ptr(), dy.data_ptr(), part.data_ptr<float>(), splits, dw.data_ptr(), sh,
                        cur_stream());
  return dw;
}

// dX [N, C, H, W] (channels_last) for y = conv_any_fwd(x, w, stride, pad, up, reflect): the
// forward kernel on dy dilated by the stride with flipped weights (stride-phase tiles: only
// the taps that meet real dy pixels).  Zero padding without upsampling writes dX directly
// (output grid H x W, padding R-1-pad); reflect / upsampled inputs go through the padded
// virtual grid and the fold.  `wt`: the flipped transpose [C][R][S][K] when the caller
// keeps one cached (ops/flipcache.py _flipped), else built here.
Tensor conv_any_dgrad(const Tensor& dy_, const Tensor& w_, int64_t H, int64_t W, int64_t stride, int64_t pad,
                      int64_t up, bool reflect, const optional<Tensor>& wt_) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  const int f32 = any_f32(dy_, "dy");
  TORCH_CHECK(w_.scalar_type() == dy_.scalar_type(), "conv_any: dy and w dtypes differ");
  Tensor dy = nhwc(dy_);
  const int64_t K = w_.size(0), C = w_.size(1), R = w_.size(2), S = w_.size(3);
  const auto fwd = any_shape(dy.size(0), C, H, W, K, R, S, stride, pad, up, 1, reflect);
  TORCH_CHECK(dy.size(1) == K && dy.size(2) == fwd.P && dy.size(3) == fwd.Q, "conv_any_dgrad: dy shape");
  // flipped transpose as a [C][R][S][K] conv weight (out channels C, in channels K)
  Tensor wt;
  if (given(wt_)) {
    wt = wt_->permute({0, 2, 3, 1});
    TORCH_CHECK(wt.is_contiguous() && wt.size(0) == C && wt.size(1) == R && wt.size(2) == S && wt.size(3) == K &&
                    wt.scalar_type() == w_.scalar_type(),
                "conv_any_dgrad: wt must be the channels_last [C, K, R, S] flipped transpose");
  } else {
    wt = w_.flip({2, 3}).permute({1, 2, 3, 0}).contiguous();
  }
  if (!reflect && up == 1 && pad <= R - 1 && pad <= S - 1) {
    auto g = any_shape(dy.size(0), K, fwd.P, fwd.Q, C, R, S, 1, R - 1 - pad, 1, stride, false);
    TORCH_CHECK(g.P <= H && g.Q <= W, "conv_any_dgrad: internal geometry");
    g.P = (int)H;  // rows / cols no tap reaches get zero gradient (the padding reads)
    g.Q = (int)W;
    Tensor dx = at::empty({fwd.N, C, H, W}, dy.options().memory_format(kNHWC));
    tbamd::conv_any_fwd(f32, dy.data_ptr(), wt.data_ptr(), nullptr, dx.data_ptr(), g, cur_stream());
    return dx;
  }
  const int64_t Hg = (int64_t)(fwd.P - 1) * stride + R, Wg = (int64_t)(fwd.Q - 1) * stride + S;
  auto g = any_shape(dy.size(0), K, fwd.P, fwd.Q, C, R, S, 1, R - 1, 1, stride, false);
  TORCH_CHECK(g.P == Hg && g.Q == Wg, "conv_any_dgrad: internal geometry");
  Tensor dxp = at::empty({g.N, Hg, Wg, C}, dy.options().memory_format(at::MemoryFormat::Contiguous));
  // wt is already [Cout=C][R][S][Cin=K]: pass it as the packed weight (conv_any_fwd reads [K][R][S][C])
  tbamd::conv_any_fwd(f32, dy.data_ptr(), wt.data_ptr(), nullptr, dxp.data_ptr(), g, cur_stream());
  Tensor dx = at::empty({fwd.N, C, H, W}, dy.options().memory_format(kNHWC));
  tbamd::conv_any_fold(f32, dxp.data_ptr(), (int)Hg, (int)Wg, dx.data_ptr(), fwd, cur_stream());
  return dx;
}

// ---------------------------------------------------------------- narrow-output convs (K <= 16)
// y = conv2d(pad(upsample_nearest(x, up), pad, reflect|zero), w, bias), stride 1, for K <= 16
// output channels (the RGB heads of the style-transfer decoders): halo-tile kernel.  f32 (the
// reference precision of the style-transfer examples): the kernel splits the fp32 halo into bf16
// hi / lo in LDS, three MFMAs per pair (csrc/conv_narrow.hip conv_narrow_fwd32).
Tensor narrow_fwd(const Tensor& x_, const Tensor& w_, const optional<Tensor>& bias, int64_t pad, int64_t up,
                  bool reflect, bool f32, const char* op) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const auto dt = f32 ? at::kFloat : at::kBFloat16;
  TORCH_CHECK(x_.scalar_type() == dt && w_.scalar_type() == dt, op, f32 ? ": fp32 only" : ": bf16 only");
  TORCH_CHECK(x_.dim() == 4 && w_.dim() == 4 && w_.size(1) == x_.size(1), op, ": shape");
  Tensor x = nhwc(x_);
  ConvGeom g = ConvGeom::of(x, w_);
  TORCH_CHECK(tbamd::conv_narrow_supported(g.C, g.K, g.R, g.S, 1, (int)up) && (!f32 || x.numel() % 4 == 0), op,
              ": unsupported shape");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(1, pad, up, reflect, kFitsNonEmpty, op);
  Tensor w16 = pack_w16(w_.permute({0, 2, 3, 1})), w16h, w16l;
  if (f32) std::tie(w16h, w16l) = split_hi_lo(w16);
  Tensor b = f32_or_undef(bias);
  Tensor y = at::empty({N, K, P, Q}, x.options().memory_format(kNHWC));
  if (f32)
    tbamd::conv_narrow_fwd32(x.data_ptr<float>(), w16h.data_ptr(), w16l.data_ptr(), f32_or_null(b),
                             y.data_ptr<float>(), N, H, W, C, K, R, S, (int)pad, (int)up, reflect ? 1 : 0,
                             cur_stream());
  else
    tbamd::conv_narrow_fwd(x.data_ptr(), w16.data_ptr(), f32_or_null(b), y.data_ptr(), N, H, W, C, K, R, S, (int)pad,
                           (int)up, reflect ? 1 : 0, cur_stream());
  return y;
}

Tensor conv_narrow_fwd(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, int64_t pad, int64_t up,
                       bool reflect) {
  return narrow_fwd(x, w, bias, pad, up, reflect, false, "conv_narrow_fwd");
}

Tensor conv_narrow_fwd_split32(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, int64_t pad,
                               int64_t up, bool reflect) {
  return narrow_fwd(x, w, bias, pad, up, reflect, true, "conv_narrow_fwd_split32");
}

// y = conv_transpose2d(x, w, bias, stride, pad) for <= 16 output channels (the DCGAN generator's
// RGB head): st x st stride phases, each a narrow halo-tile forward with that phase's taps
Tensor conv_narrow_transpose_fwd(const Tensor& x_, const Tensor& w_, const optional<Tensor>& bias, int64_t stride,
                                 int64_t pad) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  TORCH_CHECK(x_.scalar_type() == at::kBFloat16 && w_.scalar_type() == at::kBFloat16,
              "conv_narrow_transpose_fwd: bf16 only");
  TORCH_CHECK(x_.dim() == 4 && w_.dim() == 4 && w_.size(0) == x_.size(1) && w_.size(2) == w_.size(3),
              "conv_narrow_transpose_fwd: x [N, Ci, H, W], w [Ci, Co, R, R]");
  Tensor x = nhwc(x_);
  const int N = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  const int K = (int)w_.size(1), R = (int)w_.size(2), st = (int)stride, p = (int)pad;
  const int Ho = (H - 1) * st - 2 * p + R, Wo = (W - 1) * st - 2 * p + R;
  TORCH_CHECK(st >= 1 && Ho > 0 && Wo > 0, "conv_narrow_transpose_fwd: geometry");
  auto floordiv = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
  auto ceildiv = [&](int a, int b) { return -floordiv(-a, b); };
  Tensor wt = w_.permute({1, 2, 3, 0});  // [Co][R][S][Ci]
  Tensor b = f32_or_undef(bias);
  Tensor y = at::empty({N, K, Ho, Wo}, x.options().memory_format(kNHWC));
  struct Ph { int dmax, taps, n; std::vector<int64_t> k; };
  auto phase = [&](int a, int n_out) {
    Ph ph{};
    ph.dmax = floordiv(R - 1 - a - p, st);
    const int dmin = ceildiv(-a - p, st);
    ph.taps = ph.dmax - dmin + 1;
    ph.n = n_out > a ? (n_out - a + st - 1) / st : 0;
    for (int r = 0; r < ph.taps; ++r) ph.k.push_back(st * (ph.dmax - r) + a + p);
    return ph;
  };
  for (int a = 0; a < st; ++a) {
    const Ph pa = phase(a, Ho);
    TORCH_CHECK(pa.taps >= 1 && pa.taps <= 9, "conv_narrow_transpose_fwd: phase taps");
    for (int bb = 0; bb < st; ++bb) {
      const Ph pb = phase(bb, Wo);
      TORCH_CHECK(pb.taps >= 1 && pb.taps <= 9, "conv_narrow_transpose_fwd: phase taps");
      TORCH_CHECK(tbamd::conv_narrow_supported(C, K, pa.taps, pb.taps, 1, 1), "conv_narrow_transpose_fwd: shape");
      if (pa.n == 0 || pb.n == 0) continue;
      // the phase's taps are ky = st * (dmax - r') + a + p: a stride-st slice of the kernel,
      // reversed (no index tensors, no host-to-device copies)
      const int64_t ky0 = pa.k.back(), kx0 = pb.k.back();
      Tensor sel = wt.slice(1, ky0, pa.k.front() + 1, st).slice(2, kx0, pb.k.front() + 1, st).flip({1, 2});
      Tensor w16 = pack_w16(sel);
      tbamd::conv_narrow_fwd_phase(x.data_ptr(), w16.data_ptr(), f32_or_null(b),
                                   y.data_ptr(), N, H, W, C, K, pa.taps, pb.taps, pa.dmax, pb.dmax, pa.n, pb.n, st, a,
                                   bb, Ho, Wo, cur_stream());
    }
  }
  return y;
}

// dW [K, C, R, S] (channels_last) of conv_narrow_fwd's convolution: split-K partials over pixel
// tiles [splits][16][R*S][C] f32 from the halo-tile kernel, summed here.  f32 (the style decoders'
// 9x9 RGB heads at the reference precision): dy and x split into bf16 (hi, lo) pairs,
// dW = dyh.xh + dyh.xl + dyl.xh as three kernel runs into one f32 partial workspace, summed in f32.
Tensor narrow_wgrad(const Tensor& dy_, const Tensor& x_, int64_t R_, int64_t S_, int64_t pad, int64_t up, bool reflect,
                    bool f32, const char* op) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const auto dt = f32 ? at::kFloat : at::kBFloat16;
  TORCH_CHECK(x_.scalar_type() == dt && dy_.scalar_type() == dt, op, f32 ? ": fp32" : ": bf16 only");
  Tensor x = nhwc(x_);
  Tensor dy = nhwc(dy_);
  ConvGeom g = ConvGeom::of(x, dy, R_, S_);
  TORCH_CHECK(tbamd::conv_narrow_supported(g.C, g.K, g.R, g.S, 1, (int)up), op, ": unsupported shape");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(1, pad, up, reflect, ConvGeom::kReflectFits, op);
  TORCH_CHECK(!f32 || (x.numel() % 4 == 0 && dy.numel() % 4 == 0), op, ": numel % 4");
  TORCH_CHECK(g.fits(dy), op, ": dy shape");
  Tensor xh, xl, dyh, dyl;
  if (f32) {
    auto bf = x.options().dtype(at::kBFloat16).memory_format(kNHWC);
    xh = at::empty_like(x, bf), xl = at::empty_like(x, bf), dyh = at::empty_like(dy, bf), dyl = at::empty_like(dy, bf);
    tbamd::split_bf16(x.data_ptr<float>(), x.numel(), (uint16_t*)xh.data_ptr(), (uint16_t*)xl.data_ptr(), cur_stream());
    tbamd::split_bf16(dy.data_ptr<float>(), dy.numel(), (uint16_t*)dyh.data_ptr(), (uint16_t*)dyl.data_ptr(),
                      cur_stream());
  }
  const int splits = tbamd::conv_narrow_wgrad_splits(N, H, W, C, R, S, (int)pad, (int)up);
  const int runs = f32 ? 3 : 1;
  Tensor part = at::empty({runs * splits, 16, R * S, C}, x.options().dtype(at::kFloat));
  const Tensor* xs[3] = {f32 ? &xh : &x, &xl, &xh};
  const Tensor* ds[3] = {f32 ? &dyh : &dy, &dyh, &dyl};
  for (int t = 0; t < runs; ++t)
    tbamd::conv_narrow_wgrad(xs[t]->data_ptr(), ds[t]->data_ptr(), part.data_ptr<float>() + (int64_t)t * splits * 16 * R * S * C,
                             splits, N, H, W, C, K, R, S, (int)pad, (int)up, reflect ? 1 : 0, cur_stream());
  Tensor dw = part.narrow(1, 0, K).sum(0).view({K, R, S, C}).permute({0, 3, 1, 2});
  return f32 ? dw : dw.to(at::kBFloat16);
}

Tensor conv_narrow_wgrad(const Tensor& dy, const Tensor& x, int64_t R, int64_t S, int64_t pad, int64_t up,
                         bool reflect) {
  return narrow_wgrad(dy, x, R, S, pad, up, reflect, false, "conv_narrow_wgrad");
}

Tensor conv_narrow_wgrad_split32(const Tensor& dy, const Tensor& x, int64_t R, int64_t S, int64_t pad, int64_t up,
                                 bool reflect) {
  return narrow_wgrad(dy, x, R, S, pad, up, reflect, true, "conv_narrow_wgrad_split32");
}

// ---------------------------------------------------------------- tiny-input-channel convs
// reduction index -> (r | s << 8 | c << 16) of the tiny-channel kernels, cached per (device, C, R, S)
Tensor tiny_tab(const Tensor& x, int C, int R, int S) {
  const int kred = C * R * S;
  static std::mutex mu;
  static std::map<std::tuple<int, int, int, int>, Tensor> tabs;
  Tensor tab;
  {
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple((int)x.get_device(), C, R, S);
    auto it = tabs.find(key);
    if (it == tabs.end()) {
      std::vector<int32_t> h(kred);
      for (int k = 0; k < kred; ++k) {
        const int c = k % C, rs = k / C;
        h[k] = (rs / S) | ((rs % S) << 8) | (c << 16);
      }
      Tensor t = at::empty({kred}, at::TensorOptions().dtype(at::kInt));
      std::memcpy(t.data_ptr<int32_t>(), h.data(), sizeof(int32_t) * kred);
      it = tabs.emplace(key, t.to(x.device())).first;
    }
    tab = it->second;
  }
  return tab;
}

// y = conv2d(pad(x), w, bias, stride) (+ ReLU) for C*R*S <= 256 input taps (RGB / grey input convs):
// the im2col row is gathered straight into the MFMA operand (csrc/conv_narrow.hip conv_tinyc_fwd).
// f32: as split-bf16 MFMA, the im2col values split in registers, the packed weights as a hi / lo
// pair (conv_tiny32_fwd).
Tensor tiny_fwd(const Tensor& x_, const Tensor& w_, const optional<Tensor>& bias, int64_t stride, int64_t pad,
                bool reflect, bool relu, bool f32, const char* op) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const auto dt = f32 ? at::kFloat : at::kBFloat16;
  TORCH_CHECK(x_.scalar_type() == dt && w_.scalar_type() == dt, op, f32 ? ": fp32 only" : ": bf16 only");
  TORCH_CHECK(x_.dim() == 4 && w_.dim() == 4 && w_.size(1) == x_.size(1), op, ": shape");
  Tensor x = nhwc(x_);
  ConvGeom g = ConvGeom::of(x, w_);
  TORCH_CHECK(tbamd::conv_tinyc_supported(g.C, g.K, g.R, g.S) && stride >= 1, op, ": unsupported shape");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(stride, pad, 1, reflect, kFitsNonEmpty, op);
  Tensor wp = pack_tiny(w_), wph, wpl;
  if (f32) std::tie(wph, wpl) = split_hi_lo(wp);
  Tensor tab = tiny_tab(x, C, R, S);
  Tensor b = f32_or_undef(bias);
  Tensor y = at::empty({N, K, P, Q}, x.options().memory_format(kNHWC));
  if (f32)
    tbamd::conv_tiny32_fwd(x.data_ptr<float>(), wph.data_ptr(), wpl.data_ptr(), tab.data_ptr<int32_t>(),
                           f32_or_null(b), y.data_ptr<float>(), N, H, W, C, K, R, S,
                           (int)stride, (int)pad, reflect ? 1 : 0, relu, cur_stream());
  else
    tbamd::conv_tinyc_fwd(x.data_ptr(), wp.data_ptr(), tab.data_ptr<int32_t>(), f32_or_null(b),
                          y.data_ptr(), N, H, W, C, K, R, S, (int)stride, (int)pad, reflect ? 1 : 0, relu, cur_stream());
  return y;
}

Tensor conv_tinyc_fwd(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, int64_t stride, int64_t pad,
                      bool reflect, bool relu) {
  return tiny_fwd(x, w, bias, stride, pad, reflect, relu, false, "conv_tinyc_fwd");
}

Tensor conv_tiny32_fwd(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, int64_t stride, int64_t pad,
                       bool reflect, bool relu) {
  return tiny_fwd(x, w, bias, stride, pad, reflect, relu, true, "conv_tiny32_fwd");
}

// stride-1 conv with C <= 4 input channels from an LDS halo tile (csrc/conv_narrow.hip conv_tinyhalo_fwd):
// bf16, or fp32 as split-bf16 (x split while staging, weights packed as a hi / lo pair)
Tensor conv_tinyhalo_fwd(const Tensor& x_, const Tensor& w_, const optional<Tensor>& bias, int64_t pad, bool reflect,
                         bool relu) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const bool f32 = x_.scalar_type() == at::kFloat;
  TORCH_CHECK((f32 || x_.scalar_type() == at::kBFloat16) && w_.scalar_type() == x_.scalar_type(),
              "conv_tinyhalo_fwd: fp32 or bf16");
  TORCH_CHECK(x_.dim() == 4 && w_.dim() == 4 && w_.size(1) == x_.size(1), "conv_tinyhalo_fwd: shape");
  Tensor x = nhwc(x_);
  ConvGeom g = ConvGeom::of(x, w_);
  TORCH_CHECK(tbamd::conv_tinyhalo_supported(g.C, g.K, g.R, g.S, 1, 1), "conv_tinyhalo_fwd: unsupported shape");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(1, pad, 1, reflect, kFitsNonEmpty, "conv_tinyhalo_fwd");
  const int KT = (R * S + 7) / 8;
  // [K][R*S][4] (channels past C zero) -> [K][32*KT] (taps past R*S zero)
  Tensor wf = at::zeros({K, 8 * KT, 4}, w_.options().dtype(at::kFloat).memory_format(at::MemoryFormat::Contiguous));
  wf.narrow(1, 0, R * S).narrow(2, 0, C).copy_(w_.permute({0, 2, 3, 1}).reshape({K, R * S, C}));
  wf = wf.view({K, 32 * KT});
  Tensor wph = wf.to(at::kBFloat16);
  Tensor wpl = f32 ? (wf - wph.to(at::kFloat)).to(at::kBFloat16) : wph;
  Tensor b = f32_or_undef(bias);
  Tensor y = at::empty({N, K, P, Q}, x.options().memory_format(kNHWC));
  tbamd::conv_tinyhalo_fwd(f32, x.data_ptr(), wph.data_ptr(), wpl.data_ptr(), f32_or_null(b),
                           y.data_ptr(), N, H, W, C, K, R, S, (int)pad, reflect ? 1 : 0, relu, cur_stream());
  return y;
}

// dW [K, C, R, S] (channels_last) of conv_tinyhalo_fwd's convolution (csrc/conv_narrow.hip conv_tinyhalo_wgrad)
Tensor conv_tinyhalo_wgrad(const Tensor& dy_, const Tensor& x_, int64_t R_, int64_t S_, int64_t pad, bool reflect) {
  const at::DeviceGuard guard = on_device_of(x_, "x");
  const bool f32 = x_.scalar_type() == at::kFloat;
  TORCH_CHECK((f32 || x_.scalar_type() == at::kBFloat16) && dy_.scalar_type() == x_.scalar_type(),
              "conv_tinyhalo_wgrad: fp32 or bf16");
  Tensor x = nhwc(x_);
  Tensor dy = nhwc(dy_);
  ConvGeom g = ConvGeom::of(x, dy, R_, S_);
  TORCH_CHECK(tbamd::conv_tinyhalo_supported(g.C, g.K, g.R, g.S, 1, 1) && g.K <= 64, "conv_tinyhalo_wgrad: shape");
  const auto [N, C, H, W, K, R, S, P, Q] = g.window(1, pad, 1, reflect, ConvGeom::kReflectFits, "conv_tinyhalo_wgrad");
  TORCH_CHECK(g.fits(dy), "conv_tinyhalo_wgrad: dy shape");
  const int nb = tbamd::conv_tinyhalo_wgrad_blocks(N, H, W, R, S, (int)pad);
  const int NJ = tbamd::conv_tinyhalo_wgrad_cols(R, S);
  Tensor part = at::empty({(int64_t)nb * K * 16 * NJ}, x.options().dtype(at::kFloat).memory_format(at::MemoryFormat::Contiguous));
  Tensor dw = at::empty({K, C, R, S}, x.options().memory_format(kNHWC));
  tbamd::conv_tinyhalo_wgrad(f32, x.data_ptr(), dy.data_ptr(), part.data_ptr<float>(), dw.data_ptr(), N, H, W, C, K,
                             R, S, (int)pad, reflect ? 1 : 0, cur_stream());
  return dw;
}

}  // namespace

void register_conv_small(pybind11::module& m) {
  m.def("conv_any_fwd", &conv_any_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("stride"),
        py::arg("pad"), py::arg("up") = 1, py::arg("reflect") = false);
  m.def("conv_any_wgrad", &conv_any_wgrad, py::arg("dy"), py::arg("x"), py::arg("R"), py::arg("S"),
        py::arg("stride"), py::arg("pad"), py::arg("up") = 1, py::arg("reflect") = false);
  m.def("conv_any_dgrad", &conv_any_dgrad, py::arg("dy"), py::arg("w"), py::arg("H"), py::arg("W"),
        py::arg("stride"), py::arg("pad"), py::arg("up") = 1, py::arg("reflect") = false, py::arg("wt") = py::none());
  m.def("conv_any_set_f32_split", &tbamd::conv_any_set_f32_split, py::arg("on"),
        "fp32 generic convs: split-bf16 MFMA (true, default) or exact-f32 MFMA (false)");
  m.def("conv_any_f32_split", &tbamd::conv_any_f32_split);
  m.def("conv_narrow_fwd", &conv_narrow_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("pad"),
        py::arg("up") = 1, py::arg("reflect") = false);
  m.def("conv_narrow_fwd_split32", &conv_narrow_fwd_split32, py::arg("x"), py::arg("w"), py::arg("bias"),
        py::arg("pad"), py::arg("up") = 1, py::arg("reflect") = false);
  m.def("conv_narrow_transpose_fwd", &conv_narrow_transpose_fwd, py::arg("x"), py::arg("w"), py::arg("bias"),
        py::arg("stride"), py::arg("pad"));
  m.def("conv_narrow_wgrad", &conv_narrow_wgrad, py::arg("dy"), py::arg("x"), py::arg("R"), py::arg("S"),
        py::arg("pad"), py::arg("up") = 1, py::arg("reflect") = false);
  m.def("conv_narrow_wgrad_split32", &conv_narrow_wgrad_split32);
  m.def("conv_tinyc_fwd", &conv_tinyc_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("stride"),
        py::arg("pad"), py::arg("reflect") = false, py::arg("relu") = false);
  m.def("conv_tiny32_fwd", &conv_tiny32_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("stride"),
        py::arg("pad"), py::arg("reflect") = false, py::arg("relu") = false);
  m.def("conv_tinyhalo_fwd", &conv_tinyhalo_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("pad"),
        py::arg("reflect") = false, py::arg("relu") = false);
  m.def("conv_tinyhalo_wgrad", &conv_tinyhalo_wgrad, py::arg("dy"), py::arg("x"), py::arg("R"), py::arg("S"),
        py::arg("pad"), py::arg("reflect") = false);
}
