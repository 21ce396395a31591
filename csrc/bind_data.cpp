// Bindings of the input-pipeline kernels (data.hip).
#include "bind_common.h"

namespace {
using namespace tbbind;

// in: uint8 [N, Hi, Wi, C] on the GPU -> [N, C, Ho, Wo] (channels_last memory)
Tensor u8_crop_flip_normalize(const Tensor& in_, int64_t Ho, int64_t Wo, const optional<Tensor>& offs,
                              const optional<Tensor>& flip, const Tensor& mean, const Tensor& inv_std,
                              at::ScalarType out_dtype) {
  const at::DeviceGuard guard = on_device_of(in_, "images");
  TORCH_CHECK(in_.scalar_type() == at::kByte && in_.dim() == 4, "expected uint8 [N, H, W, C]");
  Tensor in = in_.contiguous();
  const int N = (int)in.size(0), Hi = (int)in.size(1), Wi = (int)in.size(2), C = (int)in.size(3);
  TORCH_CHECK(C >= 1 && C <= 4, "1..4 channels supported");
  Tensor m = mean.to(in.device(), at::kFloat).contiguous();
  Tensor is = inv_std.to(in.device(), at::kFloat).contiguous();
  TORCH_CHECK(m.numel() == C && is.numel() == C, "mean/std size");
  Tensor o, f;
  if (given(offs)) {
    o = offs->to(in.device(), at::kInt).contiguous();
    TORCH_CHECK(o.numel() == 2 * N, "offsets must be [N, 2]");
  }
  if (given(flip)) {
    f = flip->to(in.device(), at::kByte).contiguous();
    TORCH_CHECK(f.numel() == N, "flip must be [N]");
  }
  Tensor out = at::empty({N, Ho, Wo, C}, in.options().dtype(out_dtype));
  tbamd::u8_crop_flip_normalize(dt_code(out), in.data_ptr<uint8_t>(), N, Hi, Wi, C, (int)Ho, (int)Wo,
                                o.defined() ? o.data_ptr<int32_t>() : nullptr,
                                f.defined() ? f.data_ptr<uint8_t>() : nullptr, m.data_ptr<float>(),
                                is.data_ptr<float>(), out.data_ptr(), cur_stream());
  return out.permute({0, 3, 1, 2});
}

// images uint8 [Nsrc, Hi, Wi, C] (device); src int32 [B] rows (optional: 0..B-1); params f32 [B, 8]
// (see csrc/data.hip augment_u8_k) -> [B, C, Ho, Wo] channels_last
Tensor augment_u8(const Tensor& in_, const optional<Tensor>& src, int64_t Ho, int64_t Wo, const Tensor& params,
                  const Tensor& mean, const Tensor& inv_std, at::ScalarType out_dtype, bool crop_only) {
  const at::DeviceGuard guard = on_device_of(in_, "images");
  TORCH_CHECK(in_.scalar_type() == at::kByte && in_.dim() == 4, "augment_u8: expected uint8 [N, H, W, C]");
  Tensor in = in_.contiguous();
  const int Hi = (int)in.size(1), Wi = (int)in.size(2), C = (int)in.size(3);
  TORCH_CHECK(crop_only || Ho * Wo * C <= tbamd::augment_max_bytes(),
              "augment_u8: rotation / RandAugment need the image in LDS (", tbamd::augment_max_bytes(),
              " B); larger images support crop + flip only");
  TORCH_CHECK(params.dim() == 2 && params.size(1) == 8, "augment_u8: params must be [B, 8]");
  const int B = (int)params.size(0);
  Tensor pr = params.to(in.device(), at::kFloat).contiguous();
  Tensor sr;
  if (given(src)) {
    sr = src->to(in.device(), at::kInt).contiguous();
    TORCH_CHECK(sr.numel() == B, "augment_u8: src must be [B]");
  } else {
    TORCH_CHECK(in.size(0) == B, "augment_u8: without src the batch is the image tensor");
  }
  Tensor m = mean.to(in.device(), at::kFloat).contiguous();
  Tensor is = inv_std.to(in.device(), at::kFloat).contiguous();
  TORCH_CHECK(m.numel() == C && is.numel() == C, "augment_u8: mean/std size");
  Tensor out = at::empty({B, Ho, Wo, C}, in.options().dtype(out_dtype));
  (crop_only ? tbamd::crop_flip_u8 : tbamd::augment_u8)(
      dt_code(out), in.data_ptr<uint8_t>(), sr.defined() ? sr.data_ptr<int32_t>() : nullptr, B, Hi, Wi, C, (int)Ho,
      (int)Wo, pr.data_ptr<float>(), m.data_ptr<float>(), is.data_ptr<float>(), out.data_ptr(), cur_stream());
  return out.permute({0, 3, 1, 2});
}

}  // namespace

void register_data(pybind11::module& m) {
  m.def("u8_crop_flip_normalize", &u8_crop_flip_normalize);
  m.def("augment_u8", &augment_u8, py::arg("images"), py::arg("src"), py::arg("Ho"), py::arg("Wo"),
        py::arg("params"), py::arg("mean"), py::arg("inv_std"), py::arg("out_dtype"), py::arg("crop_only") = false);
}
