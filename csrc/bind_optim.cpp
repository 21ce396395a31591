// Bindings of the multi-tensor kernels (optim.hip): optimizer steps, gradient norm / scaling, and
// the batched weight flip of the conv input gradients.
#include "bind_common.h"

namespace {
using namespace tbbind;

void adamw_mt(const Tensor& chunks, int64_t nchunks, const Tensor& table, int64_t pdt, int64_t gdt,
              bool master, bool ema, bool amsgrad, double lr, double beta1, double beta2, double eps,
              double wd, double bc1, double bc2_sqrt, double ema_decay, const optional<Tensor>& clip_coef,
              const optional<Tensor>& inv_scale, const optional<Tensor>& found_inf,
              const optional<Tensor>& hyper) {
  const at::DeviceGuard guard(table.device());
  tbamd::adamw_mt((int)pdt, (int)gdt, master, ema, amsgrad, chunks.data_ptr(), (int)nchunks,
                  table.data_ptr<int64_t>(), (float)lr, (float)beta1, (float)beta2, (float)eps, (float)wd,
                  (float)bc1, (float)bc2_sqrt, (float)ema_decay, fptr(clip_coef), fptr(inv_scale),
                  fptr(found_inf), cur_stream(), fptr(hyper));
}

void sgd_mt(const Tensor& chunks, int64_t nchunks, const Tensor& table, int64_t pdt, int64_t gdt,
            bool master, double momentum, double dampening, bool nesterov, double wd, double lr,
            bool first_step, const optional<Tensor>& clip_coef, const optional<Tensor>& inv_scale,
            const optional<Tensor>& found_inf, const optional<Tensor>& hyper) {
  const at::DeviceGuard guard(table.device());
  tbamd::sgd_mt((int)pdt, (int)gdt, master, (float)momentum, (float)dampening, nesterov, (float)wd,
                (float)lr, first_step ? 1 : 0, chunks.data_ptr(), (int)nchunks, table.data_ptr<int64_t>(),
                fptr(clip_coef), fptr(inv_scale), fptr(found_inf), cur_stream(), fptr(hyper));
}

// returns [norm, clip_coef, nonfinite]
Tensor grad_norm_mt(const Tensor& chunks, int64_t nchunks, const Tensor& table, int64_t gdt,
                    double max_norm, const optional<Tensor>& inv_scale, const Tensor& partial) {
  const at::DeviceGuard guard(table.device());
  Tensor out = at::empty({3}, table.options().dtype(at::kFloat));
  tbamd::grad_norm_mt((int)gdt, chunks.data_ptr(), (int)nchunks, table.data_ptr<int64_t>(),
                      (float)max_norm, fptr(inv_scale), partial.data_ptr<float>(), out.data_ptr<float>(),
                      cur_stream());
  return out;
}

Tensor grad_norm_multi(const std::vector<Tensor>& chunks, const std::vector<int64_t>& nchunks,
                       const std::vector<Tensor>& tables, const std::vector<int64_t>& gdts, double max_norm,
                       const optional<Tensor>& inv_scale) {
  TORCH_CHECK(!tables.empty() && chunks.size() == tables.size() && nchunks.size() == tables.size() &&
                  gdts.size() == tables.size(), "grad_norm_multi: list sizes");
  const at::DeviceGuard guard(tables[0].device());
  const int ng = (int)tables.size();
  std::vector<const void*> cp(ng);
  std::vector<const int64_t*> tp(ng);
  std::vector<int> nc(ng), gd(ng);
  int64_t total = 0;
  for (int i = 0; i < ng; ++i) {
    cp[i] = chunks[i].data_ptr();
    tp[i] = tables[i].data_ptr<int64_t>();
    nc[i] = (int)nchunks[i];
    gd[i] = (int)gdts[i];
    total += nchunks[i];
  }
  Tensor partial = at::empty({std::max<int64_t>(total, 1)}, tables[0].options().dtype(at::kFloat));
  Tensor out = at::empty({3}, tables[0].options().dtype(at::kFloat));
  tbamd::grad_norm_multi(ng, gd.data(), cp.data(), nc.data(), tp.data(), (float)max_norm, fptr(inv_scale),
                         partial.data_ptr<float>(), out.data_ptr<float>(), cur_stream());
  return out;
}

void scale_mt(const Tensor& chunks, int64_t nchunks, const Tensor& table, int64_t gdt, const Tensor& s) {
  const at::DeviceGuard guard(table.device());
  tbamd::scale_mt((int)gdt, chunks.data_ptr(), (int)nchunks, table.data_ptr<int64_t>(),
                  s.data_ptr<float>(), cur_stream());
}

// several flipped copies in one launch: chunks int32x2+int64x2 rows (tensor, pad, start, len)
// as an int64 [n, 3] tensor (first column packs tensor index), table int64 [T, 8]
void conv_flip_weights_mt(const Tensor& chunks, int64_t nchunks, const Tensor& table) {
  const at::DeviceGuard guard(table.device());
  TORCH_CHECK(table.scalar_type() == at::kLong && chunks.scalar_type() == at::kLong, "conv_flip_weights_mt: int64 tables");
  tbamd::conv_flip_transpose_weights_mt(chunks.data_ptr(), (int)nchunks, table.data_ptr<int64_t>(), cur_stream());
}

}  // namespace

void register_optim(pybind11::module& m) {
  m.def("adamw_mt", &adamw_mt, py::arg("chunks"), py::arg("nchunks"), py::arg("table"), py::arg("pdt"),
        py::arg("gdt"), py::arg("master"), py::arg("ema"), py::arg("amsgrad"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("wd"), py::arg("bc1"), py::arg("bc2_sqrt"), py::arg("ema_decay"),
        py::arg("clip_coef"), py::arg("inv_scale"), py::arg("found_inf"), py::arg("hyper") = py::none());
  m.def("sgd_mt", &sgd_mt, py::arg("chunks"), py::arg("nchunks"), py::arg("table"), py::arg("pdt"), py::arg("gdt"),
        py::arg("master"), py::arg("momentum"), py::arg("dampening"), py::arg("nesterov"), py::arg("wd"),
        py::arg("lr"), py::arg("first_step"), py::arg("clip_coef"), py::arg("inv_scale"), py::arg("found_inf"),
        py::arg("hyper") = py::none());
  m.def("grad_norm_mt", &grad_norm_mt);
  m.def("grad_norm_multi", &grad_norm_multi);
  m.def("scale_mt", &scale_mt);
  m.def("conv_flip_weights_mt", &conv_flip_weights_mt, py::arg("chunks"), py::arg("nchunks"), py::arg("table"));
}
