// Bindings of the dense GEMM kernels (gemm.hip, gemm8.hip) and of the bias-gradient / GELU kernels
// that go with them (colsum.hip).
#include "bind_common.h"

namespace {
using namespace tbbind;

void check_rows_bf16(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, "gemm: ", name, " must be bf16");
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) % 8 == 0, "gemm: ", name,
              " must be a 2-D row-major view with a row stride multiple of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "gemm: ", name, " must be 16-B aligned");
}

// y = epi(x @ w^T) (tw false, w [Q][K]) or epi(x @ w) (tw true, w [K][Q]); x [P][K], or
// x [K][P] with tx (y = x^T @ ...).  splits > 1: split-K with f32 partials (no epilogue);
// splits = 0: automatic split count (no epilogue only).
std::vector<Tensor> gemm(const Tensor& x, const Tensor& w, bool tw, const optional<Tensor>& bias,
                         const optional<Tensor>& residual, int64_t epi, bool want_z, int64_t tile,
                         const optional<Tensor>& out, bool tx, int64_t splits) {
  check_rows_bf16(x, "x");
  const at::DeviceGuard guard(x.device());
  Tensor wc = w.contiguous();
  check_rows_bf16(wc, "w");
  const int64_t P = tx ? x.size(1) : x.size(0), K = tx ? x.size(0) : x.size(1);
  const int64_t Q = tw ? wc.size(1) : wc.size(0);
  TORCH_CHECK((tw ? wc.size(0) : wc.size(1)) == K, "gemm: inner dimensions differ");
  // row-read operands move k in 16-B chunks; transposed ones move whole k rows
  TORCH_CHECK(Q % 8 == 0 && ((tx && tw) || K % 8 == 0), "gemm: Q (and K unless both operands are transposed) "
              "must be multiples of 8");
  TORCH_CHECK(!tx || P % 8 == 0, "gemm: P must be a multiple of 8 with a transposed x");
  TORCH_CHECK(P < (1ll << 31) && Q < (1ll << 31) && K < (1ll << 31), "gemm: dims too large");
  Tensor y;
  if (given(out)) {
    y = *out;
    check_rows_bf16(y, "out");
    TORCH_CHECK(y.size(0) == P && y.size(1) == Q, "gemm: out shape");
  } else {
    y = at::empty({P, Q}, x.options());
  }
  Tensor bc;
  if (given(bias)) {
    bc = bias->to(at::kBFloat16).contiguous();
    TORCH_CHECK(bc.numel() == Q, "gemm: bias size");
  }
  const void* bp = ptr_or_null(bc);
  Tensor rc;
  if (given(residual)) {
    rc = residual->to(at::kBFloat16).contiguous();
    TORCH_CHECK(rc.dim() == 2 && rc.size(0) == P && rc.size(1) == Q && y.stride(0) == Q, "gemm: residual shape");
  }
  const void* rp = ptr_or_null(rc);
  TORCH_CHECK(!((epi == 1 || epi == 2 || epi == 3 || epi == 6) && bp == nullptr), "gemm: epilogue needs a bias");
  TORCH_CHECK(!((epi == 3 || epi == 4) && rp == nullptr), "gemm: epilogue needs a residual");
  int t = (int)tile;
  if (t < 0 || t >= tbamd::gemm_num_tiles()) t = tbamd::gemm_pick_tile((int)P, (int)Q, (int)K);
  int s = (int)splits;
  if (s == 0) s = epi == 0 ? tbamd::gemm_pick_splits((int)P, (int)Q, (int)K, t) : 1;
  if (t >= 16 && !tx) s = 1;  // the 8-phase NT / NN kernel (and its whole-round + tail split) runs whole-k tiles
  TORCH_CHECK(s == 1 || epi == 0, "gemm: split-K has no epilogue");
  Tensor part;
  if (s > 1) part = at::empty({(int64_t)s * P * Q}, x.options().dtype(at::kFloat));
  Tensor z;
  if (epi == 2 && want_z) z = at::empty({P, Q}, x.options());
  tbamd::gemm_bf16(x.data_ptr(), x.stride(0), tx, wc.data_ptr(), tw, y.data_ptr(), y.stride(0), bp, rp,
                   ptr_or_null(z), (int)P, (int)Q, (int)K, (int)epi, t, s, f32_or_null(part), cur_stream());
  if (z.defined()) return {y, z};
  return {y};
}

// dZ = (dy @ w) * GELU'(z) and db = column sums of dZ, in one 8-phase NN GEMM (csrc/gemm8.hip):
// the input gradient of a Linear whose input was GELU(z) fused with that GELU's backward and the
// preceding Linear's bias gradient (ViT MLP fc2 -> fc1).  dy [P][K], w [K][Q], z [P][Q] bf16.
std::vector<Tensor> gemm_nn_gelu_bwd(const Tensor& dy, const Tensor& w_, const Tensor& z_,
                                     const optional<Tensor>& db_out, const optional<Tensor>& wt_) {
  check_rows_bf16(dy, "dy");
  const at::DeviceGuard guard(dy.device());
  Tensor w = w_.contiguous();
  Tensor z = z_.contiguous();
  check_rows_bf16(w, "w");
  check_rows_bf16(z, "z");
  const int64_t P = dy.size(0), K = dy.size(1), Q = w.size(1);
  TORCH_CHECK(w.size(0) == K && z.size(0) == P && z.size(1) == Q, "gemm_nn_gelu_bwd: shapes");
  TORCH_CHECK(tbamd::gemm8_nn_supported((int)P, (int)Q, (int)K, dy.stride(0)),
              "gemm_nn_gelu_bwd: needs K % 64 == 0 and Q % 8 == 0");
  Tensor y = at::empty({P, Q}, dy.options());
  const int ntp = (int)((P + 255) / 256);
  Tensor part = at::empty({(int64_t)ntp * Q}, dy.options().dtype(at::kFloat));
  Tensor db;
  if (given(db_out)) {
    db = *db_out;
    TORCH_CHECK(db.is_contiguous() && db.numel() == Q, "gemm_nn_gelu_bwd: db_out");
  } else {
    db = at::empty({Q}, dy.options());
  }
  if (given(wt_)) {  // wt = wᵀ [Q][K]: the NT kernel (row-read operands)
    const Tensor& wt = *wt_;
    check_rows_bf16(wt, "wt");
    TORCH_CHECK(wt.is_contiguous() && wt.size(0) == Q && wt.size(1) == K, "gemm_nn_gelu_bwd: wt must be w^T");
    tbamd::gemm8_nt_gelu_bwd_bf16(dy.data_ptr(), dy.stride(0), wt.data_ptr(), y.data_ptr(), Q, z.data_ptr(),
                                  part.data_ptr<float>(), (int)P, (int)Q, (int)K, cur_stream());
  } else {
    tbamd::gemm8_nn_bf16(dy.data_ptr(), dy.stride(0), w.data_ptr(), y.data_ptr(), Q, z.data_ptr(),
                         part.data_ptr<float>(), (int)P, (int)Q, (int)K, cur_stream());
  }
  tbamd::colsum_finalize(dt_code(db), part.data_ptr<float>(), ntp, (int)Q, db.data_ptr(), cur_stream());
  return {y, db};
}

// --------------------------------------------- bias gradients / GELU
Tensor colsum_out(const Tensor& dy, const optional<Tensor>& out) {
  const int64_t C = dy.size(1);
  if (given(out)) {  // zero-copy gradient slot
    TORCH_CHECK(out->numel() == C && out->is_contiguous() && out->scalar_type() == dy.scalar_type(),
                "colsum: out must be a contiguous [C] tensor of dy's dtype");
    return *out;
  }
  return at::empty({C}, dy.options());
}

// dy: [M, C] -> [C] column sums (the bias gradient), in dy's dtype
Tensor colsum(const Tensor& dy_, const optional<Tensor>& out) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  TORCH_CHECK(dy_.dim() == 2 && dy_.size(1) % 8 == 0, "colsum: expected [M, C] with C % 8 == 0");
  Tensor dy = as_rows(dy_);
  const int64_t M = dy.size(0);
  const int C = (int)dy.size(1);
  Tensor o = colsum_out(dy, out);
  Tensor part = at::empty({(int64_t)tbamd::colsum_splits(M, C) * C}, dy.options().dtype(at::kFloat));
  tbamd::colsum(dt_code(dy), dy.data_ptr(), nullptr, nullptr, M, C, part.data_ptr<float>(), o.data_ptr(),
                cur_stream());
  return o;
}

// y = GELU(z) (exact erf) on a contiguous tensor with numel % 8 == 0
Tensor gelu_fwd(const Tensor& z_) {
  const at::DeviceGuard guard = on_device_of(z_, "z");
  Tensor z = z_.contiguous();
  TORCH_CHECK(z.numel() % 8 == 0, "gelu_fwd: numel must be a multiple of 8");
  Tensor y = at::empty_like(z);
  tbamd::gelu_forward(dt_code(z), z.data_ptr(), y.data_ptr(), z.numel(), cur_stream());
  return y;
}

// (dz = dy * GELU'(z), column sums of dz)
std::vector<Tensor> gelu_bwd_colsum(const Tensor& dy_, const Tensor& z_, const optional<Tensor>& out) {
  const at::DeviceGuard guard = on_device_of(dy_, "dy");
  TORCH_CHECK(dy_.dim() == 2 && dy_.size(1) % 8 == 0 && z_.sizes() == dy_.sizes(),
              "gelu_bwd_colsum: expected matching [M, C] with C % 8 == 0");
  Tensor z = as_rows(z_);
  Tensor dy = as_rows(dy_.to(z.scalar_type()));
  const int64_t M = dy.size(0);
  const int C = (int)dy.size(1);
  Tensor dz = at::empty_like(dy);
  Tensor o = colsum_out(dy, out);
  Tensor part = at::empty({(int64_t)tbamd::colsum_splits(M, C) * C}, dy.options().dtype(at::kFloat));
  tbamd::colsum(dt_code(dy), dy.data_ptr(), z.data_ptr(), dz.data_ptr(), M, C, part.data_ptr<float>(), o.data_ptr(),
                cur_stream());
  return {dz, o};
}

}  // namespace

void register_gemm(pybind11::module& m) {
  m.def("gemm", &gemm, py::arg("x"), py::arg("w"), py::arg("tw") = false, py::arg("bias") = py::none(),
        py::arg("residual") = py::none(), py::arg("epi") = 0, py::arg("want_z") = false, py::arg("tile") = -1,
        py::arg("out") = py::none(), py::arg("tx") = false, py::arg("splits") = 1);
  m.def("gemm_nn_gelu_bwd", &gemm_nn_gelu_bwd, py::arg("dy"), py::arg("w"), py::arg("z"),
        py::arg("db_out") = py::none(), py::arg("wt") = py::none());
  m.def("colsum", &colsum, py::arg("dy"), py::arg("out") = py::none());
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd_colsum", &gelu_bwd_colsum, py::arg("dy"), py::arg("z"), py::arg("out") = py::none());
  m.def("gemm_pick_splits", &tbamd::gemm_pick_splits);
  m.def("gemm8_set_stagger", &tbamd::gemm8_set_stagger);
  m.def("gemm_pick_tile", &tbamd::gemm_pick_tile);
  m.def("gemm_num_tiles", &tbamd::gemm_num_tiles);
}
