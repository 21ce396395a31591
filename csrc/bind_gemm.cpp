// Bindings of the dense GEMM kernels (gemm.hip, gemm8.hip, gemm_mx.hip), of the grouped GEMM (gemm_grouped.hip) and
// of the bias-gradient / GELU kernels that go with them (colsum.hip).
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
  if (epi == 2 && want_z) {
    // the kernels store z with y's row stride
    TORCH_CHECK(y.stride(0) == Q, "gemm: the saved pre-activation needs a contiguous out");
    z = at::empty({P, Q}, x.options());
  }
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

// y [P, Q] = epi(x @ dq(codes, scales)^T + bias) on an MXFP4 weight (gemm_mx.hip): x bf16 [P, K], codes uint8
// [Q, K / 2], scales uint8 [Q, K / 32], any P and Q, K % 32 == 0.  epi 0 (none), 1 (exact GELU) or
// 2 (+ residual [P, Q]).
Tensor gemm_mx(const Tensor& x, const Tensor& codes, const Tensor& scales, const optional<Tensor>& bias, int64_t epi,
               const optional<Tensor>& residual) {
  check_rows_bf16(x, "x");
  const at::DeviceGuard guard(x.device());
  check_cuda(codes, "codes");
  check_cuda(scales, "scales");
  TORCH_CHECK(codes.scalar_type() == at::kByte && scales.scalar_type() == at::kByte && codes.dim() == 2 &&
                  scales.dim() == 2 && codes.is_contiguous() && scales.is_contiguous() &&
                  codes.device() == x.device() && scales.device() == x.device(),
              "gemm_mx: codes [Q, K / 2] and scales [Q, K / 32] must be contiguous uint8 on the device of x");
  const int64_t P = x.size(0), K = x.size(1), Q = codes.size(0);
  TORCH_CHECK(K % 32 == 0 && K >= 32 && codes.size(1) * 2 == K && scales.size(0) == Q && scales.size(1) * 32 == K,
              "gemm_mx: K % 32 == 0, K >= 32, codes [Q, K / 2] and scales [Q, K / 32]");
  TORCH_CHECK(P >= 1 && Q >= 1 && P < (1ll << 31) - 256 && Q < (1ll << 31) - 256 && K < (1ll << 31) - 256 &&
                  ((P + 63) / 64) * ((Q + 31) / 32) < (1ll << 31),
              "gemm_mx: dims out of range");
  TORCH_CHECK(x.stride(0) >= K || P == 1, "gemm_mx: overlapping rows of x");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(codes.data_ptr()) % 16 == 0, "gemm_mx: codes must be 16-B aligned");
  TORCH_CHECK(epi >= 0 && epi <= 2, "gemm_mx: epilogue 0 (none), 1 (gelu) or 2 (residual)");
  tbamd::GemmMxArgs a{};
  a.X = reinterpret_cast<const uint16_t*>(x.data_ptr());
  a.codes = codes.data_ptr<uint8_t>();
  a.scales = scales.data_ptr<uint8_t>();
  a.ldx = x.stride(0);
  if (given(bias)) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kBFloat16 && bias->dim() == 1 && bias->size(0) == Q &&
                    bias->is_contiguous() && bias->device() == x.device(),
                "gemm_mx: bias must be contiguous bf16 [Q]");
    a.bias = reinterpret_cast<const uint16_t*>(bias->data_ptr());
  }
  TORCH_CHECK((epi == 2) == given(residual), "gemm_mx: a residual comes with epilogue 2 and only with it");
  if (given(residual)) {
    const Tensor& r = *residual;
    check_cuda(r, "residual");
    TORCH_CHECK(r.scalar_type() == at::kBFloat16 && r.dim() == 2 && r.size(0) == P && r.size(1) == Q &&
                    r.stride(1) == 1 && (P == 1 || r.stride(0) >= Q) && r.device() == x.device(),
                "gemm_mx: residual must be bf16 [P, Q] with a unit column stride");
    a.res = reinterpret_cast<const uint16_t*>(r.data_ptr());
    a.ldres = r.stride(0);
  }
  Tensor y = at::empty({P, Q}, x.options());
  a.Y = reinterpret_cast<uint16_t*>(y.data_ptr());
  a.P = (int)P, a.Q = (int)Q, a.K = (int)K, a.epi = (int)epi;
  tbamd::gemm_mx(a, cur_stream());
  return y;
}

// --------------------------------------------- grouped GEMM (gemm_grouped.hip)
void check_grouped(const Tensor& t, int64_t dim, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() == dim && t.is_contiguous(), "grouped gemm: ", name,
              " must be a contiguous ", dim, "-D bf16 tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "grouped gemm: ", name, " must be 16-B aligned");
}
int64_t check_offsets(const Tensor& offsets, const Tensor& like) {
  TORCH_CHECK(offsets.is_cuda() && offsets.device() == like.device() && offsets.scalar_type() == at::kInt &&
                  offsets.dim() == 1 && offsets.is_contiguous() && offsets.numel() >= 2,
              "grouped gemm: offsets must be a contiguous int32 [E + 1] tensor on the operands' device");
  return offsets.numel() - 1;
}

// y [R, Q] = x[r] @ w[e(r)]^T (tw false, w [E, Q, K]) or x[r] @ w[e(r)] (tw true, w [E, K, Q]); x [R, K];
// the rows of expert e are offsets[e] .. offsets[e + 1] - 1, rows of no expert come back zero
Tensor grouped_rows(const Tensor& x, const Tensor& w, const Tensor& offsets, bool tw) {
  check_grouped(x, 2, "x");
  check_grouped(w, 3, "w");
  const at::DeviceGuard guard(x.device());
  const int64_t E = check_offsets(offsets, x);
  const int64_t R = x.size(0), K = x.size(1), Q = tw ? w.size(2) : w.size(1);
  TORCH_CHECK(w.device() == x.device() && w.size(0) == E && (tw ? w.size(1) : w.size(2)) == K,
              "grouped gemm: w must be [E, ", tw ? "K, Q" : "Q, K", "] with E = offsets.numel() - 1");
  TORCH_CHECK(K % 8 == 0 && Q % 8 == 0, "grouped gemm: K and Q must be multiples of 8");
  TORCH_CHECK(R < (1ll << 31) - 65536 && Q < (1ll << 31) - 128 && K < (1ll << 31) - 64 && E < (1 << 20),
              "grouped gemm: dims too large");
  Tensor y = at::empty({R, Q}, x.options());
  tbamd::grouped_rows_bf16(x.data_ptr(), w.data_ptr(), tw, offsets.data_ptr<int>(), y.data_ptr(), (int)R, (int)E,
                           (int)Q, (int)K, cur_stream());
  return y;
}

// dw [E, P, Q]: dw[e] = dy[rows of e]^T @ x[rows of e]; dy [R, P], x [R, Q]
Tensor grouped_tn(const Tensor& dy, const Tensor& x, const Tensor& offsets, const optional<Tensor>& out) {
  check_grouped(dy, 2, "dy");
  check_grouped(x, 2, "x");
  const at::DeviceGuard guard(x.device());
  const int64_t E = check_offsets(offsets, x);
  const int64_t R = x.size(0), P = dy.size(1), Q = x.size(1);
  TORCH_CHECK(dy.device() == x.device() && dy.size(0) == R, "grouped gemm: dy and x must have the same rows");
  TORCH_CHECK(P % 8 == 0 && Q % 8 == 0, "grouped gemm: P and Q must be multiples of 8");
  TORCH_CHECK(R < (1ll << 31) - 65536 && Q < (1ll << 31) - 128 && P < (1ll << 31) - 128 && E < 65536,
              "grouped gemm: dims too large");
  Tensor dw;
  if (given(out)) {
    dw = *out;
    check_grouped(dw, 3, "out");
    TORCH_CHECK(dw.device() == x.device() && dw.size(0) == E && dw.size(1) == P && dw.size(2) == Q,
                "grouped gemm: out must be [E, P, Q]");
  } else {
    dw = at::empty({E, P, Q}, x.options());
  }
  tbamd::grouped_tn_bf16(dy.data_ptr(), x.data_ptr(), offsets.data_ptr<int>(), dw.data_ptr(), (int)R, (int)E, (int)P,
                         (int)Q, cur_stream());
  return dw;
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
  m.def("gemm_mx", &gemm_mx, py::arg("x"), py::arg("codes"), py::arg("scales"), py::arg("bias") = py::none(),
        py::arg("epi") = 0, py::arg("residual") = py::none());
  m.def("gemm_mx_tile_rows", [](int64_t P) {
    TORCH_CHECK(P >= 1 && P < (1ll << 31), "gemm_mx_tile_rows: bad P");
    return (int64_t)tbamd::gemm_mx_tile_rows((int)P);
  });
  m.def("gemm_nn_gelu_bwd", &gemm_nn_gelu_bwd, py::arg("dy"), py::arg("w"), py::arg("z"),
        py::arg("db_out") = py::none(), py::arg("wt") = py::none());
  m.def("grouped_rows", &grouped_rows, py::arg("x"), py::arg("w"), py::arg("offsets"), py::arg("tw") = false);
  m.def("grouped_tn", &grouped_tn, py::arg("dy"), py::arg("x"), py::arg("offsets"), py::arg("out") = py::none());
  m.def("colsum", &colsum,py::arg("dy"), py::arg("out") = py::none());
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd_colsum", &gelu_bwd_colsum, py::arg("dy"), py::arg("z"), py::arg("out") = py::none());
  m.def("gemm_pick_splits", &tbamd::gemm_pick_splits);
  m.def("gemm8_set_stagger", &tbamd::gemm8_set_stagger);
  m.def("gemm_pick_tile", &tbamd::gemm_pick_tile);
  m.def("gemm_num_tiles", &tbamd::gemm_num_tiles);
}
