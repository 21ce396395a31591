// Shared by the bind_*.cpp translation units: the argument checks, optional-tensor handling, conv
// geometry and weight packing that the Python bindings of the native library (_C) have in common.
//
// Tensors are validated in the bindings (device, dtype, contiguity, 16-B alignment for the
// vectorised paths), workspaces come from the PyTorch caching allocator, and every launch goes onto
// the caller's current HIP stream, so all ops are hipGraph-capturable.  The helpers here issue the
// ATen calls of the code they stand for, in its order: what a captured graph records does not depend
// on which helper a binding uses.
#pragma once

#include <utility>
#include <vector>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include "tbamd.h"

namespace tbbind {

using at::Tensor;
using c10::optional;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline int dt_code(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return tbamd::kF32;
    case at::kBFloat16: return tbamd::kBF16;
    case at::kHalf: return tbamd::kF16;
    default: TORCH_CHECK(false, "torchbooster_amd: unsupported dtype ", t.scalar_type());
  }
  return -1;
}

inline void check_cuda(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "torchbooster_amd: ", name, " must be a GPU tensor");
}

// how nearly every op starts: t must be on a GPU, and the op runs with t's device current
inline at::DeviceGuard on_device_of(const Tensor& t, const char* name) {
  check_cuda(t, name);
  return at::DeviceGuard(t.device());
}

// ---- optional tensors
inline bool given(const optional<Tensor>& t) { return t.has_value() && t->defined(); }

// the f32 contiguous copy of an optional parameter (bias, affine weight), or an undefined tensor
inline Tensor f32_or_undef(const optional<Tensor>& t) {
  return given(t) ? t->to(at::kFloat).contiguous() : Tensor();
}

// data pointer of a tensor that may be undefined
inline void* ptr_or_null(const Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }
inline float* f32_or_null(const Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

inline const float* fptr(const optional<Tensor>& t) {
  if (!given(t)) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous(), "expected contiguous f32 tensor");
  return t->data_ptr<float>();
}
inline float* fptr_mut(const optional<Tensor>& t) { return const_cast<float*>(fptr(t)); }

// [M, C] view requirement: contiguous, and 16-B aligned for the 8-wide path.
inline Tensor as_rows(const Tensor& t) {
  Tensor c = t.contiguous();
  if (reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 != 0) c = c.clone();
  return c;
}

inline Tensor nhwc(const Tensor& t) { return t.contiguous(at::MemoryFormat::ChannelsLast); }

// zero-copy gradient slot of an affine norm parameter ([C] f32 contiguous) or a new tensor
inline Tensor slot_or_new(const optional<Tensor>& o, int64_t C, const at::TensorOptions& fopt, const char* what) {
  if (given(o)) {
    TORCH_CHECK(o->scalar_type() == at::kFloat && o->numel() == C && o->is_contiguous(), what, ": gradient slot");
    return *o;
  }
  return at::empty({C}, fopt);
}

// ---- grouped-query attention: H query heads share Hkv key / value heads (query head h reads kv head
// h / (H / Hkv)).  kv_heads = 0 stands for heads; it is never inferred from a cache's shape.
inline int64_t kv_heads_of(int64_t heads, int64_t kv_heads, const char* what) {
  TORCH_CHECK(heads >= 1 && kv_heads >= 0, what, ": heads must be >= 1 and kv_heads >= 0");
  const int64_t hkv = kv_heads == 0 ? heads : kv_heads;
  TORCH_CHECK(heads % hkv == 0, what, ": kv_heads ", hkv, " must divide heads ", heads);
  return hkv;
}
// the cache of such a layer is [B, Hkv, cap, 64]
inline void check_kv_cache(const Tensor& cache, int64_t hkv, const char* what) {
  TORCH_CHECK(cache.dim() == 4 && cache.size(1) == hkv, what, ": cache must be [B, kv_heads = ", hkv, ", cap, 64]");
}
// ---- rolling cache (csrc/attn_ring.h): the cache [B, Hkv, R, 64] is a ring of R slots.  It needs a window
// 1 <= W <= R (W == R is a real window here, not "none"), and a call that appends T rows before its first
// query reads needs T <= R - W + 1.  Returns W.
inline int ring_window(int64_t window, int64_t R, int64_t T, const char* what) {
  TORCH_CHECK(window >= 1 && window <= R, what, ": a rolling cache needs a window in [1, rows = ", R, "], not ", window);
  TORCH_CHECK(T <= R - window + 1, what, ": ", T, " new rows need a ring of at least window + ", T - 1, " rows, not ", R);
  return (int)window;
}
// elements of a packed q | k | v row, head dim 64
inline int64_t packed_qkv_width(int64_t heads, int64_t hkv) { return (heads + 2 * hkv) * 64; }

// ---- conv geometry: x [N, C, H, W], weight [K, C, R, S], output [N, K, P, Q] over the virtual
// input pad(upsample_nearest(x, up)) (or, with dil > 1, x dilated by dil).  of() takes the sizes;
// window() adds P, Q and runs the checks the caller names, under the caller's op name.
struct ConvGeom {
  int N, C, H, W, K, R, S, P, Q;
  enum : unsigned { kReflectFits = 1, kNonEmpty = 2 };

  static ConvGeom of(const Tensor& x, int64_t K, int64_t R, int64_t S) {
    return {(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)K, (int)R, (int)S, 0, 0};
  }
  static ConvGeom of(const Tensor& x, const Tensor& w) { return of(x, w.size(0), w.size(2), w.size(3)); }
  // the weight-gradient side: K from dy [N, K, P, Q]
  static ConvGeom of(const Tensor& x, const Tensor& dy, int64_t R, int64_t S) { return of(x, dy.size(1), R, S); }

  ConvGeom& window(int64_t stride, int64_t pad, int64_t up, bool reflect, unsigned checks, const char* op,
                   int64_t dil = 1) {
    const int64_t Hv = dil > 1 ? (int64_t)(H - 1) * dil + 1 : H * up, Wv = dil > 1 ? (int64_t)(W - 1) * dil + 1 : W * up;
    if (checks & kReflectFits)
      TORCH_CHECK(!reflect || (pad < Hv && pad < Wv), op, ": reflect pad must be < input size");
    P = (int)((Hv + 2 * pad - R) / stride + 1);
    Q = (int)((Wv + 2 * pad - S) / stride + 1);
    if (checks & kNonEmpty) TORCH_CHECK(P > 0 && Q > 0, op, ": empty output");
    return *this;
  }
  int64_t NPQ() const { return (int64_t)N * P * Q; }
  bool fits(const Tensor& dy) const { return dy.size(0) == N && dy.size(2) == P && dy.size(3) == Q; }
};

// ---- weight packing
// w [K <= 16][R][S][C] (any strides) -> zero-padded contiguous [16, R, S, C] of the narrow kernels
inline Tensor pack_w16(const Tensor& krsc) {
  Tensor w16 = at::zeros({16, krsc.size(1), krsc.size(2), krsc.size(3)},
                         krsc.options().memory_format(at::MemoryFormat::Contiguous));
  w16.narrow(0, 0, krsc.size(0)).copy_(krsc);
  return w16;
}

// w [K, C, R, S] -> [K, 32 * KT] rows of the C*R*S reduction in (r, s, c) order, zero past C*R*S
inline Tensor pack_tiny(const Tensor& w) {
  const int64_t K = w.size(0), kred = w.size(1) * w.size(2) * w.size(3), KT = (kred + 31) / 32;
  Tensor wp = at::zeros({K, 32 * KT}, w.options().memory_format(at::MemoryFormat::Contiguous));
  wp.narrow(1, 0, kred).copy_(w.permute({0, 2, 3, 1}).reshape({K, kred}));
  return wp;
}

// (hi, lo) bf16 pair of an f32 tensor through ATen: hi = bf16(t), lo = bf16(t - hi)
inline std::pair<Tensor, Tensor> split_hi_lo(const Tensor& t) {
  Tensor hi = t.to(at::kBFloat16);
  return {hi, (t - hi.to(at::kFloat)).to(at::kBFloat16)};
}

}  // namespace tbbind
