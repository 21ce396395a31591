// Bindings of the attention kernels (attention.hip, attention_decode.hip, attention_extend.hip), of
// the rotary position embedding (rope.hip) and of the few-row decode products (rows_gemm.hip).
#include <cmath>

#include "bind_common.h"

namespace {
using namespace tbbind;

// the leading nd strides of a bf16 view into s (each a multiple of 8 elements unless its dim has
// size 1) and its 16-B aligned base pointer
const uint16_t* aligned_rows(const Tensor& t, int nd, int64_t* s, const char* what, const char* name) {
  for (int i = 0; i < nd; ++i) {
    TORCH_CHECK(t.stride(i) % 8 == 0 || t.size(i) == 1, what, ": ", name, " strides must be multiples of 8");
    s[i] = t.stride(i);
  }
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, what, ": ", name, " not 16-B aligned");
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}

// q, k, v (and dq, dk, dv, o, dout): [B, H, N, 64] bf16 views with a unit
// head-dim stride and 16-B aligned rows (any batch/head/token strides, so the
// packed qkv projection output is consumed and the packed dqkv written in place)
void attn_view(const Tensor& t, const char* name, int64_t B, int64_t H, int64_t N, const uint16_t** p, int64_t* s) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() == 4, "attention: ", name, " must be bf16 [B, H, N, D]");
  TORCH_CHECK(t.size(0) == B && t.size(1) == H && t.size(2) == N && t.size(3) == 64 && t.stride(3) == 1,
              "attention: ", name, " shape/stride mismatch (head dim 64, unit stride)");
  *p = aligned_rows(t, 3, s, "attention", name);
}

// the caller's f32 workspace (tests) when given, else `need` floats from the caching allocator
Tensor workspace_or_new(const optional<Tensor>& workspace, int64_t need, const Tensor& like, const char* what) {
  if (!given(workspace)) return need > 0 ? at::empty({need}, like.options().dtype(at::kFloat)) : Tensor();
  const Tensor& ws = *workspace;
  check_cuda(ws, "workspace");
  TORCH_CHECK(ws.scalar_type() == at::kFloat && ws.is_contiguous() && ws.numel() >= need &&
                  ws.device() == like.device() && reinterpret_cast<uintptr_t>(ws.data_ptr()) % 16 == 0,
              what, ": workspace must be contiguous, 16-B aligned f32 with at least ", need, " elements");
  return ws;
}

// The masks (self-attention; both optional): causal, and key_lengths = [B] int32 on q's device,
// contiguous -- keys j >= key_lengths[b] are hidden from every query of batch b.  The kernels read
// the lengths from device memory (no host sync, graph-capture safe) and clamp each into [1, N].
// window (0: none; needs causal): the sliding window of csrc/attention.hip.  One that can hide nothing
// (>= N) is no window: the same kernels as without it.
void attn_masks(tbamd::AttnArgs& a, const Tensor& q, int64_t B, bool causal, const optional<Tensor>& key_lengths,
                int64_t window) {
  TORCH_CHECK(window >= 0, "attention: window must be >= 1 (0: none)");
  TORCH_CHECK(window == 0 || causal, "attention: a window needs causal attention");
  a.causal = causal ? 1 : 0;
  a.window = window < a.N ? (int)window : 0;
  a.klen = nullptr;
  if (!given(key_lengths)) return;
  const Tensor& kl = *key_lengths;
  check_cuda(kl, "key_lengths");
  TORCH_CHECK(kl.scalar_type() == at::kInt, "attention: key_lengths must be int32");
  TORCH_CHECK(kl.device() == q.device(), "attention: key_lengths must be on the device of q");
  TORCH_CHECK(kl.dim() == 1 && kl.size(0) == B, "attention: key_lengths must have shape [B]");
  TORCH_CHECK(kl.is_contiguous(), "attention: key_lengths must be contiguous");
  a.klen = kl.data_ptr<int>();
}

// -> (o [B, N, H, 64] contiguous, lse [B, H, N] f32)
std::vector<Tensor> attn_forward(const Tensor& q, const Tensor& k, const Tensor& v, double scale, bool causal,
                                 const optional<Tensor>& key_lengths, int64_t window) {
  const at::DeviceGuard guard(q.device());
  const int64_t B = q.size(0), H = q.size(1), N = q.size(2);
  TORCH_CHECK(N >= 1 && B * H * ((N + 127) / 128) < (int64_t)INT32_MAX, "attention: bad size");
  tbamd::AttnArgs a{};
  attn_view(q, "q", B, H, N, &a.q, a.sq);
  attn_view(k, "k", B, H, N, &a.k, a.sk);
  attn_view(v, "v", B, H, N, &a.v, a.sv);
  Tensor o = at::empty({B, N, H, 64}, q.options());
  Tensor lse = at::empty({B, H, N}, q.options().dtype(at::kFloat));
  Tensor ov = o.permute({0, 2, 1, 3});
  const uint16_t* op;
  attn_view(ov, "o", B, H, N, &op, a.so);
  a.o = const_cast<uint16_t*>(op);
  a.lse = lse.data_ptr<float>();
  a.B = (int)B, a.H = (int)H, a.N = (int)N, a.scale = (float)scale;
  attn_masks(a, q, B, causal, key_lengths, window);
  tbamd::attn_fwd(a, cur_stream());
  return {o, lse};
}

// writes dq, dk, dv (views, e.g. slices of one packed dqkv buffer)
void attn_backward(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o, const Tensor& dout,
                   const Tensor& lse, double scale, const Tensor& dq, const Tensor& dk, const Tensor& dv, bool causal,
                   const optional<Tensor>& key_lengths, int64_t window) {
  const at::DeviceGuard guard(q.device());
  const int64_t B = q.size(0), H = q.size(1), N = q.size(2);
  tbamd::AttnArgs a{};
  attn_view(q, "q", B, H, N, &a.q, a.sq);
  attn_view(k, "k", B, H, N, &a.k, a.sk);
  attn_view(v, "v", B, H, N, &a.v, a.sv);
  const uint16_t* p;
  attn_view(o, "o", B, H, N, &p, a.so);
  a.o = const_cast<uint16_t*>(p);
  attn_view(dout, "dout", B, H, N, &a.dout, a.sdo);
  attn_view(dq, "dq", B, H, N, &p, a.sdq);
  a.dq = const_cast<uint16_t*>(p);
  attn_view(dk, "dk", B, H, N, &p, a.sdk);
  a.dk = const_cast<uint16_t*>(p);
  attn_view(dv, "dv", B, H, N, &p, a.sdv);
  a.dv = const_cast<uint16_t*>(p);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.numel() == B * H * N, "attention: lse");
  Tensor delta = at::empty({B, H, N}, lse.options());
  a.lse = lse.data_ptr<float>();
  a.delta = delta.data_ptr<float>();
  a.B = (int)B, a.H = (int)H, a.N = (int)N, a.scale = (float)scale;
  attn_masks(a, q, B, causal, key_lengths, window);
  tbamd::attn_bwd(a, cur_stream());
}

// ---- KV-cache decoding (csrc/attention_decode.hip).  Cache: [B, Hkv, cap, 64] bf16 views (checked as
// attn_view checks q/k/v); lengths / positions: [B] int32 on the same device, read by the kernels.
// kv_heads (trailing, 0 = heads) is grouped-query attention: it must divide heads, the cache must
// have that many heads and a packed row is (H + 2*Hkv)*64 wide (bind_common.h).  window (trailing, 0 =
// none): the sliding window of the decode / extend kernels; one that can hide nothing (>= cap) is none.
// k_scale / v_scale (trailing, 1.0): the scales of an fp8 cache pair -- both caches float8_e4m3fn (csrc/attn_fp8.h);
// with bf16 caches they must stay 1.0.  The workspaces and the grids do not depend on the cache's type.
// rolling (trailing, false = the linear cache): the cache is a ring (bind_common.h ring_window): the window
// is required, kept as given, and lengths / positions are not clamped to the cache's rows.
// A cache tensor of a decode / extend call: bf16 (attn_view) or, with fp8, float8_e4m3fn codes [B, Hkv, cap, 64]
// with a unit last stride, the other strides multiples of 16 bytes and a 16-B aligned base (the conditions of
// attn_view, in bytes).  The strides returned count elements of the cache's own type.
void cache_view(const Tensor& t, const char* name, int64_t B, int64_t H, int64_t N, bool fp8, const uint16_t** p,
                int64_t* s) {
  if (!fp8) return attn_view(t, name, B, H, N, p, s);
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat8_e4m3fn && t.dim() == 4, "attention: ", name,
              " must be float8_e4m3fn [B, H, N, D] like the other cache");
  TORCH_CHECK(t.size(0) == B && t.size(1) == H && t.size(2) == N && t.size(3) == 64 && t.stride(3) == 1,
              "attention: ", name, " shape/stride mismatch (head dim 64, unit stride)");
  for (int i = 0; i < 3; ++i) {
    TORCH_CHECK(t.stride(i) % 16 == 0 || t.size(i) == 1, "attention: ", name, " strides must be multiples of 16");
    s[i] = t.stride(i);
  }
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "attention: ", name, " not 16-B aligned");
  *p = reinterpret_cast<const uint16_t*>(t.data_ptr());
}

// Is the cache pair fp8?  Both float8_e4m3fn: yes, and the two scales must be finite and > 0; otherwise the
// scales must be the defaults (a bf16 pair has none) and attn_view rejects anything that is not bf16.
bool cache_fp8(const Tensor& k_cache, const Tensor& v_cache, double k_scale, double v_scale, const char* what) {
  const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn && v_cache.scalar_type() == at::kFloat8_e4m3fn;
  if (fp8) {
    TORCH_CHECK(std::isfinite(k_scale) && k_scale > 0 && std::isfinite(v_scale) && v_scale > 0, what,
                ": the scales of an fp8 cache must be finite and > 0");
  } else {
    TORCH_CHECK(k_scale == 1.0 && v_scale == 1.0, what, ": k_scale / v_scale need float8_e4m3fn caches");
  }
  return fp8;
}

int cache_window(int64_t window, int64_t cap, const char* what) {
  TORCH_CHECK(window >= 0, what, ": window must be >= 1 (0: none)");
  return window < cap ? (int)window : 0;
}

const int* decode_lengths(const Tensor& t, const char* name, const Tensor& like, int64_t B) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kInt, "attention decode: ", name, " must be int32");
  TORCH_CHECK(t.device() == like.device(), "attention decode: ", name, " must be on the device of the cache");
  TORCH_CHECK(t.dim() == 1 && t.size(0) == B, "attention decode: ", name, " must have shape [B]");
  TORCH_CHECK(t.is_contiguous(), "attention decode: ", name, " must be contiguous");
  return t.data_ptr<int>();
}

// packed [B, T, (H + 2*Hkv)*64] bf16: unit last stride, batch / token strides multiples of 8, 16-B aligned
const uint16_t* packed_qkv(const Tensor& t, int64_t B, int64_t H, int64_t Hkv, const Tensor& like, int64_t* s) {
  check_cuda(t, "qkv");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() == 3,
              "attention decode: qkv must be bf16 [B, T, (H + 2*Hkv)*64]");
  TORCH_CHECK(t.size(0) == B && t.size(2) == packed_qkv_width(H, Hkv) && t.stride(2) == 1,
              "attention decode: qkv shape/stride mismatch (head dim 64, unit stride)");
  TORCH_CHECK(t.device() == like.device(), "attention decode: qkv must be on the device of the cache");
  return aligned_rows(t, 2, s, "attention decode", "qkv");
}

void attn_kv_append(const Tensor& qkv, int64_t heads, const Tensor& k_cache, const Tensor& v_cache,
                    const Tensor& positions, int64_t kv_heads, bool rolling, const optional<Tensor>& lengths,
                    double k_scale, double v_scale) {
  const at::DeviceGuard guard(k_cache.device());
  const bool fp8 = cache_fp8(k_cache, v_cache, k_scale, v_scale, "attention decode");
  TORCH_CHECK(rolling || !given(lengths), "attention decode: append lengths need a rolling cache");
  const int64_t Hkv = kv_heads_of(heads, kv_heads, "attention decode");
  check_kv_cache(k_cache, Hkv, "attention decode");
  const int64_t B = k_cache.size(0), H = heads, cap = k_cache.size(2);
  TORCH_CHECK(qkv.dim() == 3, "attention decode: qkv must be bf16 [B, T, (H + 2*Hkv)*64]");
  const int64_t T = qkv.size(1);
  TORCH_CHECK(B >= 1 && cap >= 1 && T >= 0 && B * T * H < (int64_t)1 << 34 && cap < (int64_t)INT32_MAX,
              "attention decode: bad size");
  tbamd::AttnAppendArgs a{};
  a.qkv = packed_qkv(qkv, B, H, Hkv, k_cache, a.sqkv);
  const uint16_t* p;
  cache_view(k_cache, "k_cache", B, Hkv, cap, fp8, &p, a.sk);
  a.kc = const_cast<uint16_t*>(p);
  cache_view(v_cache, "v_cache", B, Hkv, cap, fp8, &p, a.sv);
  a.vc = const_cast<uint16_t*>(p);
  if (fp8) a.fp8 = 1, a.kinv = (float)(1.0 / k_scale), a.vinv = (float)(1.0 / v_scale);
  TORCH_CHECK(v_cache.device() == k_cache.device(), "attention decode: caches on different devices");
  a.pos = decode_lengths(positions, "positions", k_cache, B);
  a.B = (int)B, a.T = (int)T, a.H = (int)H, a.Hkv = (int)Hkv, a.cap = (int)cap;
  a.ring = rolling ? 1 : 0;
  if (given(lengths)) a.len = decode_lengths(*lengths, "lengths", k_cache, B);
  TORCH_CHECK(!rolling || T < (int64_t)INT32_MAX / 2, "attention decode: bad size");
  tbamd::attn_kv_append(a, cur_stream());
}

// What attn_decode and attn_decode_append share of AttnDecodeArgs: the cache views, the size checks, the
// lengths and the output o [B, H*64], which is returned.  qkv: the packed [B, 1, (H + 2*Hkv)*64] whose q
// part is read in place (a.sq[0] is its batch stride); null leaves a.q / a.sq to the caller.  a.ws too.
Tensor decode_args(tbamd::AttnDecodeArgs& a, const Tensor* qkv, int64_t H, int64_t Hkv, const Tensor& k_cache,
                   const Tensor& v_cache, const Tensor& lengths, const char* lengths_name, int64_t add, double scale,
                   double k_scale, double v_scale) {
  check_kv_cache(k_cache, Hkv, "attention decode");
  const bool fp8 = cache_fp8(k_cache, v_cache, k_scale, v_scale, "attention decode");
  const int64_t B = k_cache.size(0), cap = k_cache.size(2);
  TORCH_CHECK(B >= 1 && cap >= 1 && cap < (int64_t)INT32_MAX / 2 && add >= -cap && add <= cap,
              "attention decode: bad size");
  TORCH_CHECK(B * H * (int64_t)tbamd::attn_decode_chunks((int)cap) < (int64_t)INT32_MAX / 64,
              "attention decode: bad size");
  if (qkv != nullptr) {
    TORCH_CHECK(qkv->dim() == 3 && qkv->size(1) == 1, "attention decode: qkv must be bf16 [B, 1, (H + 2*Hkv)*64]");
    a.q = packed_qkv(*qkv, B, H, Hkv, k_cache, a.sq);
    a.sq[1] = 64;  // from head to head, not packed_qkv's token stride
  }
  cache_view(k_cache, "k_cache", B, Hkv, cap, fp8, &a.k, a.sk);
  cache_view(v_cache, "v_cache", B, Hkv, cap, fp8, &a.v, a.sv);
  TORCH_CHECK(v_cache.device() == k_cache.device(), "attention decode: caches on different devices");
  a.klen = decode_lengths(lengths, lengths_name, k_cache, B);
  Tensor o = at::empty({B, H * 64}, k_cache.options().dtype(at::kBFloat16));
  a.o = reinterpret_cast<uint16_t*>(o.data_ptr());
  a.so[0] = H * 64, a.so[1] = 64;
  a.B = (int)B, a.H = (int)H, a.Hkv = (int)Hkv, a.cap = (int)cap, a.add = (int)add, a.scale = (float)scale;
  if (fp8) {  // k_scale rides in the score factor: one f32 product here
    a.fp8 = 1, a.scale = (float)scale * (float)k_scale, a.vscale = (float)v_scale;
    a.kinv = (float)(1.0 / k_scale), a.vinv = (float)(1.0 / v_scale);
  }
  return o;
}

// q: [B, H, 64] (any batch / head strides) or the packed [B, 1, (H + 2*Hkv)*64] whose q part is read in
// place -> o [B, H*64].  len = clamp(lengths[b] + add, 1, cap).  workspace (optional, tests): f32,
// at least attn_decode_workspace floats; by default it comes from the caching allocator.
Tensor attn_decode(const Tensor& q, int64_t heads, const Tensor& k_cache, const Tensor& v_cache, const Tensor& lengths,
                   int64_t add, double scale, const optional<Tensor>& workspace, int64_t kv_heads, int64_t window,
                   bool rolling, double k_scale, double v_scale) {
  const at::DeviceGuard guard(k_cache.device());
  const int64_t H = heads, Hkv = kv_heads_of(heads, kv_heads, "attention decode");
  const bool packed = q.dim() == 3 && q.size(1) == 1 && q.size(2) == packed_qkv_width(H, Hkv);
  tbamd::AttnDecodeArgs a{};
  Tensor o = decode_args(a, packed ? &q : nullptr, H, Hkv, k_cache, v_cache, lengths, "lengths", add, scale, k_scale,
                         v_scale);
  if (!packed) {
    check_cuda(q, "q");
    TORCH_CHECK(q.scalar_type() == at::kBFloat16 && q.dim() == 3 && q.size(0) == a.B && q.size(1) == H &&
                    q.size(2) == 64 && q.stride(2) == 1,
                "attention decode: q must be bf16 [B, H, 64] with a unit head-dim stride (or packed [B, 1, (H + 2*Hkv)*64])");
    TORCH_CHECK(q.device() == k_cache.device(), "attention decode: q must be on the device of the cache");
    a.q = aligned_rows(q, 2, a.sq, "attention decode", "q");
  }
  Tensor ws = workspace_or_new(workspace, tbamd::attn_decode_workspace(a.B, a.H, a.cap), k_cache, "attention decode");
  a.ws = ws.data_ptr<float>();
  a.ring = rolling ? 1 : 0;
  a.window = rolling ? ring_window(window, a.cap, 1, "attention decode") : cache_window(window, a.cap, "attention decode");
  tbamd::attn_decode(a, cur_stream());
  return o;
}

// One decode step with the append folded in: qkv packed [B, 1, (H + 2*Hkv)*64]; the k / v of the token go to
// cache row positions[b] (dropped outside [0, cap)) and the query sees rows j <= positions[b] ->
// o [B, H*64].  Same bits, output and caches, as attn_kv_append followed by attn_decode(add = 1).
Tensor attn_decode_append(const Tensor& qkv, int64_t heads, const Tensor& k_cache, const Tensor& v_cache,
                          const Tensor& positions, double scale, int64_t kv_heads, int64_t window, bool rolling,
                          double k_scale, double v_scale) {
  const at::DeviceGuard guard(k_cache.device());
  const int64_t H = heads, Hkv = kv_heads_of(heads, kv_heads, "attention decode");
  tbamd::AttnDecodeArgs a{};
  Tensor o = decode_args(a, &qkv, H, Hkv, k_cache, v_cache, positions, "positions", 1, scale, k_scale, v_scale);
  a.ring = rolling ? 1 : 0;
  a.window = rolling ? ring_window(window, a.cap, 1, "attention decode") : cache_window(window, a.cap, "attention decode");
  Tensor ws;  // a single chunk is normalised in the split kernel: no partials
  if (tbamd::attn_decode_chunks(a.cap) > 1) {
    ws = at::empty({tbamd::attn_decode_workspace(a.B, a.H, a.cap)}, k_cache.options().dtype(at::kFloat));
    a.ws = ws.data_ptr<float>();
  }
  tbamd::attn_decode_append(a, a.q + H * 64, a.q + (H + Hkv) * 64, a.sq[0], cur_stream());
  return o;
}

// ------------------------------------------------------------ few-row products (csrc/rows_gemm.hip)
// x [M, K] bf16 (1 <= M <= 16, unit column stride, row stride a multiple of 8) . weight [Q, K]^T ->
// [M, Q].  gamma / beta: f32 [K] LayerNorm prologue (both or neither); rms: gamma alone, the RMSNorm
// prologue; epi: 0 none, 1 GELU, 2 + residual [M, Q], 3 SwiGLU (weight [2Q, K] gate | up rows, bias
// [2Q], result [M, Q]).  out (optional, tests): contiguous bf16 [M, Q] written instead of a fresh tensor.
Tensor rows_linear(const Tensor& x, const Tensor& weight, const optional<Tensor>& bias, const optional<Tensor>& gamma,
                   const optional<Tensor>& beta, double eps, int64_t epi, const optional<Tensor>& residual,
                   const optional<Tensor>& out, bool rms) {
  const at::DeviceGuard guard = on_device_of(x, "x");
  check_cuda(weight, "weight");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && weight.scalar_type() == at::kBFloat16, "rows_linear: bf16 only");
  TORCH_CHECK(x.dim() == 2 && weight.dim() == 2 && weight.is_contiguous() && weight.device() == x.device(),
              "rows_linear: x [M, K], weight [Q, K] contiguous, on one device");
  TORCH_CHECK(epi >= 0 && epi <= 3, "rows_linear: epilogue 0 (none), 1 (gelu), 2 (residual) or 3 (swiglu)");
  const bool glu = epi == tbamd::kRowsSwiglu;
  TORCH_CHECK(!glu || weight.size(0) % 2 == 0, "rows_linear: the swiglu epilogue needs weight [2F, K]");
  const int64_t M = x.size(0), K = x.size(1), WQ = weight.size(0), Q = glu ? WQ / 2 : WQ;
  TORCH_CHECK(M >= 1 && M <= 16 && K % 8 == 0 && K >= 8 && K <= 4096 && weight.size(1) == K && Q >= 1 &&
                  Q < (int64_t)INT32_MAX / 16,
              "rows_linear: 1 <= M <= 16, K % 8 == 0, K <= 4096");
  TORCH_CHECK(x.stride(1) == 1 && (M == 1 || x.stride(0) % 8 == 0) && (M == 1 || x.stride(0) >= 0) &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(weight.data_ptr()) % 16 == 0,
              "rows_linear: rows must be 16-B aligned with a unit column stride");
  tbamd::RowsLinearArgs a{};
  a.x = reinterpret_cast<const uint16_t*>(x.data_ptr());
  a.w = reinterpret_cast<const uint16_t*>(weight.data_ptr());
  a.sx = M == 1 ? 0 : x.stride(0);
  if (given(bias)) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kBFloat16 && bias->dim() == 1 && bias->size(0) == WQ &&
                    bias->is_contiguous() && bias->device() == x.device(),
                "rows_linear: bias must be contiguous bf16 [Q] ([2F] under swiglu)");
    a.bias = reinterpret_cast<const uint16_t*>(bias->data_ptr());
  }
  const bool ln = given(gamma);
  TORCH_CHECK(rms ? (ln && !given(beta)) : ln == given(beta),
              "rows_linear: gamma and beta come together (LayerNorm), or gamma alone with rms");
  if (rms) {
    const Tensor* t = &*gamma;
    check_cuda(*t, "gamma");
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->dim() == 1 && t->size(0) == K && t->is_contiguous() &&
                    t->device() == x.device() && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "rows_linear: gamma must be contiguous, 16-B aligned f32 [K]");
    a.gamma = gamma->data_ptr<float>();
    a.rms = 1;
  } else if (ln) {
    for (const Tensor* t : {&*gamma, &*beta}) {
      check_cuda(*t, "gamma / beta");
      TORCH_CHECK(t->scalar_type() == at::kFloat && t->dim() == 1 && t->size(0) == K && t->is_contiguous() &&
                      t->device() == x.device() && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                  "rows_linear: gamma / beta must be contiguous, 16-B aligned f32 [K]");
    }
    a.gamma = gamma->data_ptr<float>();
    a.beta = beta->data_ptr<float>();
  }
  Tensor y;
  if (given(out)) {
    y = *out;
    check_cuda(y, "out");
    TORCH_CHECK(y.scalar_type() == at::kBFloat16 && y.dim() == 2 && y.size(0) == M && y.size(1) == Q &&
                    y.is_contiguous() && y.device() == x.device(),
                "rows_linear: out must be contiguous bf16 [M, Q]");
  } else {
    y = at::empty({M, Q}, x.options());
  }
  TORCH_CHECK(!glu || !given(residual), "rows_linear: the swiglu epilogue takes no residual");
  if (epi == 2) {
    TORCH_CHECK(given(residual), "rows_linear: the residual epilogue needs a residual");
    const Tensor& r = *residual;
    check_cuda(r, "residual");
    TORCH_CHECK(r.scalar_type() == at::kBFloat16 && r.dim() == 2 && r.size(0) == M && r.size(1) == Q &&
                    r.stride(1) == 1 && (M == 1 || r.stride(0) >= 0) && r.device() == x.device(),
                "rows_linear: residual must be bf16 [M, Q] with a unit column stride");
    a.res = reinterpret_cast<const uint16_t*>(r.data_ptr());
    a.sres = M == 1 ? 0 : r.stride(0);
  }
  a.y = reinterpret_cast<uint16_t*>(y.data_ptr());
  a.M = (int)M, a.K = (int)K, a.Q = (int)Q, a.epi = (int)epi, a.eps = (float)eps;
  tbamd::rows_linear(a, cur_stream());
  return y;
}

// tokens int64 [B, T] (any strides); tok_weight [vocab, D], pos_weight [max_len, D] bf16 contiguous; positions
// int32 [B] or none -> [B, T, D].  Token ids and positions are clamped into range by the kernel.
// pos_weight none: the clamped token rows alone.
Tensor embed_rows(const Tensor& tokens, const Tensor& tok_weight, const optional<Tensor>& pos_weight,
                  const optional<Tensor>& positions) {
  const at::DeviceGuard guard = on_device_of(tok_weight, "tok_weight");
  check_cuda(tokens, "tokens");
  TORCH_CHECK(tokens.scalar_type() == at::kLong && tokens.dim() == 2 && tokens.device() == tok_weight.device(),
              "embed_rows: tokens must be int64 [B, T] on the device of the weights");
  TORCH_CHECK(tok_weight.scalar_type() == at::kBFloat16 && tok_weight.dim() == 2 && tok_weight.is_contiguous(),
              "embed_rows: weights must be contiguous bf16 [vocab, D] and [max_len, D]");
  const int64_t B = tokens.size(0), T = tokens.size(1), D = tok_weight.size(1);
  TORCH_CHECK(D % 8 == 0 && D >= 8 && tok_weight.size(0) >= 1 && tok_weight.size(0) < (int64_t)INT32_MAX &&
                  D < (int64_t)INT32_MAX && B * T < (int64_t)INT32_MAX,
              "embed_rows: D % 8 == 0; bad size");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(tok_weight.data_ptr()) % 16 == 0, "embed_rows: weights not 16-B aligned");
  tbamd::EmbedRowsArgs a{};
  a.max_len = 1;
  if (given(pos_weight)) {
    const Tensor& pw = *pos_weight;
    check_cuda(pw, "pos_weight");
    TORCH_CHECK(pw.scalar_type() == at::kBFloat16 && pw.dim() == 2 && pw.is_contiguous() && pw.size(1) == D &&
                    pw.device() == tok_weight.device(),
                "embed_rows: weights must be contiguous bf16 [vocab, D] and [max_len, D]");
    TORCH_CHECK(pw.size(0) >= 1 && pw.size(0) < (int64_t)INT32_MAX, "embed_rows: D % 8 == 0; bad size");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(pw.data_ptr()) % 16 == 0, "embed_rows: weights not 16-B aligned");
    a.pos_w = reinterpret_cast<const uint16_t*>(pw.data_ptr());
    a.max_len = (int)pw.size(0);
  }
  if (given(positions)) a.pos = decode_lengths(*positions, "positions", tok_weight, B);
  Tensor y = at::empty({B, T, D}, tok_weight.options());
  a.tokens = tokens.data_ptr<int64_t>();
  a.stok[0] = tokens.stride(0), a.stok[1] = tokens.stride(1);
  a.tok_w = reinterpret_cast<const uint16_t*>(tok_weight.data_ptr());
  a.y = reinterpret_cast<uint16_t*>(y.data_ptr());
  a.B = (int)B, a.T = (int)T, a.D = (int)D, a.vocab = (int)tok_weight.size(0);
  tbamd::embed_rows(a, cur_stream());
  return y;
}

// ---- rotary position embedding (csrc/rope.hip).  qkv: packed [B, T, (H + 2*Hkv)*64] bf16 (checked as
// the decode kernels' qkv); table: f32 [max_len, 2, 32] contiguous on the same device; positions: int32
// [B] or none, read by the kernel.  out none -> a new contiguous tensor, value part copied; out given
// -> it must BE qkv (in place: the value part is not touched).  Returns the output.
Tensor rope_packed(const Tensor& qkv, int64_t heads, const Tensor& table, const optional<Tensor>& positions,
                   int64_t kv_heads, bool inverse, const optional<Tensor>& out) {
  const at::DeviceGuard guard = on_device_of(qkv, "qkv");
  const int64_t Hkv = kv_heads_of(heads, kv_heads, "rope");
  TORCH_CHECK(qkv.dim() == 3, "rope: qkv must be bf16 [B, T, (H + 2*Hkv)*64]");
  const int64_t B = qkv.size(0), T = qkv.size(1), H = heads;
  TORCH_CHECK(B * T * (H + 2 * Hkv) < (int64_t)1 << 34 && B < (int64_t)INT32_MAX && T < (int64_t)INT32_MAX &&
                  H + 2 * Hkv < (int64_t)1 << 20,
              "rope: bad size");
  check_cuda(table, "table");
  TORCH_CHECK(table.scalar_type() == at::kFloat && table.dim() == 3 && table.size(1) == 2 && table.size(2) == 32 &&
                  table.is_contiguous() && table.size(0) >= 1 && table.size(0) < (int64_t)INT32_MAX / 64 &&
                  table.device() == qkv.device(),
              "rope: table must be contiguous f32 [max_len, 2, 32] on the device of qkv");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(table.data_ptr()) % 16 == 0, "rope: table not 16-B aligned");
  tbamd::RopeArgs a{};
  a.x = packed_qkv(qkv, B, H, Hkv, qkv, a.sx);
  Tensor y;
  if (given(out)) {
    TORCH_CHECK(out->is_same(qkv), "rope: out must be qkv itself (in place)");
    y = *out;
    a.sy[0] = a.sx[0], a.sy[1] = a.sx[1];
    a.copy_v = 0;
  } else {
    y = at::empty({B, T, qkv.size(2)}, qkv.options().memory_format(at::MemoryFormat::Contiguous));
    a.sy[0] = T * qkv.size(2), a.sy[1] = qkv.size(2);
    a.copy_v = 1;
  }
  a.y = reinterpret_cast<uint16_t*>(y.data_ptr());
  a.tab = table.data_ptr<float>();
  if (given(positions)) a.pos = decode_lengths(*positions, "positions", qkv, B);
  a.B = (int)B, a.T = (int)T, a.H = (int)H, a.Hkv = (int)Hkv, a.max_len = (int)table.size(0);
  a.inverse = inverse ? 1 : 0;
  tbamd::rope_packed(a, cur_stream());
  return y;
}

// q: [B, T, H, 64] (any batch / token / head strides; the q part of a packed [B, T, (H + 2*Hkv)*64] is
// such a view) -> o [B, T, H*64].  H is q's; the caches hold kv_heads (0 = H) heads.  Query t sees cache rows j < clamp(positions[b] + t + 1, 1, cap).
// workspace (optional, tests): f32, at least attn_extend_workspace floats; by default it comes
// from the caching allocator (none at all with a single key split).
Tensor attn_extend(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& positions,
                   double scale, const optional<Tensor>& workspace, int64_t kv_heads, int64_t window, bool rolling,
                   double k_scale, double v_scale) {
  const at::DeviceGuard guard(k_cache.device());
  TORCH_CHECK(k_cache.dim() == 4, "attention extend: cache must be [B, H, cap, 64]");
  const bool fp8 = cache_fp8(k_cache, v_cache, k_scale, v_scale, "attention extend");
  const int64_t B = k_cache.size(0), cap = k_cache.size(2);
  check_cuda(q, "q");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 && q.dim() == 4 && q.size(0) == B && q.size(2) >= 1 &&
                  q.size(3) == 64 && q.stride(3) == 1,
              "attention extend: q must be bf16 [B, T, H, 64] with a unit head-dim stride");
  const int64_t H = q.size(2);
  const int64_t Hkv = kv_heads_of(H, kv_heads, "attention extend");
  check_kv_cache(k_cache, Hkv, "attention extend");
  const int64_t T = q.size(1);
  TORCH_CHECK(B >= 1 && H >= 1 && T >= 1 && cap >= 1 && cap < (int64_t)INT32_MAX / 2 && T < (int64_t)INT32_MAX / 2,
              "attention extend: bad size");
  TORCH_CHECK(q.device() == k_cache.device(), "attention extend: q must be on the device of the cache");
  tbamd::AttnExtendArgs a{};
  a.q = aligned_rows(q, 3, a.sq, "attention extend", "q");
  cache_view(k_cache, "k_cache", B, Hkv, cap, fp8, &a.k, a.sk);
  cache_view(v_cache, "v_cache", B, Hkv, cap, fp8, &a.v, a.sv);
  TORCH_CHECK(v_cache.device() == k_cache.device(), "attention extend: caches on different devices");
  a.pos = decode_lengths(positions, "positions", k_cache, B);
  // the split kernel's grid (one workgroup per partial) and the merge kernel's (one per output row)
  const int64_t nqt = (T + 15) / 16;
  TORCH_CHECK(B * H * nqt * (int64_t)tbamd::attn_extend_splits((int)B, (int)H, (int)T, (int)cap) <
                      (int64_t)INT32_MAX / (16 * 66) &&
                  B * T * H < (int64_t)INT32_MAX / 64,
              "attention extend: bad size");
  const int64_t need = tbamd::attn_extend_workspace((int)B, (int)H, (int)T, (int)cap);
  Tensor ws = workspace_or_new(workspace, need, k_cache, "attention extend");
  Tensor o = at::empty({B, T, H * 64}, k_cache.options().dtype(at::kBFloat16));
  a.o = reinterpret_cast<uint16_t*>(o.data_ptr());
  a.so[0] = T * H * 64, a.so[1] = H * 64;
  a.ws = need > 0 ? ws.data_ptr<float>() : nullptr;
  a.B = (int)B, a.T = (int)T, a.H = (int)H, a.Hkv = (int)Hkv, a.cap = (int)cap, a.scale = (float)scale;
  if (fp8) a.fp8 = 1, a.scale = (float)scale * (float)k_scale, a.vscale = (float)v_scale;
  a.ring = rolling ? 1 : 0;
  a.window = rolling ? ring_window(window, cap, T, "attention extend") : cache_window(window, cap, "attention extend");
  tbamd::attn_extend(a, cur_stream());
  return o;
}

}  // namespace

void register_attn(pybind11::module& m) {
  m.def("attn_forward", &attn_forward, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("causal") = false, py::arg("key_lengths") = py::none(), py::arg("window") = 0);
  m.def("attn_backward", &attn_backward, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("dout"),
        py::arg("lse"), py::arg("scale"), py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("causal") = false,
        py::arg("key_lengths") = py::none(), py::arg("window") = 0);
  m.def("attn_kv_append", &attn_kv_append, py::arg("qkv"), py::arg("heads"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("positions"), py::arg("kv_heads") = 0, py::arg("rolling") = false, py::arg("lengths") = py::none(),
        py::arg("k_scale") = 1.0, py::arg("v_scale") = 1.0);
  m.def("attn_decode", &attn_decode, py::arg("q"), py::arg("heads"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("lengths"), py::arg("add"), py::arg("scale"), py::arg("workspace") = py::none(),
        py::arg("kv_heads") = 0, py::arg("window") = 0, py::arg("rolling") = false, py::arg("k_scale") = 1.0,
        py::arg("v_scale") = 1.0);
  m.def("attn_decode_append", &attn_decode_append, py::arg("qkv"), py::arg("heads"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("positions"), py::arg("scale"), py::arg("kv_heads") = 0, py::arg("window") = 0,
        py::arg("rolling") = false, py::arg("k_scale") = 1.0, py::arg("v_scale") = 1.0);
  m.def("rows_linear", &rows_linear, py::arg("x"), py::arg("weight"), py::arg("bias") = py::none(),
        py::arg("gamma") = py::none(), py::arg("beta") = py::none(), py::arg("eps") = 0.0, py::arg("epi") = 0,
        py::arg("residual") = py::none(), py::arg("out") = py::none(), py::arg("rms") = false);
  // test helper (tests/test_gpu_llama_block.py checks that its shapes reach every launcher setting)
  m.def("rows_swiglu_cols_per_wave", [](int64_t F) {
    TORCH_CHECK(F >= 1 && F < (int64_t)INT32_MAX / 32, "rows_swiglu_cols_per_wave: bad F");
    return (int64_t)tbamd::rows_swiglu_cols_per_wave((int)F);
  });
  m.def("embed_rows", &embed_rows, py::arg("tokens"), py::arg("tok_weight"), py::arg("pos_weight") = py::none(),
        py::arg("positions") = py::none());
  m.def("rope_packed", &rope_packed, py::arg("qkv"), py::arg("heads"), py::arg("table"),
        py::arg("positions") = py::none(), py::arg("kv_heads") = 0, py::arg("inverse") = false,
        py::arg("out") = py::none());
  m.def("attn_extend", &attn_extend, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("positions"),
        py::arg("scale"), py::arg("workspace") = py::none(), py::arg("kv_heads") = 0, py::arg("window") = 0,
        py::arg("rolling") = false, py::arg("k_scale") = 1.0, py::arg("v_scale") = 1.0);
  // knobs and workspace sizes
  m.def("attn_set_head_mask", [](int64_t m) { return (int64_t)tbamd::attn_set_head_mask((int)m); });
  m.def("attn_decode_workspace", [](int64_t B, int64_t H, int64_t cap) {
    return tbamd::attn_decode_workspace((int)B, (int)H, (int)cap);
  });
  m.def("attn_decode_set_chunk", [](int64_t n) {
    TORCH_CHECK(n < 0 || (n >= 8 && n % 8 == 0 && n <= (1 << 20)), "attn_decode_set_chunk: a multiple of 8, >= 8");
    return (int64_t)tbamd::attn_decode_set_chunk((int)n);
  });
  m.def("attn_decode_set_head_block", [](int64_t n) {
    TORCH_CHECK(n <= 4, "attn_decode_set_head_block: 0 (the default policy) or 1 .. 4");
    return (int64_t)tbamd::attn_decode_set_head_block((int)n);
  });
  m.def("attn_decode_head_block", [](int64_t B, int64_t H, int64_t kv_heads, int64_t cap, int64_t window, bool rolling) {
    const int64_t Hkv = kv_heads_of(H, kv_heads, "attn_decode_head_block");
    TORCH_CHECK(B >= 1 && cap >= 1 && B < (int64_t)INT32_MAX && H < (int64_t)INT32_MAX && cap < (int64_t)INT32_MAX / 2,
                "attn_decode_head_block: bad size");
    if (rolling)
      return (int64_t)tbamd::attn_decode_head_block((int)B, (int)H, (int)Hkv, (int)cap,
                                                    ring_window(window, cap, 1, "attn_decode_head_block"), 1);
    return (int64_t)tbamd::attn_decode_head_block((int)B, (int)H, (int)Hkv, (int)cap,
                                                  cache_window(window, cap, "attn_decode_head_block"));
  }, py::arg("B"), py::arg("H"), py::arg("kv_heads"), py::arg("cap"), py::arg("window") = 0,
        py::arg("rolling") = false);
  m.def("attn_extend_splits", [](int64_t B, int64_t H, int64_t T, int64_t cap) {
    return (int64_t)tbamd::attn_extend_splits((int)B, (int)H, (int)T, (int)cap);
  });
  m.def("attn_extend_workspace", [](int64_t B, int64_t H, int64_t T, int64_t cap) {
    return tbamd::attn_extend_workspace((int)B, (int)H, (int)T, (int)cap);
  });
  m.def("attn_extend_set_split", [](int64_t n) {
    TORCH_CHECK(n <= 0 || (n >= 8 && n % 8 == 0 && n <= (1 << 20)),
                "attn_extend_set_split: 0 (the default policy) or a multiple of 8, >= 8");
    return (int64_t)tbamd::attn_extend_set_split((int)n);
  });
}
