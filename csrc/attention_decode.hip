// KV-cache incremental decoding (split-KV "flash-decoding"), head dim 64, bf16, gfx950, wave64.
//
// Not in the reference (it has no attention model): the inference counterpart of
// csrc/attention.hip for models/gpt.py.  A decode step has ONE query row per (batch, head), so there
// is nothing for MFMA to do: the step is a streaming read of the cache, len x 64 x 2 x 2 bytes per
// (batch, head), and its parallelism has to come from the keys.
//
//   attn_kv_append_k   copies the k and v rows of a packed qkv [B, T, 3*H*64] into the per-layer
//                      cache [B, H, cap, 64] at rows pos[b] + t, 16 B per lane.
//   attn_decode_split_k  one wave per (batch, head, chunk of `chunk` keys).  A wave load is 8 key rows
//                      x 128 B = one coalesced 1 KiB: lane = 8 * rowgroup + c reads dims 8c .. 8c+7 of
//                      row `rowgroup`.  q.k is a per-lane partial over 8 dims reduced over the 8 lanes
//                      of the row (xor-shuffles 1, 2, 4); every row group keeps its own online
//                      softmax (m, l) and each lane the 8 output dims of its c.  kUnroll rows per
//                      group are loaded before any is used (2 * kUnroll KiB in flight per wave).  The
//                      8 row groups are merged once at the end (xor-shuffles 8, 16, 32: a fixed
//                      tree) and lanes 0..7 write the partial: un-normalised fp32 o[64], running max
//                      (log2 domain) and sum.
//   attn_decode_append_split_k  the same wave with the append folded in (attn_decode_append): the
//                      step's own row comes from the packed qkv and is stored to the cache by the
//                      lanes that load it; a single-chunk cache is normalised and written here too.
//   attn_decode_merge_k  one wave per (batch, head): merges the chunk partials in chunk order, divides
//                      by the sum and writes bf16.  No float atomics: deterministic, every output
//                      element written exactly once.
//
// len = clamp(klen[b] + add, 1, cap) is read from device memory by the kernels; the grids depend
// on cap only, so there is no host sync, a capture is safe and a replay follows in-place changes
// of klen.  A wave whose chunk starts at or past len writes m = -inf ("empty") and exits; the
// merge skips such partials without reading their o.
//
// Rows at or past len never enter arithmetic: their loads are not issued (the row index is
// clamped to the chunk's first row, which is < len, and the load is predicated), and their
// probability is the constant 0, not exp2 of anything.  The cache may hold any bit pattern there.
#include "common.h"
#include "tbamd.h"

namespace tbamd {
namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kUnroll = 4;  // key rows per row group in flight

__device__ __forceinline__ float group8_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

__device__ __forceinline__ void unpack8(const uint4& r, float (&v)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ int decode_len(const int* klen, int b, int add, int cap) {
  const int64_t l = (int64_t)klen[b] + add;
  return (int)(l < 1 ? 1 : (l > cap ? cap : l));
}

__global__ __launch_bounds__(256) void attn_kv_append_k(AttnAppendArgs a) {
  // one lane per 16 B: (b, t, k|v, h, c)
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)a.B * a.T * 2 * a.H * 8;
  if (id >= total) return;
  const int c = (int)(id & 7);
  int64_t r = id >> 3;
  const int h = (int)(r % a.H);
  r /= a.H;
  const int which = (int)(r & 1);
  r >>= 1;
  const int t = (int)(r % a.T);
  const int b = (int)(r / a.T);
  const int64_t row = (int64_t)a.pos[b] + t;
  if (row < 0 || row >= a.cap) return;  // dropped: a bad position never moves an address
  const uint16_t* src = a.qkv + b * a.sqkv[0] + t * a.sqkv[1] + (int64_t)(1 + which) * a.H * 64 + h * 64 + c * 8;
  uint16_t* dst = which ? a.vc + b * a.sv[0] + h * a.sv[1] + row * a.sv[2] + c * 8
                        : a.kc + b * a.sk[0] + h * a.sk[1] + row * a.sk[2] + c * 8;
  *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
}

// The k / v row of this step's token for the fused append: the k and v parts of the packed qkv.
struct AttnNewRow {
  const uint16_t* k;
  const uint16_t* v;
  int64_t s;  // batch stride; the head stride is 64
};

// grid: B * H * nchunks one-wave workgroups, chunk fastest.  FUSED (attn_decode_append): row
// p = klen[b] comes from `n` instead of the cache and the lanes that load it store it to the cache;
// it is the last visible row (len = p + 1), so exactly one wave of a (batch, head) meets it and no
// other wave reads it.  p outside [0, cap) equals no visible row index: nothing is stored.  With one
// chunk the wave finishes with the merge kernel's own arithmetic (M - M, fma by exp2 of it, divide)
// and writes bf16.
template <bool FUSED>
__device__ __forceinline__ void attn_decode_split_body(const AttnDecodeArgs& a, const AttnNewRow& n) {
  const int lane = threadIdx.x;
  const int g = lane >> 3, c = lane & 7;
  const int part = blockIdx.x;
  const int ck = part % a.nchunks;
  const int bh = part / a.nchunks;
  const int h = bh % a.H, b = bh / a.H;
  const int len = decode_len(a.klen, b, a.add, a.cap);
  const int start = ck * a.chunk;
  float* wm = a.ws + (int64_t)a.nparts * 64;
  float* wl = wm + a.nparts;
  if (start >= len) {  // wave-uniform
    if (lane == 0) {
      wm[part] = -INFINITY;
      wl[part] = 0.f;
    }
    return;
  }
  const int end = min(start + a.chunk, len);

  float q[8];
  unpack8(*reinterpret_cast<const uint4*>(a.q + b * a.sq[0] + h * a.sq[1] + c * 8), q);
  const float sc = a.scale * kLog2e;
  const uint16_t* kb = a.k + b * a.sk[0] + h * a.sk[1] + c * 8;
  const uint16_t* vb = a.v + b * a.sv[0] + h * a.sv[1] + c * 8;
  const int64_t p = FUSED ? (int64_t)a.klen[b] : -1;

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;

  for (int r0 = start + g; r0 < end; r0 += 8 * kUnroll) {
    uint4 kr[kUnroll], vr[kUnroll];
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int r = r0 + 8 * u;
      ok[u] = r < end;
      const int rr = ok[u] ? r : start;  // a hidden row never forms an address
      kr[u] = make_uint4(0, 0, 0, 0);
      vr[u] = make_uint4(0, 0, 0, 0);
      if (FUSED && ok[u] && (int64_t)r == p) {  // 0 <= r < len <= cap: the store is inside the cache
        kr[u] = *reinterpret_cast<const uint4*>(n.k + b * n.s + h * 64 + c * 8);
        vr[u] = *reinterpret_cast<const uint4*>(n.v + b * n.s + h * 64 + c * 8);
        *reinterpret_cast<uint4*>(const_cast<uint16_t*>(kb) + rr * a.sk[2]) = kr[u];
        *reinterpret_cast<uint4*>(const_cast<uint16_t*>(vb) + rr * a.sv[2]) = vr[u];
      } else if (ok[u]) {
        kr[u] = *reinterpret_cast<const uint4*>(kb + rr * a.sk[2]);
        vr[u] = *reinterpret_cast<const uint4*>(vb + rr * a.sv[2]);
      }
    }
    float s[kUnroll];
    float mn = m;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      float kf[8];
      unpack8(kr[u], kf);
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d = fmaf(q[i], kf[i], d);
      d = group8_sum(d) * sc;
      s[u] = ok[u] ? d : -INFINITY;
      mn = fmaxf(mn, s[u]);
    }
    // r0 < end: row u = 0 is visible, so mn is finite from here on
    const float alpha = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mn);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= alpha;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const float p = ok[u] ? __builtin_amdgcn_exp2f(s[u] - mn) : 0.f;
      float vf[8];
      unpack8(vr[u], vf);  // zeros where !ok
      l += p;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(p, vf[i], acc[i]);
    }
    m = mn;
  }

  // merge the 8 row groups (a group with no row has m = -inf, l = 0, acc = 0)
  float M = m;
  M = fmaxf(M, __shfl_xor(M, 8, 64));
  M = fmaxf(M, __shfl_xor(M, 16, 64));
  M = fmaxf(M, __shfl_xor(M, 32, 64));
  const float f = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - M);
  l *= f;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] *= f;
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    l += __shfl_xor(l, o, 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += __shfl_xor(acc[i], o, 64);
  }
  if (FUSED && a.nchunks == 1) {  // what attn_decode_merge_k computes from this one partial
    if (g == 0) {
      const float f = __builtin_amdgcn_exp2f(M - M);
      const float L = fmaf(f, l, 0.f);
      float o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = fmaf(f, acc[i], 0.f) / L;
      Vec8<kBF16>::store(a.o + b * a.so[0] + h * a.so[1] + c * 8, o);
    }
    return;
  }
  if (g == 0) {
    float* wo = a.ws + (int64_t)part * 64 + c * 8;
    *reinterpret_cast<float4*>(wo) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(wo + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    if (c == 0) {
      wm[part] = M;
      wl[part] = l;
    }
  }
}

__global__ __launch_bounds__(64) void attn_decode_split_k(AttnDecodeArgs a) {
  attn_decode_split_body<false>(a, AttnNewRow{nullptr, nullptr, 0});
}

__global__ __launch_bounds__(64) void attn_decode_append_split_k(AttnDecodeArgs a, AttnNewRow n) {
  attn_decode_split_body<true>(a, n);
}

// grid: B * H one-wave workgroups; lane = output dim
__global__ __launch_bounds__(64) void attn_decode_merge_k(AttnDecodeArgs a) {
  const int d = threadIdx.x;
  const int bh = blockIdx.x;
  const int h = bh % a.H, b = bh / a.H;
  const float* wo = a.ws + (int64_t)bh * a.nchunks * 64;
  const float* wm = a.ws + (int64_t)a.nparts * 64 + (int64_t)bh * a.nchunks;
  const float* wl = wm + a.nparts;
  float M = -INFINITY;
  for (int ck = 0; ck < a.nchunks; ++ck) M = fmaxf(M, wm[ck]);  // chunk 0 is never empty: finite
  float o = 0.f, L = 0.f;
  for (int ck = 0; ck < a.nchunks; ++ck) {
    const float mc = wm[ck];
    if (mc == -INFINITY) continue;  // empty: its o was never written and is never read
    const float f = __builtin_amdgcn_exp2f(mc - M);
    L = fmaf(f, wl[ck], L);
    o = fmaf(f, wo[(int64_t)ck * 64 + d], o);
  }
  a.o[b * a.so[0] + h * a.so[1] + d] = f2bf(o / L);
}

}  // namespace

// Keys per workgroup.  One wave streams 8 rows per load, kUnroll = 4 loads deep: 128 keys are four
// full-depth iterations per wave (32 KiB read per workgroup against 264 B of partial written).  At
// gpt2_small shapes (H = 12, cap = 1024) that is 8 chunks per head, 96 waves at batch 1 and 768 at
// batch 8 over 256 CUs.  Reasoned from the code the first choice was 64 (twice the waves); measured
// (profiles/decode/README.md: 32 / 64 / 128 / 256 at B*H 12 .. 384, len 128 .. 4096) 128 is the
// faster of the two at 8 of the 12 shapes: by about 12 % at len 1024 and 1.1 .. 1.4x at len 4096,
// a few per cent either way at len 512, and slower by 6 .. 16 % at len 128, where a call is 6 .. 9
// us of launches.  256 wins from len 4096 on.  The per-chunk cost that does not stream (q load, the
// 8-group merge, the partial, one serial merge step per chunk in attn_decode_merge_k) is what 64
// pays twice as often.
static int g_decode_chunk = 128;

int attn_decode_set_chunk(int n) {
  const int old = g_decode_chunk;
  if (n >= 8 && n % 8 == 0) g_decode_chunk = n;
  return old;
}

int attn_decode_chunks(int cap) { return (cap + g_decode_chunk - 1) / g_decode_chunk; }

int64_t attn_decode_workspace(int B, int H, int cap) { return (int64_t)B * H * attn_decode_chunks(cap) * 66; }

void attn_kv_append(const AttnAppendArgs& a, hipStream_t st) {
  const int64_t total = (int64_t)a.B * a.T * 2 * a.H * 8;
  if (total == 0) return;
  hipLaunchKernelGGL(attn_kv_append_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

void attn_decode(const AttnDecodeArgs& a_, hipStream_t st) {
  AttnDecodeArgs a = a_;
  a.chunk = g_decode_chunk;
  a.nchunks = attn_decode_chunks(a.cap);
  a.nparts = a.B * a.H * a.nchunks;
  hipLaunchKernelGGL(attn_decode_split_k, dim3(a.nparts), dim3(64), 0, st, a);
  hipLaunchKernelGGL(attn_decode_merge_k, dim3(a.B * a.H), dim3(64), 0, st, a);
}

void attn_decode_append(const AttnDecodeArgs& a_, const uint16_t* nk, const uint16_t* nv, int64_t snew,
                        hipStream_t st) {
  AttnDecodeArgs a = a_;
  a.add = 1;
  a.chunk = g_decode_chunk;
  a.nchunks = attn_decode_chunks(a.cap);
  a.nparts = a.B * a.H * a.nchunks;
  hipLaunchKernelGGL(attn_decode_append_split_k, dim3(a.nparts), dim3(64), 0, st, a, AttnNewRow{nk, nv, snew});
  if (a.nchunks > 1) hipLaunchKernelGGL(attn_decode_merge_k, dim3(a.B * a.H), dim3(64), 0, st, a);
}

}  // namespace tbamd
