// KV-cache incremental decoding (split-KV "flash-decoding"), head dim 64, bf16, gfx950, wave64.
//
// Not in the reference (it has no attention model): the inference counterpart of
// csrc/attention.hip for models/gpt.py.  A decode step has ONE query row per (batch, head), so there
// is nothing for MFMA to do: the step is a streaming read of the cache, len x 64 x 2 x 2 bytes per
// (batch, head), and its parallelism has to come from the keys.
//
// Grouped-query attention: H query heads share Hkv key / value heads (G = H / Hkv, query head h reads
// kv head h / G; Hkv = H is plain multi-head attention), the cache is [B, Hkv, cap, 64] and the
// stream per step is G times shorter in HBM.  A wave serves a HEAD BLOCK of GB in {1, 2, 3, 4} query
// heads of one group: one load of each row, GB independent copies of the per-head state and
// arithmetic below.  GB divides G (G = 12: three blocks of 4, G = 6: two of 3, G = 5: five of 1).
// With GB = 1 the G waves of a group load the same rows and the L2 serves the repeats; the host
// shares loads only when the grid can spare the waves (attn_decode_head_block below: a block of GB
// divides the waves by GB).  Per head the operations and their order do not depend on GB, so the
// output has the bits of the G = 1 kernel on the cache expanded to H heads; the partials stay
// indexed by query head, so the merge kernel and the workspace do not know about groups.
//
//   attn_kv_append_k   copies the k and v rows of a packed qkv [B, T, (H + 2*Hkv)*64] into the
//                      per-layer cache [B, Hkv, cap, 64] at rows pos[b] + t, 16 B per lane.
//   attn_decode_split_k  one wave per (batch, kv head, head block, chunk of `chunk` keys).  A wave
//                      load is 8 key rows x 128 B = one coalesced 1 KiB: lane = 8 * rowgroup + c
//                      reads dims 8c .. 8c+7 of row `rowgroup`.  Per query head of the block: q.k
//                      is a per-lane partial over 8 dims reduced over the 8 lanes of the row
//                      (xor-shuffles 1, 2, 4); every row group keeps its own online softmax
//                      (m, l) and each lane the 8 output dims of its c.  kUnroll rows per
//                      group are loaded before any is used (2 * kUnroll KiB in flight per wave).  The
//                      8 row groups are merged once at the end (xor-shuffles 8, 16, 32: a fixed
//                      tree) and lanes 0..7 write the partial: un-normalised fp32 o[64], running max
//                      (log2 domain) and sum.
//   attn_decode_append_split_k  the same wave with the append folded in (attn_decode_append): the
//                      step's own row comes from the packed qkv in every wave that meets it and is
//                      stored to the cache by the lanes of the group's first head block; a
//                      single-chunk cache is normalised and written here too.
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
//
// Sliding window (AttnDecodeArgs::window = W > 0, a host value): the query sees rows lo <= j < len,
// lo = max(0, len - W), and the rows below lo are treated exactly as the rows at or past len: not
// loaded, probability the constant 0.  A wave whose chunk ends at or below lo writes "empty" and exits,
// so a step streams at most W rows (plus what 8-row alignment adds) whatever len is; the chunk lo cuts
// starts its row loop at lo rounded down to 8, which keeps a wave load one aligned 1 KiB.  The grid is
// still a function of cap.  The merge takes its maximum over all chunks and skips the empty ones
// wherever they are: the chunk that holds row len - 1 is never empty.  The split kernels are templates
// on WIN: the <false> instantiations, which every call without a window takes, are the code they were.
//
// Rolling cache (AttnDecodeArgs::ring / AttnAppendArgs::ring, host values; needs 1 <= W <= R): the cache
// is a ring of R = cap slots, logical row j lives in slot j mod R and len = max(klen[b] + add, 1) counts
// tokens: it is not clamped to R.  Slot p holds logical row j(p), the largest j = p (mod R) below len
// (csrc/attn_ring.h), and the query sees slot p iff max(0, len - W) <= j(p): the rule above over logical
// rows.  j(p) < 0 is a slot never written; it is hidden by the same test.  The loops stay over physical
// slots -- a wave load is still one aligned 1 KiB, the grid a function of R -- and only the per-slot
// predicate and the chunk's "empty" decision change: a hidden slot is not loaded (its index is replaced
// by the chunk's first slot before an address is formed) and its probability is the constant 0.  At
// most R - W slots of a full ring are hidden, so the row loop starts at the chunk's start; a chunk with
// no visible slot writes "empty" (possible once R - W >= chunk), and the chunk of slot (len - 1) mod R is
// never empty, which is all the merge needs.  A row group may meet hidden slots anywhere in its walk,
// not only first: the m = -inf guard below is what covers it (mn = m, alpha = 1 or the constant 0, p = 0).
// The fused append takes the step's row from qkv in every wave that meets slot positions[b] mod R, which
// IS the newest row's slot, and the group's first head block stores it there.
//
// Why a ring is safe where the linear cache relied on "rows past the position are never read": an extend
// appends its T rows before its first query reads, and the host requires T <= R - W + 1.  The row written
// for token T - 1 replaces logical row pos + T - 1 - R <= pos - W, below the first query's lower limit
// pos + 1 - W, and later queries only look further right.  The same inequality covers rows past the
// position -- the pad tokens of a ragged extend, the rejected rows of a speculative round: such a stale
// slot is read as logical row pos + t - R, which no later query can see, until the sequence overwrites it.
//
// attn_kv_append_k<true> stores token t to slot (pos[b] + t) mod R iff pos[b] + t >= 0 and n_b - R <= t <
// n_b, n_b = clamp(len[b], 1, T) (T without len): the last R valid rows of a long prefill, no pad rows,
// and -- R consecutive t -- at most one store per slot per launch, so there is no write race.  A negative
// position still never becomes an address.  RING is a template parameter next to WIN: every call without
// `ring` takes the instantiations that existed before.
//
// FP8 cache (AttnDecodeArgs::fp8 / AttnAppendArgs::fp8, host values; csrc/attn_fp8.h): kc / vc hold OCP e4m3
// codes, a cache row is 64 B and the strides count bytes.  attn_kv_append_k<.., true> still gives one lane 16 B
// of qkv (8 bf16); the lane quantises them -- clamp(f32(x) * inv, -448, 448), NaN passed through, then
// v_cvt_pk_fp8_f32 -- and stores 8 B; placement, ring or linear, is the same statement.  The split kernels keep
// the (row group, c) lane map with an 8-B load per lane, so a wave load is one aligned 512 B, and unpack the
// codes with v_cvt_pk_f32_fp8 where the bf16 halves were shifted.  The scales never meet an element: k_scale is
// inside a.scale (sc = scale * k_scale * log2e, the first product an f32 one on the host), P.V accumulates the
// unscaled codes and acc is multiplied by vscale once per head after the 8 row groups are merged, ahead of the
// partial or of the single-chunk normalised store -- so the merge kernel and the workspace are those of bf16.
// The fused append quantises the step's row from qkv in EVERY wave that meets it and multiplies the codes; head
// block 0 stores them: fused and unfused calls have the same bits, output and cache.  Hidden rows are the zero
// code without a load, as they were the zero bf16: the cache may hold the NaN code there.  The lane map and
// kUnroll are those of bf16 (profiles/kv_fp8/README.md has the measurements).  FP8 is a template parameter next
// to WIN and RING: every call on a bf16 cache takes the instantiations that existed before
// (profiles/kv_fp8/resources.txt).
#include <type_traits>

#include "attn_fp8.h"
#include "attn_ring.h"
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

template <bool RING, bool FP8 = false>
__global__ __launch_bounds__(256) void attn_kv_append_k(AttnAppendArgs a) {
  // one lane per 16 B of qkv: (b, t, k|v, h, c); FP8: the 8 values leave as 8 B of codes
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)a.B * a.T * 2 * a.Hkv * 8;
  if (id >= total) return;
  const int c = (int)(id & 7);
  int64_t r = id >> 3;
  const int h = (int)(r % a.Hkv);
  r /= a.Hkv;
  const int which = (int)(r & 1);
  r >>= 1;
  const int t = (int)(r % a.T);
  const int b = (int)(r / a.T);
  int64_t row = (int64_t)a.pos[b] + t;
  if constexpr (RING) {
    int n = a.T;
    if (a.len != nullptr) n = min(max(a.len[b], 1), a.T);
    if (row < 0 || t >= n || t < n - a.cap) return;  // pad rows, and all but the last cap valid rows
    row = (int64_t)((uint32_t)row % (uint32_t)a.cap);  // 0 <= row < 2^32
  } else if (row < 0 || row >= a.cap) {
    return;  // dropped: a bad position never moves an address
  }
  const uint16_t* src = a.qkv + b * a.sqkv[0] + t * a.sqkv[1] + (int64_t)(a.H + which * a.Hkv) * 64 + h * 64 + c * 8;
  if constexpr (FP8) {  // the cache strides count codes (bytes)
    uint8_t* dst = which ? reinterpret_cast<uint8_t*>(a.vc) + b * a.sv[0] + h * a.sv[1] + row * a.sv[2] + c * 8
                         : reinterpret_cast<uint8_t*>(a.kc) + b * a.sk[0] + h * a.sk[1] + row * a.sk[2] + c * 8;
    *reinterpret_cast<uint2*>(dst) = fp8_quant8(*reinterpret_cast<const uint4*>(src), which ? a.vinv : a.kinv);
    return;
  }
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

// grid: B * Hkv * (G / GB) * nchunks one-wave workgroups, chunk fastest, then the head block: the
// wave serves query heads h0 .. h0 + GB - 1 of kv head hk, h0 = hk * G + hb * GB, and writes head
// h0 + j's partial to that head's slot (b * H + h0 + j) * nchunks + ck.  With G = 1 the block index
// IS that slot.  FUSED (attn_decode_append): row p = klen[b] comes from `n` (kv head hk of the packed
// k / v parts) instead of the cache, in EVERY wave that meets it -- it is the last visible row (len =
// p + 1), so one wave per (batch, kv head, head block) does -- and the lanes of head block 0 store it
// to the cache: exactly one store per row, and no wave reads that cache row.  p outside [0, cap)
// equals no visible row index: nothing is stored.  With one chunk the wave finishes each head with
// the merge kernel's own arithmetic (M - M, fma by exp2 of it, divide) and writes bf16.
//
// FP8 (csrc/attn_fp8.h): a cache row is 64 codes, a lane's piece of it 8 B (the same (row group, c) lane
// map: a wave load is one aligned 512 B) converted by v_cvt_pk_f32_fp8 where the bf16 halves were shifted;
// a.scale carries k_scale, and acc is multiplied by v_scale once, after the 8 row groups are merged.  The
// fused append quantises the step's row from qkv and uses the codes: what head block 0 stores is what every
// wave multiplies.
template <bool FUSED, int GB, bool WIN, bool RING, bool FP8>
__device__ __forceinline__ void attn_decode_split_body(const AttnDecodeArgs& a, const AttnNewRow& n) {
  using Row = typename std::conditional<FP8, uint2, uint4>::type;   // a lane's 8 values of a cache row
  using Elt = typename std::conditional<FP8, uint8_t, uint16_t>::type;  // what the cache strides count
  const int lane = threadIdx.x;
  const int g = lane >> 3, c = lane & 7;
  const int ck = blockIdx.x % a.nchunks;
  int bh = blockIdx.x / a.nchunks;
  const int hb = bh % a.nblk;
  bh /= a.nblk;
  const int hk = bh % a.Hkv, b = bh / a.Hkv;
  const int h0 = hk * a.group + hb * GB;
  const int part0 = (b * a.H + h0) * a.nchunks + ck;  // head h0 + j: part0 + j * nchunks
  // RING: len is the ring's size, the bound of the slots; the length itself is n below
  const int len = RING ? a.cap : decode_len(a.klen, b, a.add, a.cap);
  const int start = ck * a.chunk;
  float* wm = a.ws + (int64_t)a.nparts * 64;
  float* wl = wm + a.nparts;
  const int lo = WIN && !RING ? max(len - a.window, 0) : 0;  // the first visible row (< len)
  // RING: n = the unclamped length, pm = the slot of logical row n - 1, wv = how many rows the query
  // sees; slot r is visible iff ring_back(pm, r, cap) < wv, and a chunk none of whose slots is is empty
  int pm = 0, wv = 0;
  if constexpr (RING) {
    const int64_t n = max((int64_t)a.klen[b] + a.add, (int64_t)1);
    pm = ring_newest(n, a.cap);
    wv = (int)min((int64_t)a.window, n);
  }
  if (RING ? !ring_any(pm, 0, wv, start, min(start + a.chunk, len), len)
           : (start >= len || (WIN && start + a.chunk <= lo))) {  // wave-uniform
    if (lane < GB) {
      wm[part0 + lane * a.nchunks] = -INFINITY;
      wl[part0 + lane * a.nchunks] = 0.f;
    }
    return;
  }
  const int end = min(start + a.chunk, len);
  // the chunk's first visible row (lo < len and lo < start + chunk: < end), and the 8-row group it is in
  // (RING: the chunk's start -- a slot of the tensor, which is all a replaced index has to be)
  const int vis = WIN && !RING ? max(start, lo) : start;
  const int first = WIN && !RING ? max(start, lo & ~7) : start;

  float q[GB][8];
#pragma unroll
  for (int j = 0; j < GB; ++j)
    unpack8(*reinterpret_cast<const uint4*>(a.q + b * a.sq[0] + (h0 + j) * a.sq[1] + c * 8), q[j]);
  const float sc = a.scale * kLog2e;
  const Elt* kb = reinterpret_cast<const Elt*>(a.k) + b * a.sk[0] + hk * a.sk[1] + c * 8;
  const Elt* vb = reinterpret_cast<const Elt*>(a.v) + b * a.sv[0] + hk * a.sv[1] + c * 8;
  // RING: the step's row is logical row klen[b] = n - 1 when that is >= 0: slot pm; -1 meets no slot
  const int64_t p = FUSED ? (RING ? ((int64_t)a.klen[b] >= 0 ? (int64_t)pm : -1) : (int64_t)a.klen[b]) : -1;

  float m[GB], l[GB], acc[GB][8];
#pragma unroll
  for (int j = 0; j < GB; ++j) {
    m[j] = -INFINITY, l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
  }

  for (int r0 = first + g; r0 < end; r0 += 8 * kUnroll) {
    Row kr[kUnroll], vr[kUnroll];
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int r = r0 + 8 * u;
      if constexpr (RING) ok[u] = r < end && ring_back(pm, r, len) < wv;
      else ok[u] = r < end && (!WIN || r >= lo);
      const int rr = ok[u] ? r : vis;  // a hidden row never forms an address
      if constexpr (FP8) {
        kr[u] = make_uint2(0, 0);  // the code of +0
        vr[u] = make_uint2(0, 0);
      } else {
        kr[u] = make_uint4(0, 0, 0, 0);
        vr[u] = make_uint4(0, 0, 0, 0);
      }
      if (FUSED && ok[u] && (int64_t)r == p) {  // 0 <= r < len <= cap: the store is inside the cache
        if constexpr (FP8) {
          kr[u] = fp8_quant8(*reinterpret_cast<const uint4*>(n.k + b * n.s + hk * 64 + c * 8), a.kinv);
          vr[u] = fp8_quant8(*reinterpret_cast<const uint4*>(n.v + b * n.s + hk * 64 + c * 8), a.vinv);
        } else {
          kr[u] = *reinterpret_cast<const uint4*>(n.k + b * n.s + hk * 64 + c * 8);
          vr[u] = *reinterpret_cast<const uint4*>(n.v + b * n.s + hk * 64 + c * 8);
        }
        if (hb == 0) {  // wave-uniform: one storing wave per (batch, kv head)
          *reinterpret_cast<Row*>(const_cast<Elt*>(kb) + rr * a.sk[2]) = kr[u];
          *reinterpret_cast<Row*>(const_cast<Elt*>(vb) + rr * a.sv[2]) = vr[u];
        }
      } else if (ok[u]) {
        kr[u] = *reinterpret_cast<const Row*>(kb + rr * a.sk[2]);
        vr[u] = *reinterpret_cast<const Row*>(vb + rr * a.sv[2]);
      }
    }
    // from here on: GB copies of one head's arithmetic on the same rows
    float s[GB][kUnroll];
    float mn[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) mn[j] = m[j];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      float kf[8];
      if constexpr (FP8) fp8_unpack8(kr[u], kf);
      else unpack8(kr[u], kf);
#pragma unroll
      for (int j = 0; j < GB; ++j) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d = fmaf(q[j][i], kf[i], d);
        d = group8_sum(d) * sc;
        s[j][u] = ok[u] ? d : -INFINITY;
        mn[j] = fmaxf(mn[j], s[j][u]);
      }
    }
    // r0 < end: row u = 0 is visible, so mn is finite from here on -- except in a row group's first
    // pass over the chunk a window cuts, where r0 may lie below lo: if none of its rows is visible,
    // mn = m = -inf, alpha is the constant 0 and no p is exp2 of anything.  In a ring a pass may be all
    // hidden anywhere in the walk: before the first visible slot it is that case, after it mn = m is
    // finite, alpha is exp2(0) and every p the constant 0
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const float alpha = m[j] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[j] - mn[j]);
      l[j] *= alpha;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j][i] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      float vf[8];
      if constexpr (FP8) fp8_unpack8(vr[u], vf);
      else unpack8(vr[u], vf);  // zeros where !ok
#pragma unroll
      for (int j = 0; j < GB; ++j) {
        const float p = ok[u] ? __builtin_amdgcn_exp2f(s[j][u] - mn[j]) : 0.f;
        l[j] += p;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] = fmaf(p, vf[i], acc[j][i]);
      }
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) m[j] = mn[j];
  }

#pragma unroll
  for (int j = 0; j < GB; ++j) {
    // merge the 8 row groups (a group with no row has m = -inf, l = 0, acc = 0)
    float M = m[j];
    M = fmaxf(M, __shfl_xor(M, 8, 64));
    M = fmaxf(M, __shfl_xor(M, 16, 64));
    M = fmaxf(M, __shfl_xor(M, 32, 64));
    const float f = m[j] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[j] - M);
    l[j] *= f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] *= f;
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      l[j] += __shfl_xor(l[j], o, 64);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j][i] += __shfl_xor(acc[j][i], o, 64);
    }
    if constexpr (FP8) {  // P.V ran on the unscaled codes
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j][i] *= a.vscale;
    }
    if (FUSED && a.nchunks == 1) {  // what attn_decode_merge_k computes from this one partial
      if (g == 0) {
        const float f = __builtin_amdgcn_exp2f(M - M);
        const float L = fmaf(f, l[j], 0.f);
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = fmaf(f, acc[j][i], 0.f) / L;
        Vec8<kBF16>::store(a.o + b * a.so[0] + (h0 + j) * a.so[1] + c * 8, o);
      }
      continue;
    }
    if (g == 0) {
      const int part = part0 + j * a.nchunks;
      float* wo = a.ws + (int64_t)part * 64 + c * 8;
      *reinterpret_cast<float4*>(wo) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
      *reinterpret_cast<float4*>(wo + 4) = make_float4(acc[j][4], acc[j][5], acc[j][6], acc[j][7]);
      if (c == 0) {
        wm[part] = M;
        wl[part] = l[j];
      }
    }
  }
}

template <int GB, bool WIN, bool RING = false, bool FP8 = false>
__global__ __launch_bounds__(64) void attn_decode_split_k(AttnDecodeArgs a) {
  attn_decode_split_body<false, GB, WIN, RING, FP8>(a, AttnNewRow{nullptr, nullptr, 0});
}

template <int GB, bool WIN, bool RING = false, bool FP8 = false>
__global__ __launch_bounds__(64) void attn_decode_append_split_k(AttnDecodeArgs a, AttnNewRow n) {
  attn_decode_split_body<true, GB, WIN, RING, FP8>(a, n);
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
  for (int ck = 0; ck < a.nchunks; ++ck) M = fmaxf(M, wm[ck]);  // the chunk of row len - 1 is never empty: finite
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
  const int64_t total = (int64_t)a.B * a.T * 2 * a.Hkv * 8;
  if (total == 0) return;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (a.fp8) {
    if (a.ring) hipLaunchKernelGGL((attn_kv_append_k<true, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_kv_append_k<false, true>), grid, dim3(256), 0, st, a);
  } else if (a.ring) {
    hipLaunchKernelGGL(attn_kv_append_k<true>, grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(attn_kv_append_k<false>, grid, dim3(256), 0, st, a);
  }
}

// Query heads per wave.  A head block of GB loads a K / V row G / GB times instead of G times, and
// leaves 1 / GB of the waves.  Reasoned from the bytes the first choice was the largest GB that
// divides G; measured (profiles/gqa/README.md: H = 12, Hkv 6 .. 1, len 1024 .. 16384, B 1 .. 128) the
// L2 serves the repeats of a group at no visible cost while the grid is small, and the waves are what
// a call is short of: with W = B * H * nchunks one-head waves, GB = 1 is the fastest at every shape
// up to W = 3072 (B = 8, len 4096: 23.6 us against 26.1 at GB = 4 and 35.5 on the expanded cache), at
// W = 6144 GB = 2 leads by 6 % and GB = 4 trails, at W = 12288 GB = 4 leads GB = 1 by 6 .. 11 %, and
// at W = 49152 sharing wins by 13 .. 18 %.  So the default is the largest GB of 4, 3, 2 that divides
// G and still leaves kDecodeShareWaves waves (12 per CU on 256 CUs), else 1: a function of shapes
// only.  The worst this rule does at a measured shape is 2.5 % behind the best block (G = 3,
// W = 12288).  Any G runs natively whatever the block; G = 1 is always GB = 1.
static int g_decode_head_block = 0;  // 0: the default policy; otherwise a forced block where it divides G
constexpr int64_t kDecodeShareWaves = 3072;

int attn_decode_set_head_block(int n) {
  const int old = g_decode_head_block;
  if (n >= 0 && n <= 4) g_decode_head_block = n;
  return old;
}

int attn_decode_head_block(int B, int H, int Hkv, int cap, int window, int ring) {
  if (ring) window = 0;  // a ring is cap live rows: any chunk may hold visible slots
  const int G = H / Hkv;
  if (g_decode_head_block && G % g_decode_head_block == 0) return g_decode_head_block;
  // the waves that stream rows: under a window the other chunks write "empty" and exit
  int live = attn_decode_chunks(cap);
  if (window > 0 && (int64_t)window + g_decode_chunk < cap) live = attn_decode_chunks(window + g_decode_chunk);
  const int64_t waves = (int64_t)B * H * live;
  for (int gb = 4; gb > 1; --gb)
    if (G % gb == 0 && waves / gb >= kDecodeShareWaves) return gb;
  return 1;
}

// chunk / nchunks / nparts / group / nblk, and the head block the grid is built for
static int decode_plan(AttnDecodeArgs& a) {
  a.chunk = g_decode_chunk;
  a.nchunks = attn_decode_chunks(a.cap);
  a.nparts = a.B * a.H * a.nchunks;
  a.group = a.H / a.Hkv;
  const int gb = attn_decode_head_block(a.B, a.H, a.Hkv, a.cap, a.window, a.ring);
  a.nblk = a.group / gb;
  return gb;
}

// the split launch for head block gb; WIN: the windowed instantiations, RING: the rolling ones, FP8: the
// e4m3-cache ones
template <bool WIN, bool RING = false, bool FP8 = false>
static void launch_split(int gb, dim3 grid, const AttnDecodeArgs& a, hipStream_t st) {
  switch (gb) {
    case 1: hipLaunchKernelGGL((attn_decode_split_k<1, WIN, RING, FP8>), grid, dim3(64), 0, st, a); break;
    case 2: hipLaunchKernelGGL((attn_decode_split_k<2, WIN, RING, FP8>), grid, dim3(64), 0, st, a); break;
    case 3: hipLaunchKernelGGL((attn_decode_split_k<3, WIN, RING, FP8>), grid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL((attn_decode_split_k<4, WIN, RING, FP8>), grid, dim3(64), 0, st, a); break;
  }
}

template <bool WIN, bool RING = false, bool FP8 = false>
static void launch_append_split(int gb, dim3 grid, const AttnDecodeArgs& a, const AttnNewRow& n, hipStream_t st) {
  switch (gb) {
    case 1: hipLaunchKernelGGL((attn_decode_append_split_k<1, WIN, RING, FP8>), grid, dim3(64), 0, st, a, n); break;
    case 2: hipLaunchKernelGGL((attn_decode_append_split_k<2, WIN, RING, FP8>), grid, dim3(64), 0, st, a, n); break;
    case 3: hipLaunchKernelGGL((attn_decode_append_split_k<3, WIN, RING, FP8>), grid, dim3(64), 0, st, a, n); break;
    default: hipLaunchKernelGGL((attn_decode_append_split_k<4, WIN, RING, FP8>), grid, dim3(64), 0, st, a, n); break;
  }
}

void attn_decode(const AttnDecodeArgs& a_, hipStream_t st) {
  AttnDecodeArgs a = a_;
  const int gb = decode_plan(a);
  const dim3 grid(a.nparts / gb);  // B * Hkv * nblk * nchunks
  if (a.fp8) {
    if (a.ring) launch_split<true, true, true>(gb, grid, a, st);
    else if (a.window > 0) launch_split<true, false, true>(gb, grid, a, st);
    else launch_split<false, false, true>(gb, grid, a, st);
  } else if (a.ring) launch_split<true, true>(gb, grid, a, st);
  else if (a.window > 0) launch_split<true>(gb, grid, a, st);
  else launch_split<false>(gb, grid, a, st);
  hipLaunchKernelGGL(attn_decode_merge_k, dim3(a.B * a.H), dim3(64), 0, st, a);
}

void attn_decode_append(const AttnDecodeArgs& a_, const uint16_t* nk, const uint16_t* nv, int64_t snew,
                        hipStream_t st) {
  AttnDecodeArgs a = a_;
  a.add = 1;
  const int gb = decode_plan(a);
  const dim3 grid(a.nparts / gb);
  const AttnNewRow n{nk, nv, snew};
  if (a.fp8) {
    if (a.ring) launch_append_split<true, true, true>(gb, grid, a, n, st);
    else if (a.window > 0) launch_append_split<true, false, true>(gb, grid, a, n, st);
    else launch_append_split<false, false, true>(gb, grid, a, n, st);
  } else if (a.ring) launch_append_split<true, true>(gb, grid, a, n, st);
  else if (a.window > 0) launch_append_split<true>(gb, grid, a, n, st);
  else launch_append_split<false>(gb, grid, a, n, st);
  if (a.nchunks > 1) hipLaunchKernelGGL(attn_decode_merge_k, dim3(a.B * a.H), dim3(64), 0, st, a);
}

}  // namespace tbamd
