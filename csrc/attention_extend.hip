// KV-cache "extend" attention: T >= 1 new queries per (batch, head) against a cache that already
// holds tokens.  Head dim 64, bf16, gfx950, wave64.
//
// Not in the reference (it has no attention model).  csrc/attention_decode.hip runs
// ONE query per (batch, head) and is pure VALU by design; a prefill (csrc/attention.hip) attends
// only within the new tokens.  This file is the piece between them: query t of batch b, whose k / v
// row was just appended at pos[b] + t, sees the cache rows
//
//     j < L(b, t) = clamp(pos[b] + t + 1, 1, cap)        (64-bit arithmetic, as decode_len)
//
// which is what continuing a conversation, chunked prefill and scoring several candidate tokens in
// one pass (speculative decoding) need.  With 16 queries there is work for v_mfma_f32_16x16x32_bf16.
//
//   attn_extend_split_k  one wave (one workgroup) per (batch, head, tile of 16 queries, key split).
//                      Swapped orientation as csrc/attention.hip: Sᵀ[key][q] = K·Qᵀ puts ONE query
//                      on a lane (fr = lane & 15), so the online softmax (log2 domain, bare exp2)
//                      is per-lane scalars, and the accumulator pair is the B operand of
//                      Oᵀ[d][q] += Vᵀ·Pᵀ.  Keys run in tiles of 64: the K operand rows are read
//                      straight from global memory (a lane's 16 B of a key row IS its A fragment;
//                      a one-wave workgroup has nobody to share a staged tile with), V goes
//                      through a swizzled LDS tile (direct global->LDS loads) for the transposed
//                      read.  Both are double buffered: the loads of tile i + 1 are issued before
//                      tile i's products (the compiler drains them ahead of tile i's first LDS
//                      read, so they overlap Sᵀ and the softmax, not P·V: profiles/extend).
//                      With one split the wave normalises and writes bf16 itself; otherwise it
//                      writes a partial: un-normalised fp32 o[16][64], running max and sum per row.
//   attn_extend_merge_k  one wave per (batch, query, head), lane = output dim: merges the split
//                      partials in split order, divides by the sum, writes bf16.  No atomics:
//                      deterministic, every output element written exactly once.
//
// Grouped-query attention (caches [B, Hkv, cap, 64], G = H / Hkv): a wave still serves one query
// head and reads kv head h / G; the G waves of a group read the same rows and the L2 serves the
// repeats.  Nothing else changes, so the output has the bits of the same call on the cache expanded to
// H heads.  (Packing the (t, g) rows of a group into one 16-query tile is not done: profiles/gqa.)
//
// pos is read on the device; the grid and the workspace are functions of (B, H, T, cap) only: no
// host sync, a capture is safe and a replay follows in-place changes of pos.  The last query tile
// is padded (pad queries take zeros for q and the last real query's limit; they are never stored).
//
// Key splits.  hi = the largest L of the tile's queries, cut to the split's end.  A split that
// starts at or past hi writes "empty" (m = -inf, l = 0 for its 16 rows) and exits: a
// workgroup-uniform decision.  Inside a live split a row may see no key (L(b, t) <= the split's
// start): visibility is a prefix of the split, so such a row sees nothing in ANY of its tiles, keeps
// m = -inf, l = 0, and the merge skips it without reading its o.  Split 0 holds key 0, which every
// row sees: it is never empty for any row.
//
// What may enter arithmetic.  Cache rows at or past clamp(pos[b] + T, 1, cap) NEVER do: rows at or
// past hi (<= that bound) are not loaded -- the K fragment is the constant zero and its row index is
// replaced by the split's first row before an address is formed, the V rows are staged from a zero
// row -- so the never-written part of a torch.empty cache, NaN / Inf bit patterns included, cannot
// reach the output (0 * NaN in the P·V MFMA would be NaN: masking after a load is not enough).
// Rows between a query's own limit L(b, t) and hi are the rows this call's tokens just appended
// for later queries of the same 16-query tile: real finite data.  Their scores are masked to -inf,
// their probability is an exact 0, and that 0 IS multiplied with their v in the MFMA.
//
// Sliding window (AttnExtendArgs::window = W > 0, a host value): query t sees the rows
// max(0, L(b, t) - W) <= j < L(b, t).  lo = the lower limit of the tile's FIRST query (the smallest,
// as L grows with t), raised to the split's start: a split that ends at or below it writes "empty", and
// rows below lo are treated as the rows at or past hi -- zero K fragment, index replaced before an
// address is formed, zero-row V staging -- so they never enter arithmetic.  Rows between lo and a
// query's own lower limit are real, previously appended data whose scores are masked to -inf (an
// exact-zero probability in the MFMA).  Visibility inside a split is now an interval: a row may see
// nothing in one tile and something in the next (the ms guard below covers it), and a row's first
// non-empty split need not be split 0 -- the merge takes its maximum over all splits, and the split
// that holds row L(b, t) - 1 is never empty for query t.  The split kernel is a template on WIN: the
// <false> instantiation, which every call without a window takes, is the code it was.
//
// Rolling cache (AttnExtendArgs::ring, a host value; needs 1 <= W <= R = cap and T <= R - W + 1): the
// cache is a ring, logical row j lives in slot j mod R, L(b, t) = max(pos[b] + t + 1, 1) is not clamped
// to R, and for the whole call slot p holds logical row j(p), the largest j = p (mod R) below n =
// L(b, T - 1).  Query t sees slot p iff max(0, L(b, t) - W) <= j(p) < L(b, t) -- the rule above over
// logical rows -- which the kernel tests on the distance d(p) = n - 1 - j(p) (csrc/attn_ring.h): n -
// L(b, t) <= d(p) < min(n, n - L(b, t) + W).  T - 1 + W <= R keeps these bounds inside one turn of the ring.
// The loops stay over physical slots (splits and 64-slot tiles of [0, R), from the split's start: a
// full ring hides at most R - W slots); the tile's lo / hi become the logical bounds of its 16 queries
// as distances, dlo from the last query's upper limit and dhi from the first query's lower one, and a
// slot outside them is treated exactly as a row outside [lo, hi) is: zero K fragment, index replaced
// before an address is formed, zero-row V staging.  That covers the slots never written (j(p) < 0 is
// d(p) >= n) and the stale ones.  A slot inside the tile's bounds and outside a query's own holds a
// logical row in [max(0, L(b, q0) - W), L(b, tile's last query)): real appended data, masked to -inf,
// an exact-zero probability in the MFMA.  In SLOT space the tile's set, and each query's, is a cyclic
// interval: up to two intervals of [0, R).  So "visibility is a prefix / an interval of the split" does
// not hold here and nothing below relies on it: a split is empty iff neither interval meets it
// (ring_any); inside a live split a row may see nothing in a tile before or after one in which it sees
// keys, and the ms guard covers both orders (m = -inf: alpha is exp2(-inf - 0) = 0 on zero acc and l; m
// finite and the tile hidden: mn = m, alpha = 1, every p = 0); a row that sees nothing in the whole split
// keeps m = -inf and is skipped by the merge, which takes its maximum over all splits.  The split of
// slot (L(b, t) - 1) mod R is never empty for query t.
//
// Why the ring is safe: the call's T rows are appended before its first query reads, and T <= R - W + 1
// means the row of token T - 1 replaced logical row pos + T - 1 - R <= pos - W, below the first query's
// lower limit pos + 1 - W.  Rows past the position (pad tokens of a ragged extend, rejected rows of a
// speculative round) are read as logical row pos + t - R by the same inequality: no later query sees it.
//
// FP8 cache (AttnExtendArgs::fp8, a host value; csrc/attn_fp8.h): the caches hold OCP e4m3 codes, 64 B a row,
// strides in bytes.  A lane's K fragment is an 8-B load converted to bf16x8 (v_cvt_pk_f32_fp8, then the upper
// halves: exact, a code has 4 significant bits), so the MFMA operands ARE the dequantised codes; the score factor
// carries k_scale (a.scale, an f32 product on the host).  V cannot take the direct global->LDS path, which moves
// 16 B of bf16: a lane loads 8 x 8 B of codes into registers (a wave load is 8 rows x 64 B), converts them and
// writes the same swizzled bf16 tile, so tr_frag and P.V are untouched.  The double buffering stays: the K
// fragments and V codes of tile i + 1 are in flight during tile i's products, and tile i's codes are converted
// and written to its LDS buffer at the top of its iteration, ahead of the barrier.  Hidden rows are decided by the
// predicates above (RowsLoaded) and become the zero code without forming an address.  The accumulator is
// multiplied by vscale once, before the store or the partial; the merge kernel is unchanged.  FP8 is a template
// parameter next to WIN and RING: bf16 caches take the instantiations that existed (profiles/kv_fp8/resources.txt).
#include "attn_fp8.h"
#include "attn_ring.h"
#include "common.h"
#include "mfma_tile.h"
#include "tbamd.h"

namespace tbamd {
namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kQT = 16;  // queries per wave

// s_waitcnt vmcnt(0) (gfx9 encoding: expcnt and lgkmcnt left at their maxima)
__device__ __forceinline__ void wait_loads() { __builtin_amdgcn_s_waitcnt(0x0F70); }

__device__ __forceinline__ int extend_len(const int* pos, int b, int t, int cap) {
  const int64_t l = (int64_t)pos[b] + t + 1;
  return (int)(l < 1 ? 1 : (l > cap ? cap : l));
}

// A fragments of key rows k0 .. k0 + 63: lane holds K[k0 + 16 mt + fr][32 ks + 8 fg .. + 7]
// (rows outside [lo, hi) are zeros; lo itself is a row inside the range: the split's start without a window)
template <bool WIN>
__device__ __forceinline__ void load_k(bf16x8_t (&kf)[4][2], const uint16_t* kb, int64_t rs, int k0, int lo, int hi,
                                       int fr, int fg) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int r = k0 + 16 * mt + fr;
    const bool ok = r < hi && (!WIN || r >= lo);
    const int rr = ok ? r : lo;  // a hidden row never forms an address
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[mt][ks] = bf16x8_t{};
      if (ok) kf[mt][ks] = ld_frag(kb + rr * rs + 32 * ks + 8 * fg);
    }
  }
}

// V rows k0 .. k0 + 63 -> swizzled LDS tile by ONE wave (stage_tile's four wave slots in turn);
// rows at or past hi and, under a window, rows below lo come from the zero row
template <bool WIN>
__device__ __forceinline__ void stage_v(uint4* tile, const uint16_t* vb, int64_t rs, int k0, int lo, int hi,
                                        int lane) {
  if constexpr (!WIN) {
#pragma unroll
    for (int w = 0; w < 4; ++w) stage_tile(tile, vb, rs, k0, hi, w, lane);
    return;
  }
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int it = 0; it < 2; ++it) {  // stage_tile with a lower row bound
      const int row = 32 * it + w * 8 + (lane >> 3);
      const int r = k0 + row;
      const int ch = (lane & 7) ^ aswz(row);
      const void* src = r < hi && r >= lo ? (const void*)(vb + (int64_t)r * rs + ch * 8) : (const void*)g_tile_zero;
      glds16(src, tile + (32 * it + w * 8) * 8);
    }
}

// What a wave of the rolling cache knows about its slots (csrc/attn_ring.h): slot p, start <= p < hi
// (hi <= R), is loaded iff dlo <= d(p) < dhi, the union of its 16 queries' windows.
struct RingTile {
  int pm, dlo, dhi, R, start, hi;
  __device__ __forceinline__ bool loads(int p) const {
    const int d = ring_back(pm, p, R);
    return p < hi && d >= dlo && d < dhi;
  }
};

// load_k / stage_v of a ring: the same fragments and the same LDS tile, the per-slot test of RingTile
__device__ __forceinline__ void load_k_ring(bf16x8_t (&kf)[4][2], const uint16_t* kb, int64_t rs, int k0,
                                            const RingTile& rt, int fr, int fg) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int r = k0 + 16 * mt + fr;
    const bool ok = rt.loads(r);
    const int rr = ok ? r : rt.start;  // a hidden slot never forms an address
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[mt][ks] = bf16x8_t{};
      if (ok) kf[mt][ks] = ld_frag(kb + rr * rs + 32 * ks + 8 * fg);
    }
  }
}

__device__ __forceinline__ void stage_v_ring(uint4* tile, const uint16_t* vb, int64_t rs, int k0, const RingTile& rt,
                                             int lane) {
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = 32 * it + w * 8 + (lane >> 3);
      const int r = k0 + row;
      const int ch = (lane & 7) ^ aswz(row);
      const void* src = rt.loads(r) ? (const void*)(vb + (int64_t)r * rs + ch * 8) : (const void*)g_tile_zero;
      glds16(src, tile + (32 * it + w * 8) * 8);
    }
}

// FP8 cache (csrc/attn_fp8.h): a row is 64 codes.  Which rows a wave loads is decided exactly as above --
// by [lo, hi) (lo = the split's start without a window) or by RingTile -- through one predicate:
struct RowsLoaded {
  bool win, ring;
  int lo, hi;
  RingTile rt;
  __device__ __forceinline__ bool operator()(int r) const { return ring ? rt.loads(r) : (r < hi && (!win || r >= lo)); }
  __device__ __forceinline__ int first() const { return ring ? rt.start : lo; }  // what a hidden row's index becomes
};

// load_k on codes: a lane's 8 B of a key row, converted (exactly) to the bf16x8 fragment the MFMA takes
__device__ __forceinline__ void load_k_fp8(bf16x8_t (&kf)[4][2], const uint8_t* kb, int64_t rs, int k0,
                                           const RowsLoaded& see, int fr, int fg) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int r = k0 + 16 * mt + fr;
    const bool ok = see(r);
    const int rr = ok ? r : see.first();  // a hidden row never forms an address
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint2 c = make_uint2(0, 0);  // the code of +0: a zero fragment
      if (ok) c = *reinterpret_cast<const uint2*>(kb + rr * rs + 32 * ks + 8 * fg);
      kf[mt][ks] = __builtin_bit_cast(bf16x8_t, fp8_to_bf16x8(c));
    }
  }
}

// V rows k0 .. k0 + 63 as codes into registers: pass j holds row 8 j + (lane >> 3), dims 8 (lane & 7) .. + 7
// (a wave load is 8 rows x 64 B); hidden rows are the zero code and form no address
__device__ __forceinline__ void load_v_fp8(uint2 (&vn)[8], const uint8_t* vb, int64_t rs, int k0,
                                           const RowsLoaded& see, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = k0 + 8 * j + (lane >> 3);
    vn[j] = make_uint2(0, 0);
    if (see(r)) vn[j] = *reinterpret_cast<const uint2*>(vb + (int64_t)r * rs + (lane & 7) * 8);
  }
}

// ... and from there to the swizzled bf16 tile stage_tile would have filled: chunk c of row r at c ^ aswz(r)
__device__ __forceinline__ void store_v_fp8(uint4* tile, const uint2 (&vn)[8], int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = 8 * j + (lane >> 3);
    tile[row * 8 + ((lane & 7) ^ aswz(row))] = fp8_to_bf16x8(vn[j]);
  }
}

// grid: B * H * nqt * nsplit one-wave workgroups, split fastest
template <bool WIN, bool RING = false, bool FP8 = false>
__global__ __launch_bounds__(64) void attn_extend_split_k(AttnExtendArgs a) {
  __shared__ __attribute__((aligned(16))) uint4 lds[2 * kTileU4];  // V, double buffered: 16 KiB
  const int lane = threadIdx.x;
  const int fr = lane & 15, fg = lane >> 4;
  const int part = blockIdx.x;
  const int sp = part % a.nsplit;
  int r = part / a.nsplit;
  const int qt = r % a.nqt;
  r /= a.nqt;
  const int h = r % a.H, b = r / a.H;
  const int q0 = qt * kQT;
  const int start = sp * a.split;  // host: nsplit * split < 2^31
  // the tile's largest limit (L grows with t) cut to the split: workgroup-uniform
  // RING: hi is the split's end in SLOTS, lo its start; what is visible is decided per slot from the
  // distances of RingTile, whose bounds are the tile's logical limits: dlo from its last query's upper
  // limit, dhi from its first query's lower limit (both monotone in t)
  RingTile rt{};
  int64_t rn = 0;  // L(b, T - 1), unclamped
  if constexpr (RING) {
    rn = max((int64_t)a.pos[b] + a.T, (int64_t)1);
    const int64_t l0 = max((int64_t)a.pos[b] + q0 + 1, (int64_t)1);
    const int64_t l1 = max((int64_t)a.pos[b] + min(q0 + kQT, a.T), (int64_t)1);
    rt.pm = ring_newest(rn, a.cap), rt.R = a.cap, rt.start = start, rt.hi = min(start + a.split, a.cap);
    rt.dlo = (int)(rn - l1), rt.dhi = (int)min(rn, rn - l0 + a.window);  // 0 <= dlo < dhi <= T - 1 + W <= R
  }
  const int hi = RING ? rt.hi : min(extend_len(a.pos, b, min(q0 + kQT, a.T) - 1, a.cap), start + a.split);
  float* wm = a.ws + (int64_t)a.nparts * (kQT * 64);
  float* wl = wm + (int64_t)a.nparts * kQT;
  // the tile's smallest lower limit (its first query's) raised to the split: workgroup-uniform, < hi
  // in a live split
  const int lo = WIN && !RING ? max(start, extend_len(a.pos, b, q0, a.cap) - a.window) : start;
  bool empty;  // workgroup-uniform
  if constexpr (RING) empty = !ring_any(rt.pm, rt.dlo, rt.dhi, start, hi, a.cap);
  else empty = start >= hi || (WIN && lo >= hi);
  if (empty) {
    if (lane < kQT) {
      wm[(int64_t)part * kQT + lane] = -INFINITY;
      wl[(int64_t)part * kQT + lane] = 0.f;
    }
    return;
  }
  const int qi = q0 + fr;
  const bool qreal = qi < a.T;
  // the lane's own query; RING: in distances -- it sees the slots with lim <= d(p) < low (lim from its
  // upper limit L, low from its lower one: the names keep their roles, the order flips with the distance)
  int lim, low;
  if constexpr (RING) {
    const int64_t lq = max((int64_t)a.pos[b] + (qreal ? qi : a.T - 1) + 1, (int64_t)1);
    lim = (int)(rn - lq);
    low = (int)min(rn, rn - lq + a.window);
  } else {
    lim = min(extend_len(a.pos, b, qreal ? qi : a.T - 1, a.cap), hi);
    // its lower limit (0 without a window): keys below it are masked
    low = WIN ? extend_len(a.pos, b, qreal ? qi : a.T - 1, a.cap) - a.window : 0;
  }

  // Qᵀ as the B operand: lane holds Q[q0 + fr][32 ks + 8 fg .. + 7]
  bf16x8_t qf[2];
  {
    const uint16_t* qp = a.q + b * a.sq[0] + (qreal ? qi : 0) * a.sq[1] + h * a.sq[2] + 8 * fg;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = qreal ? ld_frag(qp + 32 * ks) : bf16x8_t{};
  }
  const float c = a.scale * kLog2e;
  const int hk = h / a.group;  // grouped-query attention: the G heads of a group read the same rows
  const uint16_t* kb = a.k + b * a.sk[0] + hk * a.sk[1];
  const uint16_t* vb = a.v + b * a.sv[0] + hk * a.sv[1];

  f32x4_t acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  bf16x8_t kn[4][2];
  // tiles run from the 64-row tile of the split that holds lo (start itself without a window)
  // (a ring hides at most R - W slots: its tiles run from the split's start)
  const int kbeg = WIN && !RING ? start + (lo - start) / kTile * kTile : start;
  // FP8: K fragments and V codes of tile i + 1 are loaded into registers ahead of tile i's products (the
  // double buffering of the bf16 path, in registers where that one's V goes straight to LDS); tile i's V
  // codes are converted and written to its LDS buffer at the top of its iteration
  [[maybe_unused]] uint2 vn[8];
  [[maybe_unused]] const RowsLoaded see{WIN, RING, lo, hi, rt};
  [[maybe_unused]] const uint8_t* kb8 = reinterpret_cast<const uint8_t*>(a.k) + b * a.sk[0] + hk * a.sk[1];
  [[maybe_unused]] const uint8_t* vb8 = reinterpret_cast<const uint8_t*>(a.v) + b * a.sv[0] + hk * a.sv[1];
  if constexpr (FP8) {
    load_k_fp8(kn, kb8, a.sk[2], kbeg, see, fr, fg);
    load_v_fp8(vn, vb8, a.sv[2], kbeg, see, lane);
  } else if constexpr (RING) {
    load_k_ring(kn, kb, a.sk[2], kbeg, rt, fr, fg);
    stage_v_ring(lds, vb, a.sv[2], kbeg, rt, lane);
  } else {
    load_k<WIN>(kn, kb, a.sk[2], kbeg, lo, hi, fr, fg);
    stage_v<WIN>(lds, vb, a.sv[2], kbeg, lo, hi, lane);
  }
  int buf = 0;
  for (int k0 = kbeg; k0 < hi; k0 += kTile, buf ^= 1) {
    if constexpr (FP8) store_v_fp8(lds + buf * kTileU4, vn, lane);  // the buffer's last reads: two tiles ago
    else wait_loads();
    __syncthreads();  // tile k0 landed (registers and LDS); the other buffer's reads are done
    bf16x8_t kf[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[mt][ks] = kn[mt][ks];
    if (k0 + kTile < hi) {
      if constexpr (FP8) {
        load_k_fp8(kn, kb8, a.sk[2], k0 + kTile, see, fr, fg);
        load_v_fp8(vn, vb8, a.sv[2], k0 + kTile, see, lane);
      } else if constexpr (RING) {
        load_k_ring(kn, kb, a.sk[2], k0 + kTile, rt, fr, fg);
        stage_v_ring(lds + (buf ^ 1) * kTileU4, vb, a.sv[2], k0 + kTile, rt, lane);
      } else {
        load_k<WIN>(kn, kb, a.sk[2], k0 + kTile, lo, hi, fr, fg);
        stage_v<WIN>(lds + (buf ^ 1) * kTileU4, vb, a.sv[2], k0 + kTile, lo, hi, lane);
      }
    }
    const uint4* Vt = lds + buf * kTileU4;

    f32x4_t s[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      s[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) s[mt] = mfma(kf[mt][ks], qf[ks], s[mt]);
    }
    // s[mt][i]: key k0 + 16 mt + 4 fg + i, query fr.  Hidden keys -> -inf; rows at or past hi were
    // zeros in both operands, rows in [lim, hi) real data.
    const int key0 = k0 + 4 * fg;
    float mx = -INFINITY;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = key0 + 16 * mt + i;
        bool see;
        if constexpr (RING) {
          const int d = ring_back(rt.pm, key, rt.R);
          see = key < hi && d >= lim && d < low;
        } else {
          see = key < lim && (!WIN || key >= low);
        }
        s[mt][i] = see ? s[mt][i] * c : -INFINITY;
        mx = fmaxf(mx, s[mt][i]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    // a row that has seen no key yet (mn = -inf) must not form -inf - -inf (under a window that is
    // any row whose lower limit lies past this tile, not only one that sees nothing in the split; in a
    // ring, any row whose up to two slot intervals both lie past this tile).  A tile in which a row
    // sees nothing AFTER it has seen a key has mn = m finite: alpha = exp2(0), every p = exp2(-inf) = 0
    const float ms = mn == -INFINITY ? 0.f : mn;
    const float alpha = __builtin_amdgcn_exp2f(m - ms);  // m = -inf: 0, and acc, l are 0 anyway
    m = mn;
    float ls = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __builtin_amdgcn_exp2f(s[mt][i] - ms);  // hidden: exp2(-inf) = 0 exactly
        s[mt][i] = p;
        ls += p;
      }
    l = l * alpha + ls;  // lane-partial; summed over the 4 lane groups at the end
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] *= alpha;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8_t pf = pack_frag(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) acc[dt] = mfma(tr_frag(Vt, 32 * ks, dt, fr, fg), pf, acc[dt]);
    }
  }

  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  // acc[dt][i] = Oᵀ[16 dt + 4 fg + i][fr]
  if constexpr (FP8) {  // P.V ran on the unscaled codes
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] *= a.vscale;
  }
  if (a.nsplit == 1) {
    if (qreal) {  // the one split holds row L(b, t) - 1: l > 0
      const float inv = 1.f / l;
      uint16_t* op = a.o + b * a.so[0] + qi * a.so[1] + h * 64 + 4 * fg;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) st4(op + 16 * dt, acc[dt], inv);
    }
    return;
  }
  float* wo = a.ws + ((int64_t)part * kQT + fr) * 64 + 4 * fg;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<float4*>(wo + 16 * dt) = make_float4(acc[dt][0], acc[dt][1], acc[dt][2], acc[dt][3]);
  if (fg == 0) {
    wm[(int64_t)part * kQT + fr] = m;
    wl[(int64_t)part * kQT + fr] = l;
  }
}

// grid: B * T * H one-wave workgroups (head fastest); lane = output dim
__global__ __launch_bounds__(64) void attn_extend_merge_k(AttnExtendArgs a) {
  const int d = threadIdx.x;
  int r = blockIdx.x;
  const int h = r % a.H;
  r /= a.H;
  const int t = r % a.T, b = r / a.T;
  const int64_t part0 = (((int64_t)b * a.H + h) * a.nqt + t / kQT) * a.nsplit;
  const int row = t % kQT;
  const float* wo = a.ws + (part0 * kQT + row) * 64 + d;
  const float* wm = a.ws + (int64_t)a.nparts * (kQT * 64) + part0 * kQT + row;
  const float* wl = wm + (int64_t)a.nparts * kQT;
  float M = -INFINITY;
  for (int s = 0; s < a.nsplit; ++s) M = fmaxf(M, wm[s * kQT]);  // the split of row L(b, t) - 1 is never empty: finite
  float o = 0.f, L = 0.f;
  for (int s = 0; s < a.nsplit; ++s) {
    const float ms = wm[s * kQT];
    if (ms == -INFINITY) continue;  // empty split or a row that saw nothing: its o is never read
    const float f = __builtin_amdgcn_exp2f(ms - M);
    L = fmaf(f, wl[s * kQT], L);
    o = fmaf(f, wo[(int64_t)s * (kQT * 64)], o);
  }
  a.o[b * a.so[0] + t * a.so[1] + h * 64 + d] = f2bf(o / L);
}

}  // namespace

// The default policy, a function of (B, H, T, cap) only.  tiles = B * H * ceil(T / 16) one-wave
// workgroups.  With 256 tiles or more (one per CU) the keys are not split, so a long continuation
// needs no workspace of the order of T * cap.  Below that the keys are split 128 to a workgroup, and
// the split size doubles while tiles * nsplit exceeds 512: past two waves per CU more splits add
// partials and merge steps and no parallelism.  Measured (profiles/extend/README.md; us per call,
// median of 5 interleaved rounds, spread < 2 %; T = 8, H = 12, cap = len, pos = len - T):
//
//     B*H  len    tiles   64     128    256    512    one split
//     12   512    12      9.2    8.2    9.3    11.3   11.2
//     12   1024   12      12.7   10.1   10.2   14.0   20.2
//     96   512    96      11.6   9.8    10.3   11.7   11.6
//     96   1024   96      18.7   13.8   12.3   14.7   20.5
//
// T = 2 .. 16 differ from these by a few per cent (one tile whatever T is).  128 is the fastest or
// within 2 % of it in three rows; in the fourth (768 waves at 128) 256 wins by 8 .. 15 %, which is
// the doubling rule.  A single wave walks the keys at about 1.2 us per 64-key tile, which is what
// one split costs at len 1024.
static int g_extend_split = 0;  // 0: the default policy; otherwise a forced split size
constexpr int kExtendSplit = 128;
constexpr int kExtendFullTiles = 256;
constexpr int kExtendMaxWaves = 512;

int attn_extend_set_split(int n) {
  const int old = g_extend_split;
  if (n == 0 || (n >= 8 && n % 8 == 0)) g_extend_split = n;
  return old;
}

static int extend_split_size(int B, int H, int T, int cap) {
  if (g_extend_split) return g_extend_split < cap ? g_extend_split : cap;
  const int64_t tiles = (int64_t)B * H * ((T + kQT - 1) / kQT);
  if (tiles >= kExtendFullTiles) return cap;
  int s = kExtendSplit;
  while (s < cap && tiles * ((cap + s - 1) / s) > kExtendMaxWaves) s *= 2;  // s <= 2 * cap: no overflow
  return s < cap ? s : cap;
}

int attn_extend_splits(int B, int H, int T, int cap) {
  const int s = extend_split_size(B, H, T, cap);
  return (cap + s - 1) / s;
}

int64_t attn_extend_workspace(int B, int H, int T, int cap) {
  const int ns = attn_extend_splits(B, H, T, cap);
  if (ns == 1) return 0;
  return (int64_t)B * H * ((T + kQT - 1) / kQT) * ns * (kQT * 66);
}

void attn_extend(const AttnExtendArgs& a_, hipStream_t st) {
  AttnExtendArgs a = a_;
  if (a.B == 0 || a.T == 0) return;
  a.split = extend_split_size(a.B, a.H, a.T, a.cap);
  a.nsplit = (a.cap + a.split - 1) / a.split;
  a.nqt = (a.T + kQT - 1) / kQT;
  a.nparts = a.B * a.H * a.nqt * a.nsplit;
  a.group = a.H / a.Hkv;
  auto* split = a.ring ? attn_extend_split_k<true, true>
                       : (a.window > 0 ? attn_extend_split_k<true> : attn_extend_split_k<false>);
  if (a.fp8)
    split = a.ring ? attn_extend_split_k<true, true, true>
                   : (a.window > 0 ? attn_extend_split_k<true, false, true> : attn_extend_split_k<false, false, true>);
  hipLaunchKernelGGL(split, dim3(a.nparts), dim3(64), 0, st, a);
  if (a.nsplit > 1) hipLaunchKernelGGL(attn_extend_merge_k, dim3(a.B * a.T * a.H), dim3(64), 0, st, a);
}

}  // namespace tbamd
