// Few-row products on MXFP4 expert stacks and the fused router of an MoE decode step, gfx950, wave64.
//
// Not in the reference.  A decode step of a mixture-of-experts MLP multiplies each of its 1 .. 16
// (token, slot) pairs with the weight of the expert the router chose for it.  The weights are the
// stacked experts in MXFP4 (csrc/rows_gemm_mx.hip: codes [E][Qw][K / 2], scales [E][Qw][K / 32]) and
// the choice is a device tensor: nothing is read on the host, and the grid depends on (Q, K) only.
//
//   rows_experts_mx_k   one template for both products of an expert MLP, with the walk of
//                   rows_linear_mx_k: 4 waves, the input rows staged and normalised in LDS at
//                   mx_pos, a wave a panel of LC columns x LB block-lanes, two weight rows per
//                   walk, one 16-B load one MX block, mx_decode8, the mx_fold butterfly.
//                   New is that the weight is chosen per pair.  One wave of every workgroup reads the
//                   P = M * top_k ids, clamps them into [0, E) (a bad id never becomes an address:
//                   the rule of embed_rows) and builds in LDS the ascending list of the distinct
//                   experts, each with the bit mask of its pairs.  A wave then loops, for its columns,
//                   over that list: it streams the weight rows of a used expert once and multiplies
//                   them with that expert's pairs only (the mask is wave-uniform; one f32
//                   accumulator per (walk slot, pair) and lane).  Weight traffic is (#distinct
//                   experts) x Qw x K x 4.25 bit however many pairs share an expert.
//                   Pair mode (kPair, kPairGlu): x [M][K], pair p reads staged row p / top_k, and
//                   y[p][c] is the pair's product (silu(gate) * up under kPairGlu); the prologues are
//                   those of rows_linear_mx_k.  Combine mode (kCombine): x [P][K], pair p reads row
//                   p; after the fold the per-pair f32 sums of the walk's columns go through a
//                   per-wave LDS scratch, and one lane per (column, token) adds gates[m][j] * sum in
//                   slot order j = 0, 1, .. onto the f32 residual (or 0) and stores once.
//   moe_route_k     one workgroup per row: the row staged and normalised in LDS as rows_linear_k
//                   does, the waves take the router's columns round-robin (16-B chunks per lane, then
//                   wave_sum: a column's summation order does not depend on the wave), the logits
//                   go to LDS, and wave 0 selects with top_k argmax passes over (value, index), ties
//                   to the lower index, and writes the ids and the f32 softmax over the chosen logits.
//
// Determinism and row invariance.  A pair's K order is fixed by (lane % LB, block) and the fold is
// mx_fold's: pair (m, j) of pair mode has the bits of rows_linear_mx_k on row m alone with expert
// e's weight, and in either mode token m has the same bits alone or among other tokens, whatever
// experts those chose.  No atomics, no workspace, every output element written exactly once.
#include "common.h"
#include "rows_mx.h"
#include "tbamd.h"

namespace tbamd {
namespace {

enum : int { kPair = 0, kPairGlu = 1, kCombine = 2 };
constexpr int kMaxPairs = 16;

// order the LDS traffic of one wave: what its lanes wrote before is what they read after
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// PB: pairs the accumulators are laid out for (P <= PB); LB: lanes per column
template <int PB, int LB, int MODE>
__global__ __launch_bounds__(64 * kMxWaves) void rows_experts_mx_k(RowsExpertsMxArgs a) {
  extern __shared__ uint4 xs[];  // [rows][K / 8] chunks of 8 bf16, at mx_pos; kCombine: then the scratch
  __shared__ int s_exp[kMaxPairs];        // the distinct experts, ascending
  __shared__ uint32_t s_mask[kMaxPairs];  // bit p: pair p goes to that expert
  __shared__ int s_ne;
  constexpr bool GLU = MODE == kPairGlu, COMB = MODE == kCombine;
  constexpr int NV = 2 * PB;
  constexpr int LC = 64 / LB;             // columns per panel
  constexpr int CO = GLU ? LC : 2 * LC;   // output columns per walk
  constexpr int R = NV > LB ? NV / LB : 1;    // values a lane holds after the fold
  constexpr int REP = LB > NV ? LB / NV : 1;  // lanes holding the same value
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nv = a.K >> 3, nb = a.K >> 5;
  const int P = a.M * a.top_k;
  const int rows = COMB ? P : a.M;

  // ---- the expert list, by the last wave while the others begin to stage
  if (wid == kMxWaves - 1) {
    int e = INT32_MAX;  // no pair
    if (lane < P) {
      e = a.ids[lane];
      e = e < 0 ? 0 : e > a.E - 1 ? a.E - 1 : e;
    }
    uint32_t same = 0;
    for (int t = 0; t < P; ++t) same |= (__shfl(e, t, 64) == e ? 1u : 0u) << t;
    const bool first = lane < P && (same & ((1u << (lane & 31)) - 1u)) == 0;
    int rank = 0;  // distinct experts below this one
    for (int t = 0; t < P; ++t) {
      const int v = __shfl(e, t, 64), f = __shfl((int)first, t, 64);
      rank += (f && v < e) ? 1 : 0;
    }
    if (first) {
      s_exp[rank] = e;
      s_mask[rank] = same;
    }
    const unsigned long long firsts = __ballot(first);
    if (lane == 0) s_ne = __popcll(firsts);
  }
  // ---- the rows into LDS, normalised there; its barrier also publishes the list
  mx_stage_rows(xs, a.x, a.sx, rows, a.K, a.gamma, a.beta, a.rms, a.eps);
  const int ne = __builtin_amdgcn_readfirstlane(s_ne);
  int xr[PB];  // where pair p's row starts in xs
#pragma unroll
  for (int p = 0; p < PB; ++p) xr[p] = (COMB ? p : p / a.top_k) * nv;
  float* scr = reinterpret_cast<float*>(xs + rows * nv) + wid * (2 * LC * PB);  // kCombine: [2 * LC][PB]

  // ---- this wave's columns
  const int bl = lane & (LB - 1), cl = lane / LB;
  const int64_t col0 = ((int64_t)blockIdx.x * kMxWaves + wid) * a.cpw;
  const int64_t cend = col0 + a.cpw < (int64_t)a.Q ? col0 + a.cpw : (int64_t)a.Q;
  const int64_t wrows = GLU ? 2 * (int64_t)a.Q : (int64_t)a.Q;
  const int nr = (nb + LB - 1) / LB;  // blocks per lane and weight row
  for (int64_t c0 = col0; c0 < cend; c0 += CO) {
    // walk slot s: output column oc[s] from weight row wr[s]
    int64_t oc[2], wr[2];
    oc[0] = c0 + cl;
    oc[1] = GLU ? oc[0] : oc[0] + LC;
    wr[0] = oc[0];
    wr[1] = GLU ? (int64_t)a.Q + oc[1] : oc[1];
    float acc[NV];  // (slot, pair) at slot * PB + pair
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int ei = 0; ei < ne; ++ei) {
      const int e = __builtin_amdgcn_readfirstlane(s_exp[ei]);
      const uint32_t pm = __builtin_amdgcn_readfirstlane(s_mask[ei]);
      const bool eok = e >= 0 && e < a.E;
      const uint8_t* ce = a.codes + (eok ? (int64_t)e : 0) * wrows * (a.K >> 1);
      const uint8_t* se = a.scales + (eok ? (int64_t)e : 0) * wrows * nb;
      for (int r0 = 0; r0 < nr; r0 += 2) {
        uint4 cd[2][2];
        uint32_t sb[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int b = bl + LB * (r0 + u);
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            cd[u][s] = make_uint4(0, 0, 0, 0);
            sb[u][s] = 127u;
            // an expert or a column out of range or a block past K never forms an address
            if (b < nb && oc[s] < cend &&
                TB_BOUNDS_OK(eok && wr[s] < wrows && b * 32 + 32 <= a.K, kBndGemmSrc)) {
              cd[u][s] = *reinterpret_cast<const uint4*>(ce + wr[s] * (a.K >> 1) + b * 16);
              sb[u][s] = se[wr[s] * nb + b];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int b = bl + LB * (r0 + u);
          if (b < nb) {
            const uint32_t cw[2][4] = {{cd[u][0].x, cd[u][0].y, cd[u][0].z, cd[u][0].w},
                                       {cd[u][1].x, cd[u][1].y, cd[u][1].z, cd[u][1].w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float wf[2][8];
#pragma unroll
              for (int s = 0; s < 2; ++s) mx_decode8(cw[s][j], sb[u][s], wf[s]);
#pragma unroll
              for (int p = 0; p < PB; ++p) {
                if ((pm >> p) & 1u) {  // wave-uniform: this expert's pairs only
                  float xf[8];
                  mx_unpack8(xs[xr[p] + j * nb + b], xf);
#pragma unroll
                  for (int s = 0; s < 2; ++s) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[s * PB + p] = fmaf(xf[k], wf[s][k], acc[s * PB + p]);
                  }
                }
              }
            }
          }
        }
      }
    }
    int base = 0;
    mx_fold<NV, NV, LB / 2>(acc, lane, base);
    const bool owner = (bl & (REP - 1)) == 0;
    if constexpr (GLU) {
      // value base + i is (slot, pair) = ((base + i) / PB, (base + i) % PB): the first stage puts the
      // gate half in the lanes with bit LB / 2 clear and pair p's up sum in the lane across it
      constexpr int RG = LB == 1 ? PB : R;
#pragma unroll
      for (int i = 0; i < RG; ++i) {
        float g = acc[i], u;
        if constexpr (LB == 1) u = acc[PB + i];
        else u = __shfl_xor(acc[i], LB / 2, 64);
        const int p = base + i;
        if (owner && p < PB && p < P && oc[0] < cend) {
          const int64_t o = (int64_t)p * a.Q + oc[0];
          if (TB_BOUNDS_OK(o < (int64_t)P * a.Q, kBndGemmDst)) a.y[o] = f2bf(silu_f(g) * u);
        }
      }
    } else if constexpr (!COMB) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int idx = base + i, s = idx / PB, p = idx - s * PB;
        const int64_t col = s ? oc[1] : oc[0];
        if (owner && p < P && col < cend) {
          const int64_t o = (int64_t)p * a.Q + col;
          if (TB_BOUNDS_OK(o < (int64_t)P * a.Q, kBndGemmDst)) a.y[o] = f2bf(acc[i]);
        }
      }
    } else {
      // the pairs' f32 sums of the walk's 2 * LC columns, then one lane per (column, token)
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int idx = base + i, s = idx / PB, p = idx - s * PB;
        if (owner && p < P) scr[(s * LC + cl) * PB + p] = acc[i];
      }
      wave_lds_sync();
      for (int t = lane; t < 2 * LC * a.M; t += 64) {
        const int cs = t / a.M, m = t - cs * a.M;
        const int64_t col = c0 + cs;  // slot cs / LC, panel column cs % LC
        if (col < cend) {
          float z = a.res ? bf2f(a.res[(int64_t)m * a.sres + col]) : 0.f;
          for (int j = 0; j < a.top_k; ++j)
            z = fmaf(a.gates[m * a.top_k + j], scr[cs * PB + m * a.top_k + j], z);
          const int64_t o = (int64_t)m * a.Q + col;
          if (TB_BOUNDS_OK(o < (int64_t)a.M * a.Q, kBndGemmDst)) a.y[o] = f2bf(z);
        }
      }
      wave_lds_sync();
    }
  }
}

// the combine scratch behind the staged rows: [kMxWaves][2 * LC][PB] f32
template <int PB, int LB>
constexpr size_t experts_scratch() { return (size_t)kMxWaves * 2 * (64 / LB) * PB * sizeof(float); }

template <int PB, int LB, int MODE>
void ex_launch(const RowsExpertsMxArgs& a, int grid, hipStream_t st) {
  // up to 16 x 4096 bf16 = 128 KiB of the CU's 160 KiB (plus 512 B of scratch at LB = 64): above the
  // default limit of a launch, raised once per device at the first launch there (the warm-up step,
  // ahead of any capture)
  static bool raised[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev >= 0 && dev < 64 && !raised[dev]) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rows_experts_mx_k<PB, LB, MODE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 16 * 4096 * 2 + 512);
    raised[dev] = true;
  }
  const int rows = MODE == kCombine ? a.M * a.top_k : a.M;
  const size_t lds = (size_t)rows * a.K * 2 + (MODE == kCombine ? experts_scratch<PB, LB>() : 0);
  hipLaunchKernelGGL((rows_experts_mx_k<PB, LB, MODE>), dim3(grid), dim3(64 * kMxWaves), lds, st, a);
}

template <int LB, int MODE>
void ex_pairs(const RowsExpertsMxArgs& a, int grid, hipStream_t st) {
  const int P = a.M * a.top_k;
  if (P <= 1) ex_launch<1, LB, MODE>(a, grid, st);
  else if (P <= 2) ex_launch<2, LB, MODE>(a, grid, st);
  else if (P <= 4) ex_launch<4, LB, MODE>(a, grid, st);
  else if (P <= 8) ex_launch<8, LB, MODE>(a, grid, st);
  else ex_launch<16, LB, MODE>(a, grid, st);
}

template <int MODE>
void ex_panel(const RowsExpertsMxArgs& a, int lb, int grid, hipStream_t st) {
  switch (lb) {
    case 1: return ex_pairs<1, MODE>(a, grid, st);
    case 2: return ex_pairs<2, MODE>(a, grid, st);
    case 4: return ex_pairs<4, MODE>(a, grid, st);
    case 8: return ex_pairs<8, MODE>(a, grid, st);
    case 16: return ex_pairs<16, MODE>(a, grid, st);
    case 32: return ex_pairs<32, MODE>(a, grid, st);
    default: return ex_pairs<64, MODE>(a, grid, st);
  }
}

// ------------------------------------------------------------------------------------ the router
constexpr int kRouteMaxE = 256;
constexpr int kRouteMaxTop = 16;

__device__ __forceinline__ void route_unpack8(const uint4& r, float (&v)[8]) { mx_unpack8(r, v); }

// (ov, oi) ahead of (bv, bi): the larger value, ties to the lower index; INT32_MAX is no candidate
__device__ __forceinline__ bool route_ahead(float ov, int oi, float bv, int bi) {
  return oi != INT32_MAX && (bi == INT32_MAX || ov > bv || (ov == bv && oi < bi));
}

__global__ __launch_bounds__(64 * kMxWaves) void moe_route_k(MoeRouteArgs a) {
  extern __shared__ uint4 xs[];  // the row: [K / 8] chunks of 8 bf16
  __shared__ float s_logit[kRouteMaxE];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nv = a.K >> 3, m = blockIdx.x;
  for (int v = tid; v < nv; v += 64 * kMxWaves) {
    uint4 r = make_uint4(0, 0, 0, 0);
    if (TB_BOUNDS_OK(m < a.M && v * 8 + 8 <= a.K, kBndGemmSrc))
      r = *reinterpret_cast<const uint4*>(a.x + (int64_t)m * a.sx + v * 8);
    xs[v] = r;
  }
  __syncthreads();
  // ---- the prologue of rows_linear_k, by wave 0: the same statistics, one rounding to bf16
  if (a.gamma) {  // workgroup-uniform
    if (wid == 0) {
      const float inv = 1.f / (float)a.K;
      float s = 0.f, mu = 0.f;
      if (!a.rms) {
        for (int v = lane; v < nv; v += 64) {
          float f[8];
          route_unpack8(xs[v], f);
#pragma unroll
          for (int k = 0; k < 8; ++k) s += f[k];
        }
        mu = wave_sum(s) * inv;
        s = 0.f;
      }
      for (int v = lane; v < nv; v += 64) {
        float f[8];
        route_unpack8(xs[v], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = f[k] - mu;  // mu is 0 under RMSNorm: f[k] itself
          s += d * d;
        }
      }
      const float rs = rsqrtf(wave_sum(s) * inv + a.eps);
      for (int v = lane; v < nv; v += 64) {
        float f[8], g[8];
        route_unpack8(xs[v], f);
        mx_load8f(a.gamma + v * 8, g);
        if (a.rms) {
#pragma unroll
          for (int k = 0; k < 8; ++k) f[k] = f[k] * rs * g[k];
        } else {
          float b[8];
          mx_load8f(a.beta + v * 8, b);
#pragma unroll
          for (int k = 0; k < 8; ++k) f[k] = (f[k] - mu) * rs * g[k] + b[k];
        }
        xs[v] = mx_pack8(f);
      }
    }
    __syncthreads();
  }
  // ---- the logits: a wave per router row, round-robin; the order of a sum is (lane, chunk) then wave_sum
  for (int e = wid; e < a.E; e += kMxWaves) {
    float s = 0.f;
    for (int v = lane; v < nv; v += 64) {
      float h[8], w[8];
      route_unpack8(xs[v], h);
      uint4 r = make_uint4(0, 0, 0, 0);
      if (TB_BOUNDS_OK(e < a.E && v * 8 + 8 <= a.K, kBndGemmSrc))
        r = *reinterpret_cast<const uint4*>(a.w + (int64_t)e * a.K + v * 8);
      route_unpack8(r, w);
#pragma unroll
      for (int k = 0; k < 8; ++k) s = fmaf(h[k], w[k], s);
    }
    s = wave_sum(s);
    if (lane == 0 && e < kRouteMaxE) s_logit[e] = s;
  }
  __syncthreads();
  if (wid != 0) return;
  // ---- top_k argmax passes by wave 0: lane l holds the logits l, l + 64, l + 128, l + 192
  float lv[kRouteMaxE / 64];
  bool taken[kRouteMaxE / 64];
#pragma unroll
  for (int i = 0; i < kRouteMaxE / 64; ++i) {
    const int e = lane + 64 * i;
    lv[i] = e < a.E ? s_logit[e] : 0.f;
    taken[i] = e >= a.E;
  }
  float top0 = 0.f, sum = 0.f, mine = 0.f;  // lane j keeps exp(top_j - top_0)
  for (int j = 0; j < a.top_k; ++j) {
    float bv = 0.f;
    int bi = INT32_MAX;
#pragma unroll
    for (int i = 0; i < kRouteMaxE / 64; ++i) {
      const int e = taken[i] ? INT32_MAX : lane + 64 * i;
      if (route_ahead(lv[i], e, bv, bi)) bv = lv[i], bi = e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (route_ahead(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    bv = __shfl(bv, 0, 64);
    bi = __shfl(bi, 0, 64);
    bi = bi < 0 ? 0 : bi > a.E - 1 ? a.E - 1 : bi;  // top_k <= E leaves a candidate; never out of [0, E)
#pragma unroll
    for (int i = 0; i < kRouteMaxE / 64; ++i) taken[i] = taken[i] || lane + 64 * i == bi;
    if (j == 0) top0 = bv;
    const float ex = expf(bv - top0);
    sum += ex;
    if (lane == j) mine = ex;
    if (lane == 0 && TB_BOUNDS_OK(m < a.M && j < a.top_k, kBndGemmDst)) a.ids[m * a.top_k + j] = bi;
  }
  if (lane < a.top_k && TB_BOUNDS_OK(m < a.M, kBndGemmDst)) a.gates[m * a.top_k + lane] = mine / sum;
}

}  // namespace

void rows_experts_mx(const RowsExpertsMxArgs& a_, hipStream_t st) {
  RowsExpertsMxArgs a = a_;
  const bool glu = a.glu != 0 && !a.gates;
  a.cpw = rows_mx_cols_per_wave(a.Q, a.K, glu);
  const int64_t per_wg = (int64_t)a.cpw * kMxWaves;
  const int grid = (int)((a.Q + per_wg - 1) / per_wg);
  const int lb = rows_mx_block_lanes(a.K);
  if (a.gates) ex_panel<kCombine>(a, lb, grid, st);
  else if (glu) ex_panel<kPairGlu>(a, lb, grid, st);
  else ex_panel<kPair>(a, lb, grid, st);
}

void moe_route(const MoeRouteArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(moe_route_k, dim3(a.M), dim3(64 * kMxWaves), (size_t)a.K * 2, st, a);
}

}  // namespace tbamd
