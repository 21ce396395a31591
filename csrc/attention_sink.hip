// The gradient of the attention sinks (AttnArgs::sinks; csrc/attention.hip), gfx950, wave64.
//
// A sink is a per-head logit s_h in every row's softmax denominator with no value row.  The forward's stored
// log-sum-exp includes it, so dQ / dK / dV are what the backward kernels already compute from lse and
// delta = rowsum(dO * O), and the sink's own gradient needs nothing but those two row vectors:
//
//   dL/ds_h = sum over rows of p_sink * (dP_sink - delta) = -sum over b, i < N of exp(s_h - lse[b][h][i]) * delta[b][h][i]
//
// (dP_sink = dO . 0 = 0).  Rows at padded positions are rows like any other: the caller masks their loss, so
// their dO and delta are zero.
//
//   attn_bwd_dsink_k  one workgroup of 16 waves per head -- the grid is a function of H alone -- walks the
//                     head's B * N (lse, delta) pairs, both f32 [B][H][N]: element e = b * N + i belongs to
//                     thread e mod 1024 and to its accumulator (e / 1024) mod 4, a map that depends on nothing
//                     but e, with 4 coalesced 4-KiB loads of each vector in flight.  The 4 accumulators are
//                     added pairwise, the 64 lanes of a wave by xor-shuffles (32 .. 1), the 16 wave sums
//                     through LDS by thread 0 in wave order: a fixed tree, no atomics, dsinks[h] written
//                     once, the same bits on every run.
//
// Launched behind the dQ pass, which writes delta.  The stream is 8 * B * N bytes per head, a few per cent of
// what the dQ pass reads; it is built without packed f32 instructions.
#include "common.h"
#include "tbamd.h"

namespace tbamd {
namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kSinkThreads = 1024, kSinkWaves = kSinkThreads / 64, kSinkUnroll = 4;

__global__ __launch_bounds__(kSinkThreads) void attn_bwd_dsink_k(AttnArgs a) {
  __shared__ float part[kSinkWaves];
  const int tid = threadIdx.x, h = blockIdx.x;
  const int64_t N = a.N, total = (int64_t)a.B * N;
  const float s2 = a.sinks[h] * kLog2e;
  float sum[kSinkUnroll];
#pragma unroll
  for (int u = 0; u < kSinkUnroll; ++u) sum[u] = 0.f;
  for (int64_t e0 = tid; e0 < total; e0 += kSinkThreads * kSinkUnroll) {
    float lv[kSinkUnroll], dl[kSinkUnroll];
#pragma unroll
    for (int u = 0; u < kSinkUnroll; ++u) {
      const int64_t e = e0 + u * kSinkThreads;
      const bool ok = e < total;
      const int64_t b = ok ? e / N : 0, i = ok ? e - b * N : 0;  // past the end: element 0, selected away below
      const int64_t off = (b * a.H + h) * N + i;
      const float lse = a.lse[off], delta = a.delta[off];
      lv[u] = ok ? lse : INFINITY;  // exp2(-inf) = 0
      dl[u] = ok ? delta : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kSinkUnroll; ++u)
      sum[u] = __builtin_fmaf(__builtin_amdgcn_exp2f(__builtin_fmaf(-lv[u], kLog2e, s2)), dl[u], sum[u]);
  }
  float s = (sum[0] + sum[1]) + (sum[2] + sum[3]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < kSinkWaves; ++w) t += part[w];
    a.dsinks[h] = -t;
  }
}

}  // namespace

void attn_bwd_dsink(const AttnArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(attn_bwd_dsink_k, dim3(a.H), dim3(kSinkThreads), 0, st, a);
}

}  // namespace tbamd
