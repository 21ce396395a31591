// SwiGLU gate of a packed gate | up projection, bf16 / f32, gfx950.
//
// Not in the reference (it has no transformer).  gu holds rows [gate (F) | up (F)], the
// output of ONE Linear(dim, 2F), as the packed q | k | v of the attention is the output of one:
//   y[c]     = silu(g[c]) * u[c]                       g = gu[c], u = gu[F + c], silu(g) = g * s(g)
//   dgate[c] = dy[c] * u[c] * s(g) * (1 + g * (1 - s(g)))     s = the logistic function
//   dup[c]   = dy[c] * silu(g[c])
//
//   swiglu_fwd_k / swiglu_bwd_k   one lane per 16 B of the OUTPUT row (8 bf16 or 4 f32): it loads its
//                   gate vector and the partner F elements on (the backward: dy too), computes in f32
//                   and rounds once at the store.  The backward recomputes everything from gu and
//                   writes dgate | dup [M][2F] in the same launch.
//
// Memory-bound elementwise work: every access is a 16-B vector, rows may be strided (a window of a
// wider tensor) as long as they stay 16-B aligned.  The grid is a function of (M, F) only; no atomics,
// no workspace, nothing read on the host, every output element written exactly once: deterministic
// and capturable.
#include "common.h"
#include "tbamd.h"

namespace tbamd {
namespace {

// W elements = 16 B
template <int DT> struct Vec16;
template <> struct Vec16<kBF16> {
  static constexpr int W = 8;
  __device__ __forceinline__ static void load(const uint16_t* p, float (&v)[8]) { Vec8<kBF16>::load(p, v); }
  __device__ __forceinline__ static void store(uint16_t* p, const float (&v)[8]) { Vec8<kBF16>::store(p, v); }
};
template <> struct Vec16<kF32> {
  static constexpr int W = 4;
  __device__ __forceinline__ static void load(const float* p, float (&v)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  }
  __device__ __forceinline__ static void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

__device__ __forceinline__ float logistic_f(float x) { return 1.f / (1.f + __expf(-x)); }

template <int DT>
__global__ __launch_bounds__(256) void swiglu_fwd_k(const storage_t<DT>* __restrict__ gu, int64_t sgu, int64_t M,
                                                    int F, storage_t<DT>* __restrict__ y) {
  constexpr int W = Vec16<DT>::W;
  const int nv = F / W;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= M * nv) return;
  const int64_t m = id / nv;
  const int c = (int)(id - m * nv) * W;
  if (!TB_BOUNDS_OK(m < M && c + W <= F, kBndAnySrc)) return;
  float g[W], u[W], o[W];
  Vec16<DT>::load(gu + m * sgu + c, g);
  Vec16<DT>::load(gu + m * sgu + F + c, u);
#pragma unroll
  for (int k = 0; k < W; ++k) o[k] = g[k] * logistic_f(g[k]) * u[k];
  if (TB_BOUNDS_OK(m * F + c + W <= M * F, kBndAnyDst)) Vec16<DT>::store(y + m * F + c, o);
}

template <int DT>
__global__ __launch_bounds__(256) void swiglu_bwd_k(const storage_t<DT>* __restrict__ gu, int64_t sgu,
                                                    const storage_t<DT>* __restrict__ dy, int64_t M, int F,
                                                    storage_t<DT>* __restrict__ dgu) {
  constexpr int W = Vec16<DT>::W;
  const int nv = F / W;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= M * nv) return;
  const int64_t m = id / nv;
  const int c = (int)(id - m * nv) * W;
  if (!TB_BOUNDS_OK(m < M && c + W <= F, kBndAnySrc)) return;
  float g[W], u[W], d[W], dg[W], du[W];
  Vec16<DT>::load(gu + m * sgu + c, g);
  Vec16<DT>::load(gu + m * sgu + F + c, u);
  Vec16<DT>::load(dy + m * F + c, d);
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const float s = logistic_f(g[k]);
    dg[k] = d[k] * u[k] * s * (1.f + g[k] * (1.f - s));
    du[k] = d[k] * (g[k] * s);
  }
  if (TB_BOUNDS_OK((m * 2 + 1) * F + c + W <= M * 2 * F, kBndAnyDst)) {
    Vec16<DT>::store(dgu + m * 2 * F + c, dg);
    Vec16<DT>::store(dgu + m * 2 * F + F + c, du);
  }
}

template <int DT>
unsigned swiglu_grid(int64_t M, int F) {
  return (unsigned)((M * (F / Vec16<DT>::W) + 255) / 256);
}

}  // namespace

void swiglu_forward(int dt, const void* gu, int64_t sgu, int64_t M, int F, void* y, hipStream_t st) {
  if (M == 0 || F == 0) return;
  if (dt == kBF16)
    swiglu_fwd_k<kBF16><<<swiglu_grid<kBF16>(M, F), 256, 0, st>>>((const uint16_t*)gu, sgu, M, F, (uint16_t*)y);
  else
    swiglu_fwd_k<kF32><<<swiglu_grid<kF32>(M, F), 256, 0, st>>>((const float*)gu, sgu, M, F, (float*)y);
}

void swiglu_backward(int dt, const void* gu, int64_t sgu, const void* dy, int64_t M, int F, void* dgu,
                     hipStream_t st) {
  if (M == 0 || F == 0) return;
  if (dt == kBF16)
    swiglu_bwd_k<kBF16><<<swiglu_grid<kBF16>(M, F), 256, 0, st>>>((const uint16_t*)gu, sgu, (const uint16_t*)dy, M,
                                                                  F, (uint16_t*)dgu);
  else
    swiglu_bwd_k<kF32><<<swiglu_grid<kF32>(M, F), 256, 0, st>>>((const float*)gu, sgu, (const float*)dy, M, F,
                                                                (float*)dgu);
}

}  // namespace tbamd
