// Device helpers shared by the few-row MXFP4 kernels (csrc/rows_gemm_mx.hip, csrc/rows_experts_mx.hip):
// the bf16 chunk packing, the MX block decode, the fold over the lanes of a column, and the staging of
// the input rows in LDS with the LayerNorm / RMSNorm prologue.  gfx950, wave64.
#pragma once
#include "common.h"

namespace tbamd {

constexpr int kMxWaves = 4;

__device__ __forceinline__ void mx_unpack8(const uint4& r, float (&v)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 mx_pack8(const float (&v)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(v[2 * i]) | ((uint32_t)f2bf(v[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void mx_load8f(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// eight codes (one dword: element 2t in the low nibble of byte t) times the block's scale byte sb.
// The conversion reads the exponent of its float operand as e8m0: right for 1 .. 254, but 0 would
// be 2^-127 and 255 NaN, where the format's rule here is f32_from_bits(sb << 23), a zero and +inf.
// Those two bytes (never produced by the quantiser) convert at scale 1 and multiply.
__device__ __forceinline__ void mx_decode8(uint32_t w, uint32_t sb, float (&v)[8]) {
  const bool plain = sb - 1u < 254u;
  const float scale = __uint_as_float(sb << 23);
  const float cs = plain ? scale : 1.f;
  const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, cs, 0);
  const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, cs, 1);
  const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, cs, 2);
  const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, cs, 3);
  v[0] = p0[0]; v[1] = p0[1]; v[2] = p1[0]; v[3] = p1[1];
  v[4] = p2[0]; v[5] = p2[1]; v[6] = p3[0]; v[7] = p3[1];
  if (!plain) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] *= scale;
  }
}

// Sum each of the first N values of v over the lanes that differ in the bits O, O / 2, .. 1.  While
// N > 1 a stage sends half of the values to the partner lane and keeps the other half; base
// advances to the index of the value the lane then holds in v[0].  With no stage left the lane
// holds values base .. base + N - 1; once N is 1 the value is replicated over the later stages.
template <int NV, int N, int O>
__device__ __forceinline__ void mx_fold(float (&v)[NV], int lane, int& base) {
  if constexpr (O >= 1) {
    if constexpr (N > 1) {
      constexpr int h = N / 2;
      const bool up = (lane & O) != 0;
#pragma unroll
      for (int i = 0; i < h; ++i) {
        const float send = up ? v[i] : v[i + h];
        const float keep = up ? v[i + h] : v[i];
        v[i] = keep + __shfl_xor(send, O, 64);
      }
      base += up ? h : 0;
      mx_fold<NV, h, O / 2>(v, lane, base);
    } else {
      v[0] += __shfl_xor(v[0], O, 64);
      mx_fold<NV, 1, O / 2>(v, lane, base);
    }
  }
}

// where the 16-B chunk v of a row lives in its LDS row: quarter-major, blocks consecutive
__device__ __forceinline__ int mx_pos(int v, int nb) { return (v & 3) * nb + (v >> 2); }

// The M rows of x (row stride sx, K % 32 == 0) into xs [M][K / 8] chunks of 8 bf16 at mx_pos, then the
// LayerNorm (gamma and beta) or RMSNorm (gamma, rms) prologue on them, one wave per row, with the
// statistics and roundings of rows_linear_k.  Called by all 64 * kMxWaves threads; ends synchronised.
__device__ __forceinline__ void mx_stage_rows(uint4* xs, const uint16_t* x, int64_t sx, int M, int K,
                                              const float* gamma, const float* beta, int rms, float eps) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nv = K >> 3, nb = K >> 5;
  // ---- the M rows into LDS, raw
  for (int i = tid; i < M * nv; i += 64 * kMxWaves) {
    const int m = i / nv, v = i - m * nv;
    uint4 r = make_uint4(0, 0, 0, 0);
    if (TB_BOUNDS_OK(m < M && v * 8 + 8 <= K, kBndGemmSrc))
      r = *reinterpret_cast<const uint4*>(x + (int64_t)m * sx + v * 8);
    xs[m * nv + mx_pos(v, nb)] = r;
  }
  __syncthreads();
  // ---- LayerNorm / RMSNorm prologue: one wave per row, each lane rewrites only the chunks it read
  if (gamma && rms) {  // workgroup-uniform
    const float inv = 1.f / (float)K;
    for (int m = wid; m < M; m += kMxWaves) {
      uint4* row = xs + m * nv;
      float s = 0.f;
      for (int v = lane; v < nv; v += 64) {
        float f[8];
        mx_unpack8(row[mx_pos(v, nb)], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) s += f[k] * f[k];
      }
      const float rs = rsqrtf(wave_sum(s) * inv + eps);
      for (int v = lane; v < nv; v += 64) {
        float f[8], g[8];
        mx_unpack8(row[mx_pos(v, nb)], f);
        mx_load8f(gamma + v * 8, g);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = f[k] * rs * g[k];
        row[mx_pos(v, nb)] = mx_pack8(f);
      }
    }
    __syncthreads();
  } else if (gamma) {
    const float inv = 1.f / (float)K;
    for (int m = wid; m < M; m += kMxWaves) {
      uint4* row = xs + m * nv;
      float s = 0.f;
      for (int v = lane; v < nv; v += 64) {
        float f[8];
        mx_unpack8(row[mx_pos(v, nb)], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) s += f[k];
      }
      const float mu = wave_sum(s) * inv;
      s = 0.f;
      for (int v = lane; v < nv; v += 64) {
        float f[8];
        mx_unpack8(row[mx_pos(v, nb)], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = f[k] - mu;
          s += d * d;
        }
      }
      const float rs = rsqrtf(wave_sum(s) * inv + eps);
      for (int v = lane; v < nv; v += 64) {
        float f[8], g[8], b[8];
        mx_unpack8(row[mx_pos(v, nb)], f);
        mx_load8f(gamma + v * 8, g);
        mx_load8f(beta + v * 8, b);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = (f[k] - mu) * rs * g[k] + b[k];
        row[mx_pos(v, nb)] = mx_pack8(f);
      }
    }
    __syncthreads();
  }
}

}  // namespace tbamd
