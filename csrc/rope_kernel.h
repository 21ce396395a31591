// The kernel of csrc/rope.hip (NORM = false) and csrc/qk_norm_rope.hip (NORM = true): see rope.hip.
#pragma once
#include "common.h"
#include "tbamd.h"

namespace tbamd {
namespace {


__device__ __forceinline__ void rope_unpack8(const uint4& r, float (&v)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 rope_pack8(const float (&v)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(v[2 * i]) | ((uint32_t)f2bf(v[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void rope_load8f(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

template <bool NORM> struct RopeKernelArgs { using type = RopeArgs; };
template <> struct RopeKernelArgs<true> { using type = QkNormRopeArgs; };

// the sum of a lane's 16 values over the 4 lanes of its head, the same bits in each of them
__device__ __forceinline__ float rope_quad_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}

// sum of the 16 squares in a fixed order -> rstd of the head
__device__ __forceinline__ float rope_rstd(const float (&x1)[8], const float (&x2)[8], float eps) {
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) ss = fmaf(x1[k], x1[k], ss);
#pragma unroll
  for (int k = 0; k < 8; ++k) ss = fmaf(x2[k], x2[k], ss);
  return rsqrtf(rope_quad_sum(ss) * (1.f / 64.f) + eps);
}

template <bool NORM>
__global__ __launch_bounds__(256) void rope_packed_k(typename RopeKernelArgs<NORM>::type a) {
  const int hr = a.H + a.Hkv;  // rotated heads of a row
  const int64_t rows = (int64_t)a.B * a.T;
  const int64_t nrot = rows * hr * 4;
  const int64_t width = (int64_t)(hr + a.Hkv) * 64;  // elements of a packed row
  int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id < nrot) {
    const int c = (int)(id & 3);
    int64_t r = id >> 2;
    const int h = (int)(r % hr);
    r /= hr;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    int64_t p = (a.pos ? (int64_t)a.pos[b] : 0) + t;
    p = p < 0 ? 0 : (p >= a.max_len ? (int64_t)a.max_len - 1 : p);  // never an address out of range
    const int64_t col = (int64_t)h * 64 + c * 8;
    if (!TB_BOUNDS_OK(r < rows && col + 40 <= (int64_t)hr * 64 && p * 64 + 32 + c * 8 + 8 <= (int64_t)a.max_len * 64,
                      kBndAnySrc))
      return;
    const uint16_t* src = a.x + b * a.sx[0] + t * a.sx[1] + col;
    const uint4 lo = *reinterpret_cast<const uint4*>(src);
    const uint4 hi = *reinterpret_cast<const uint4*>(src + 32);
    float x1[8], x2[8], cs[8], sn[8];
    rope_unpack8(lo, x1);
    rope_unpack8(hi, x2);
    float y1[8], y2[8];
    if constexpr (NORM) {
      float w1[8], w2[8];
      const float* w = (h < a.H ? a.qw : a.kw) + c * 8;
      rope_load8f(w, w1);
      rope_load8f(w + 32, w2);
      const float rstd = rope_rstd(x1, x2, a.eps);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        x1[k] = x1[k] * rstd * w1[k];
        x2[k] = x2[k] * rstd * w2[k];
      }
    }
    if (NORM && !a.tab) {
#pragma unroll
      for (int k = 0; k < 8; ++k) y1[k] = x1[k], y2[k] = x2[k];
    } else {
      rope_load8f(a.tab + p * 64 + c * 8, cs);
      rope_load8f(a.tab + p * 64 + 32 + c * 8, sn);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float s = !NORM && a.inverse ? -sn[k] : sn[k];
        y1[k] = fmaf(-x2[k], s, x1[k] * cs[k]);
        y2[k] = fmaf(x1[k], s, x2[k] * cs[k]);
      }
    }
    if (TB_BOUNDS_OK(r < rows && col + 40 <= width, kBndAnyDst)) {
      uint16_t* dst = a.y + b * a.sy[0] + t * a.sy[1] + col;
      *reinterpret_cast<uint4*>(dst) = rope_pack8(y1);
      *reinterpret_cast<uint4*>(dst + 32) = rope_pack8(y2);
    }
    return;
  }
  // the value part, 16 B per lane: (row, chunk of Hkv * 8)
  id -= nrot;
  const int nv = a.Hkv * 8;
  if (!a.copy_v || id >= rows * nv) return;
  const int v = (int)(id % nv);
  const int64_t r = id / nv;
  const int t = (int)(r % a.T);
  const int b = (int)(r / a.T);
  const int64_t col = (int64_t)hr * 64 + v * 8;
  if (TB_BOUNDS_OK(r < rows && col + 8 <= width, kBndAnyDst))
    *reinterpret_cast<uint4*>(a.y + b * a.sy[0] + t * a.sy[1] + col) =
        *reinterpret_cast<const uint4*>(a.x + b * a.sx[0] + t * a.sx[1] + col);
}

}  // namespace
}  // namespace tbamd
