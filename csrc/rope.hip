// Rotary position embedding of a packed q | k | v projection, bf16, head dim 64, gfx950.
//
// Not in the reference (it has no attention model).  Rotate-half (GPT-NeoX / Llama)
// layout: with c / s the cosine / sine of position p at frequency i (i = 0 .. 31) from a host-built
// f32 table [max_len][2][32] (cosines, then sines),
//   y[i]      = x[i] * c - x[i + 32] * s
//   y[i + 32] = x[i + 32] * c + x[i] * s          (inverse: -s, the transpose = the gradient).
//
//   rope_packed_k   one lane per 16 B of the LOW half of a rotated head: (row = b * T + t, head,
//                   chunk) with head over the H query heads and then the Hkv key heads, which follow
//                   each other in a packed row, and 4 chunks per head.  The lane loads 8 bf16 at
//                   i .. i + 7, their 8 partners at i + 32 .., 8 cosines and 8 sines (two 32-B f32
//                   loads), forms both outputs in f32 with one product and one fma each, rounds once
//                   and stores two 16-B vectors.  Both inputs are in registers before either output
//                   is stored and no other lane touches these 32 elements, so y may alias x.
//                   The lanes past the rotated ones (out of place only: copy_v) copy the value part,
//                   16 B each, bit for bit: one launch per call.  In place the value part is not read.
//
// p = clamp(pos[b] + t, 0, max_len - 1), pos read from device memory once per lane (0 without pos):
// the rule of embed_rows_k, a bad position never becomes an address.  The grid is a function of
// (B, T, H, Hkv, copy_v) only; nothing is read on the host, no atomics, no workspace, every output
// element written exactly once: deterministic and capturable.
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

__global__ __launch_bounds__(256) void rope_packed_k(RopeArgs a) {
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
    rope_load8f(a.tab + p * 64 + c * 8, cs);
    rope_load8f(a.tab + p * 64 + 32 + c * 8, sn);
    float y1[8], y2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float s = a.inverse ? -sn[k] : sn[k];
      y1[k] = fmaf(-x2[k], s, x1[k] * cs[k]);
      y2[k] = fmaf(x1[k], s, x2[k] * cs[k]);
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

void rope_packed(const RopeArgs& a, hipStream_t st) {
  const int64_t rows = (int64_t)a.B * a.T;
  const int64_t total = rows * (a.H + a.Hkv) * 4 + (a.copy_v ? rows * a.Hkv * 8 : 0);
  if (total == 0) return;
  hipLaunchKernelGGL(rope_packed_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace tbamd
