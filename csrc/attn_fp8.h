// FP8 KV cache: the quantiser and the dequantiser shared by csrc/attention_decode.hip and
// csrc/attention_extend.hip.
//
// A cache row of an fp8 layer is 64 OCP e4m3 codes (torch.float8_e4m3fn: 254 finite codes, maximum 448, no
// infinities; gfx950 converts this format, not fnuz, in hardware).  One rule on every path:
//
//     code = rne_e4m3(clamp(f32(x) * inv, -448, 448)),   inv = float32(1 / scale)   (host, from double)
//     x'   = f32(code) * f32(scale)
//
// The clamp is an explicit f32 min / max ahead of v_cvt_pk_fp8_f32, so nothing depends on what the
// conversion does on overflow and +-inf saturate to +-448; a NaN is passed through unclamped and the
// conversion makes it a NaN code.  f32(code) is exact, and exact in bf16 too (4 significant bits), which is
// what lets the extend kernel feed dequantised codes to the bf16 MFMA; the scales are never applied per
// element by the kernels: k_scale rides in the score factor and v_scale multiplies the f32 accumulator once.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

namespace tbamd {

typedef float fp8_f32x2_t __attribute__((ext_vector_type(2)));

constexpr float kFp8Max = 448.f;

__device__ __forceinline__ float fp8_clamp(float y) {
  return y != y ? y : fminf(fmaxf(y, -kFp8Max), kFp8Max);
}

// 8 bf16 (16 B) -> 8 codes (8 B), element i to byte i
__device__ __forceinline__ uint2 fp8_quant8(const uint4& r, float inv) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  float f[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = fp8_clamp(__uint_as_float(w[i] << 16) * inv);
    f[2 * i + 1] = fp8_clamp(__uint_as_float(w[i] & 0xffff0000u) * inv);
  }
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

// 8 codes -> 8 floats (unscaled)
__device__ __forceinline__ void fp8_unpack8(const uint2& r, float (&v)[8]) {
  const uint32_t w[2] = {r.x, r.y};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const fp8_f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const fp8_f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    v[4 * i] = a[0], v[4 * i + 1] = a[1], v[4 * i + 2] = b[0], v[4 * i + 3] = b[1];
  }
}

// 8 codes -> 8 bf16 (16 B), exact: the upper halves of the floats
__device__ __forceinline__ uint4 fp8_to_bf16x8(const uint2& r) {
  float v[8];
  fp8_unpack8(r, v);
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (__float_as_uint(v[2 * i]) >> 16) | (__float_as_uint(v[2 * i + 1]) & 0xffff0000u);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace tbamd
