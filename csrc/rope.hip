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
//   rope_packed_k<true>   QK-norm ahead of the rotation, same lane map: the four lanes of a head hold its
//                   64 elements in f32, 16 each.  A lane sums its 16 squares in a fixed order, the quad
//                   adds them with two __shfl_xor (1, 2; every lane gets the same bits), and the lane
//                   scales its elements by rstd = rsqrt(mean + eps) and by its 16 weights (two 32-B
//                   loads from qw for h < H, from kw behind) before the same product + fma rotation: the
//                   normalised vector is never rounded or stored.  A null table skips the rotation.
//                   Loads and shuffles come before the stores and the 64 elements belong to this quad
//                   alone, so y may alias x as above.
//
// The kernel is a template in rope_kernel.h.  This file instantiates rope_packed_k<false>, which compiles
// to what it was before the norm existed; csrc/qk_norm_rope.hip instantiates rope_packed_k<true> next to
// its backward and is compiled without packed f32 instructions (torchbooster_amd/_build.py).
//
// p = clamp(pos[b] + t, 0, max_len - 1), pos read from device memory once per lane (0 without pos):
// the rule of embed_rows_k, a bad position never becomes an address.  The grid is a function of
// (B, T, H, Hkv, copy_v) only; nothing is read on the host, no atomics, no workspace, every output
// element written exactly once: deterministic and capturable.
#include "rope_kernel.h"

namespace tbamd {

void rope_packed(const RopeArgs& a, hipStream_t st) {
  const int64_t rows = (int64_t)a.B * a.T;
  const int64_t total = rows * (a.H + a.Hkv) * 4 + (a.copy_v ? rows * a.Hkv * 8 : 0);
  if (total == 0) return;
  hipLaunchKernelGGL(rope_packed_k<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace tbamd
