// QK-norm of a packed q | k | v projection fused with its rotary embedding, bf16, head dim 64, gfx950:
// the NORM instantiation of rope_packed_k (rope_kernel.h; csrc/rope.hip describes it) and its backward.
//
//   qk_norm_rope_bwd_k    the backward of the above from the saved input x and g = dL/dy (tbamd.h has
//                   the formulas).  A capped, shape-only grid; a workgroup (64 quads) walks a contiguous
//                   range of head vectors, 64 per pass, a quad per vector.  As a lane owns the same 16
//                   columns in every pass it keeps the weight-gradient terms u * x^ in registers, one
//                   set of 16 for query heads and one for key heads.  Behind the walk the workgroup
//                   copies its share of the value part of g, then folds its 64 quads through LDS in
//                   quad order into one [64] partial for each weight, and col_sum2 (layernorm.hip) adds
//                   the partials over workgroups in a fixed order: no atomics, every output element
//                   written once, the same bits on every run.
#include "rope_kernel.h"

namespace tbamd {
namespace {

constexpr int kQkBwdMaxBlocks = 1024;  // 4 workgroups per CU
constexpr int kQkRedPitch = 132;        // 2 x 64 columns of a quad, padded

__global__ __launch_bounds__(256) void qk_norm_rope_bwd_k(QkNormRopeBwdArgs a) {
  __shared__ float red[64][kQkRedPitch];
  const int tid = threadIdx.x, c = tid & 3, quad = tid >> 2;
  const int hr = a.H + a.Hkv;
  const int64_t rows = (int64_t)a.B * a.T;
  const int64_t nvec = rows * hr;
  const int64_t width = (int64_t)(hr + a.Hkv) * 64;
  const int64_t per = (nvec + gridDim.x - 1) / gridDim.x;
  const int64_t v0 = blockIdx.x * per;
  const int64_t v1 = v0 + per < nvec ? v0 + per : nvec;
  float aq1[8], aq2[8], ak1[8], ak2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) aq1[k] = aq2[k] = ak1[k] = ak2[k] = 0.f;
  for (int64_t base = v0; base < v1; base += 64) {
    int64_t r = base + quad;  // the quad's head vector: all four lanes or none
    if (r >= v1) continue;
    const int h = (int)(r % hr);
    r /= hr;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    int64_t p = (a.pos ? (int64_t)a.pos[b] : 0) + t;
    p = p < 0 ? 0 : (p >= a.max_len ? (int64_t)a.max_len - 1 : p);
    const int64_t col = (int64_t)h * 64 + c * 8;
    // (a failed check still takes the quad as a whole: every term but c is the same in its lanes)
    if (!TB_BOUNDS_OK(r < rows && col + 40 <= (int64_t)hr * 64 &&
                          (!a.tab || p * 64 + 32 + c * 8 + 8 <= (int64_t)a.max_len * 64),
                      kBndAnySrc))
      continue;
    const uint16_t* xs = a.x + b * a.sx[0] + t * a.sx[1] + col;
    const uint16_t* gs = a.g + b * a.sg[0] + t * a.sg[1] + col;
    const uint4 xlo = *reinterpret_cast<const uint4*>(xs), xhi = *reinterpret_cast<const uint4*>(xs + 32);
    const uint4 glo = *reinterpret_cast<const uint4*>(gs), ghi = *reinterpret_cast<const uint4*>(gs + 32);
    const bool isq = h < a.H;
    const float* w = (isq ? a.qw : a.kw) + c * 8;
    float x1[8], x2[8], u1[8], u2[8], w1[8], w2[8];
    rope_load8f(w, w1);
    rope_load8f(w + 32, w2);
    rope_unpack8(xlo, x1);
    rope_unpack8(xhi, x2);
    rope_unpack8(glo, u1);
    rope_unpack8(ghi, u2);
    if (a.tab) {  // u = the inverse rotation of g
      float cs[8], sn[8];
      rope_load8f(a.tab + p * 64 + c * 8, cs);
      rope_load8f(a.tab + p * 64 + 32 + c * 8, sn);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float g1 = u1[k], g2 = u2[k];
        u1[k] = fmaf(g2, sn[k], g1 * cs[k]);
        u2[k] = fmaf(-g1, sn[k], g2 * cs[k]);
      }
    }
    const float rstd = rope_rstd(x1, x2, a.eps);
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      x1[k] *= rstd;  // x^
      w1[k] *= u1[k];  // gw
      dot = fmaf(w1[k], x1[k], dot);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      x2[k] *= rstd;
      w2[k] *= u2[k];
      dot = fmaf(w2[k], x2[k], dot);
    }
    const float m = rope_quad_sum(dot) * (1.f / 64.f);
    float d1[8], d2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      d1[k] = rstd * fmaf(-x1[k], m, w1[k]);
      d2[k] = rstd * fmaf(-x2[k], m, w2[k]);
      const float e1 = u1[k] * x1[k], e2 = u2[k] * x2[k];
      aq1[k] += isq ? e1 : 0.f;
      aq2[k] += isq ? e2 : 0.f;
      ak1[k] += isq ? 0.f : e1;
      ak2[k] += isq ? 0.f : e2;
    }
    if (TB_BOUNDS_OK(r < rows && col + 40 <= width, kBndAnyDst)) {
      uint16_t* dst = a.dx + b * a.sdx[0] + t * a.sdx[1] + col;
      *reinterpret_cast<uint4*>(dst) = rope_pack8(d1);
      *reinterpret_cast<uint4*>(dst + 32) = rope_pack8(d2);
    }
  }
  // the value part of g, 16 B per lane and step: (row, chunk of Hkv * 8)
  const int nv = a.Hkv * 8;
  for (int64_t id = (int64_t)blockIdx.x * 256 + tid; id < rows * nv; id += (int64_t)gridDim.x * 256) {
    const int v = (int)(id % nv);
    const int64_t r = id / nv;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    const int64_t col = (int64_t)hr * 64 + v * 8;
    if (TB_BOUNDS_OK(r < rows && col + 8 <= width, kBndAnyDst))
      *reinterpret_cast<uint4*>(a.dx + b * a.sdx[0] + t * a.sdx[1] + col) =
          *reinterpret_cast<const uint4*>(a.g + b * a.sg[0] + t * a.sg[1] + col);
  }
  // fold the 64 quads in quad order: thread j < 128 owns column j & 63 of the query (j < 64) or key set
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    red[quad][c * 8 + k] = aq1[k];
    red[quad][32 + c * 8 + k] = aq2[k];
    red[quad][64 + c * 8 + k] = ak1[k];
    red[quad][96 + c * 8 + k] = ak2[k];
  }
  __syncthreads();
  if (tid < 128) {
    float s = 0.f;
    for (int q = 0; q < 64; ++q) s += red[q][tid];
    // part: [2][gridDim.x][64]
    a.part[((int64_t)(tid >> 6) * gridDim.x + blockIdx.x) * 64 + (tid & 63)] = s;
  }
}

}  // namespace

void qk_norm_rope_packed(const QkNormRopeArgs& a, hipStream_t st) {
  const int64_t rows = (int64_t)a.B * a.T;
  const int64_t total = rows * (a.H + a.Hkv) * 4 + (a.copy_v ? rows * a.Hkv * 8 : 0);
  if (total == 0) return;
  hipLaunchKernelGGL(rope_packed_k<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

int qk_norm_rope_bwd_blocks(int64_t nvec) {
  const int64_t b = (nvec + 63) / 64;  // a pass of 64 head vectors per workgroup at least
  return (int)(b < 1 ? 1 : (b > kQkBwdMaxBlocks ? kQkBwdMaxBlocks : b));
}

void qk_norm_rope_packed_bwd(const QkNormRopeBwdArgs& a, hipStream_t st) {
  const int nblk = qk_norm_rope_bwd_blocks((int64_t)a.B * a.T * (a.H + a.Hkv));
  hipLaunchKernelGGL(qk_norm_rope_bwd_k, dim3(nblk), dim3(256), 0, st, a);
  col_sum2(a.part, a.part + (int64_t)nblk * 64, nblk, 64, a.dqw, a.dkw, st);
}

}  // namespace tbamd
