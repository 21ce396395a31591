// Few-row products on MXFP4 weights (1 <= M <= 16 rows), gfx950, wave64.
//
// Not in the reference.  The decode product of csrc/rows_gemm.hip with the weight in the OCP
// microscaling format MXFP4: blocks of 32 e2m1 codes along K (element 2i in the low nibble of byte
// i) and one e8m0 scale byte per block, value = e2m1(code) * f32_from_bits(scale << 23).  The
// weight stream is 4.25 bits per element instead of 16; x, bias, residual and y stay bf16.
//
//   rows_linear_mx_k   y[M, Q] = epilogue(prologue(x)[M, K] . dq(codes, scales)[Q, K]^T + bias).
//                   A workgroup is 4 waves.  It stages the M rows of x in LDS as bf16 and runs the
//                   LayerNorm / RMSNorm prologue there, one wave per row, with the statistics and
//                   roundings of rows_linear_k.  The one difference is where a 16-B chunk lands:
//                   chunk v = 4 * b + j of a row (block b, quarter j) is stored at j * (K / 32) + b,
//                   so the lanes of a column, which hold consecutive blocks, read consecutive 16 B.
//                   The walk.  One 16-B load is one MX block: the lane that loads it also loads
//                   the block's scale byte and reads the block's 32 x values from LDS.  The 64
//                   lanes of a wave are a panel of LC columns x LB block-lanes (LB * LC = 64, LB
//                   the smallest power of two >= min(K / 32, 64), a template parameter chosen on
//                   the host from K alone): lane l holds blocks (l % LB) + LB * i of column l / LB.
//                   K = 768 is two columns at 24 of 32 lanes each, K = 512 four full columns,
//                   K = 4096 one column and two blocks per lane.  A wave walks two weight rows at
//                   a time (two panels of LC columns; under SwiGLU the gate and the up row of the
//                   same LC columns), so a bf16 quarter of x read from LDS and unpacked once
//                   feeds 16 fmaf, and four loads are in flight per lane.
//                   Decoding is v_cvt_scalef32_pk_f32_fp4: one byte and the block's scale as a
//                   float give two scaled f32 values, 16 conversions per block and weight row
//                   whatever M is.  The scale is a power of two, so the scaled weight is exact
//                   and every product enters the f32 fmaf chain as the reference's does.
//                   The 2 * MB per-lane sums are folded over the LB lanes of a column: stages
//                   xor LB / 2 .. 1, each halving the live values while there is more than one
//                   (rows_gemm.hip's fold_sum, over LB lanes instead of 64).  What is left in a
//                   lane, max(1, 2 * MB / LB) values, gets bias, GELU, residual or the SwiGLU
//                   pairing (gate and up differ in lane bit LB / 2: one shuffle) in f32 and one
//                   bf16 store.
//
// Determinism and row invariance.  The K order of a sum is fixed by (lane % LB, block), the fold
// gives every value what a plain butterfly in the order LB / 2 .. 1 gives it (a + b is b + a bit
// for bit), and LB is a function of K: row m has the same bits computed alone or among 16 rows.
// No atomics, no workspace, every output element written exactly once; the grid depends on (Q, K)
// only and nothing is read on the host.
//
// Scale bytes 0 and 255 are never produced by ops.linear.mx_quantize; they read as a zero scale and
// as +inf, the rule of ops.linear.mx_dequantize (mx_decode8).
#include "common.h"
#include "rows_mx.h"
#include "tbamd.h"

namespace tbamd {
namespace {

// MB: rows the accumulators are laid out for (M <= MB); LB: lanes per column; GLU: the SwiGLU
// epilogue (the two weight rows of a walk are the gate and the up row of one column)
template <int MB, int LB, bool GLU>
__global__ __launch_bounds__(64 * kMxWaves) void rows_linear_mx_k(RowsLinearMxArgs a) {
  extern __shared__ uint4 xs[];  // [M][K / 8] chunks of 8 bf16, at mx_pos
  constexpr int NV = 2 * MB;
  constexpr int LC = 64 / LB;             // columns per panel
  constexpr int CO = GLU ? LC : 2 * LC;   // output columns per walk
  constexpr int R = NV > LB ? NV / LB : 1;    // values a lane holds after the fold
  constexpr int REP = LB > NV ? LB / NV : 1;  // lanes holding the same value
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nv = a.K >> 3, nb = a.K >> 5;

  // ---- the M rows into LDS, normalised there (rows_mx.h)
  mx_stage_rows(xs, a.x, a.sx, a.M, a.K, a.gamma, a.beta, a.rms, a.eps);

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
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
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
          // a column past the wave's range or a block past K never forms an address
          if (b < nb && oc[s] < cend && TB_BOUNDS_OK(wr[s] < wrows && b * 32 + 32 <= a.K, kBndGemmSrc)) {
            cd[u][s] = *reinterpret_cast<const uint4*>(a.codes + wr[s] * (a.K >> 1) + b * 16);
            sb[u][s] = a.scales[wr[s] * nb + b];
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
            for (int m = 0; m < MB; ++m) {
              if (m < a.M) {  // wave-uniform
                float xf[8];
                mx_unpack8(xs[m * nv + j * nb + b], xf);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
#pragma unroll
                  for (int k = 0; k < 8; ++k) acc[s * MB + m] = fmaf(xf[k], wf[s][k], acc[s * MB + m]);
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
      // value base + i is (slot, row) = ((base + i) / MB, (base + i) % MB): the first stage puts the
      // gate half in the lanes with bit LB / 2 clear and row m's up sum in the lane across it
      constexpr int RG = LB == 1 ? MB : R;
#pragma unroll
      for (int i = 0; i < RG; ++i) {
        float g = acc[i], u;
        if constexpr (LB == 1) u = acc[MB + i];
        else u = __shfl_xor(acc[i], LB / 2, 64);
        const int m = base + i;
        if (owner && m < MB && m < a.M && oc[0] < cend) {
          if (a.bias) {
            g += bf2f(a.bias[oc[0]]);
            u += bf2f(a.bias[(int64_t)a.Q + oc[0]]);
          }
          const int64_t o = (int64_t)m * a.Q + oc[0];
          if (TB_BOUNDS_OK(o < (int64_t)a.M * a.Q, kBndGemmDst)) a.y[o] = f2bf(silu_f(g) * u);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int idx = base + i, s = idx / MB, m = idx - s * MB;
        const int64_t col = s ? oc[1] : oc[0];
        if (owner && m < a.M && col < cend) {
          float z = acc[i];
          if (a.bias) z += bf2f(a.bias[col]);
          if (a.epi == kRowsGelu) z = gelu_f(z);
          else if (a.epi == kRowsResidual) z += bf2f(a.res[(int64_t)m * a.sres + col]);
          const int64_t o = (int64_t)m * a.Q + col;
          if (TB_BOUNDS_OK(o < (int64_t)a.M * a.Q, kBndGemmDst)) a.y[o] = f2bf(z);
        }
      }
    }
  }
}

template <int MB, int LB, bool GLU>
void mx_launch(const RowsLinearMxArgs& a, int grid, size_t lds, hipStream_t st) {
  // up to 16 x 4096 bf16 = 128 KiB of the CU's 160 KiB: above the default limit of a launch, raised
  // once per device at the first launch there (the warm-up step, ahead of any capture)
  static bool raised[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev >= 0 && dev < 64 && !raised[dev]) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rows_linear_mx_k<MB, LB, GLU>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 16 * 4096 * 2);
    raised[dev] = true;
  }
  hipLaunchKernelGGL((rows_linear_mx_k<MB, LB, GLU>), dim3(grid), dim3(64 * kMxWaves), lds, st, a);
}

template <int LB, bool GLU>
void mx_rows(const RowsLinearMxArgs& a, int grid, size_t lds, hipStream_t st) {
  if (a.M <= 1) mx_launch<1, LB, GLU>(a, grid, lds, st);
  else if (a.M <= 2) mx_launch<2, LB, GLU>(a, grid, lds, st);
  else if (a.M <= 4) mx_launch<4, LB, GLU>(a, grid, lds, st);
  else if (a.M <= 8) mx_launch<8, LB, GLU>(a, grid, lds, st);
  else mx_launch<16, LB, GLU>(a, grid, lds, st);
}

template <bool GLU>
void mx_panel(const RowsLinearMxArgs& a, int lb, int grid, size_t lds, hipStream_t st) {
  switch (lb) {
    case 1: return mx_rows<1, GLU>(a, grid, lds, st);
    case 2: return mx_rows<2, GLU>(a, grid, lds, st);
    case 4: return mx_rows<4, GLU>(a, grid, lds, st);
    case 8: return mx_rows<8, GLU>(a, grid, lds, st);
    case 16: return mx_rows<16, GLU>(a, grid, lds, st);
    case 32: return mx_rows<32, GLU>(a, grid, lds, st);
    default: return mx_rows<64, GLU>(a, grid, lds, st);
  }
}

}  // namespace

// Lanes per column: the smallest power of two >= min(K / 32, 64).
int rows_mx_block_lanes(int K) {
  const int nb = K / 32;
  int lb = 1;
  while (lb < 64 && lb < nb) lb *= 2;
  return lb;
}

// Output columns per wave, from (Q, K) alone (Q is F under SwiGLU): a walk covers 2 * 64 / LB columns
// (64 / LB under SwiGLU, two weight rows each) and a wave takes 1, 2, 4, 8 or 16 walks, aiming at
// about two workgroups per CU as rows_linear_cols_per_wave does.
int rows_mx_cols_per_wave(int Q, int K, bool glu) {
  const int lc = 64 / rows_mx_block_lanes(K);
  const int per_walk = glu ? lc : 2 * lc;
  const int64_t unit = (int64_t)kMxWaves * per_walk * 512;
  const int64_t want = ((int64_t)Q + unit - 1) / unit;
  const int walks = want <= 1 ? 1 : want <= 2 ? 2 : want <= 4 ? 4 : want <= 8 ? 8 : 16;
  return per_walk * walks;
}

void rows_linear_mx(const RowsLinearMxArgs& a_, hipStream_t st) {
  RowsLinearMxArgs a = a_;
  const bool glu = a.epi == kRowsSwiglu;
  a.cpw = rows_mx_cols_per_wave(a.Q, a.K, glu);
  const int64_t per_wg = (int64_t)a.cpw * kMxWaves;
  const int grid = (int)((a.Q + per_wg - 1) / per_wg);
  const size_t lds = (size_t)a.M * a.K * 2;
  if (glu) mx_panel<true>(a, rows_mx_block_lanes(a.K), grid, lds, st);
  else mx_panel<false>(a, rows_mx_block_lanes(a.K), grid, lds, st);
}

}  // namespace tbamd
