// Few-row products for decoding (1 <= M <= 16 rows), bf16, gfx950, wave64.
//
// Not in the reference (it has no attention model).  A decode step multiplies one to
// sixteen activation rows by every weight of the model: the MFMA engine of csrc/gemm.hip has tiles
// of 128 - 256 rows and nothing to do there.  The product is a streaming read of the weight, so the
// kernels here are shaped like csrc/attention_decode.hip, not like a GEMM.
//
//   rows_linear_k   y[M, Q] = epilogue(prologue(x)[M, K] . W[Q, K]^T + bias).
//                   A workgroup is 4 waves; it first stages the M rows of x in LDS as bf16 (16 B per
//                   lane) and, with the LayerNorm prologue, normalises them there: one wave per row,
//                   f32 two-pass statistics as in csrc/layernorm.hip, the result rounded to bf16
//                   exactly as the separate LayerNorm kernel rounds it, but never written to memory.
//                   Every workgroup recomputes the statistics (at most 16 x 4096 values).
//                   Then each wave owns `cpw` consecutive output columns and walks them CW at a
//                   time.  A column is a contiguous row of W: lane l reads its 16-B chunks l, l + 64,
//                   ... straight into VGPRs (2 * CW loads in flight per lane, no LDS round trip) and
//                   keeps one f32 accumulator per (column, row); the x chunk comes from LDS once per
//                   CW columns.  The 64 per-lane partials of every accumulator are summed by a folded
//                   butterfly: stages xor 32, 16, 8, 4, 2, 1 for every value, each stage halving the
//                   number of live values per lane while there is more than one, so CW * MB values
//                   cost about that many shuffles instead of six times as many.  The lane left
//                   holding (column, row) applies bias, GELU or the residual to the f32 sum and
//                   stores one bf16.
//                   RMSNorm prologue (rms): the same place and shape as the LayerNorm one, one pass
//                   for the f32 mean of squares, x * rstd * gamma rounded to bf16 as the separate
//                   RMSNorm kernel rounds it.
//                   SwiGLU epilogue (GLU): W is [2Q][K], gate rows then up rows, and output column c
//                   needs rows c and Q + c.  A walk of CW weight rows is ordered [gate c0 .., up c0 ..]
//                   (CW / 2 output columns), so after the fold the two sums of an output element sit
//                   in lanes that differ in bit 5 only: one shuffle pairs them and the gate lane
//                   stores silu(g + bias[c]) * (u + bias[Q + c]) from f32 with one rounding.
//
// Determinism and row invariance.  The K order of an accumulator is fixed by (lane, chunk) alone and
// the fold gives every value the sums a plain butterfly in the order 32 .. 1 gives it, whatever M,
// MB, CW or the grid are: row m of the result has the same bits computed alone or among 16 rows.
// No atomics, no workspace, every output element written exactly once; the grid depends on (Q)
// only and nothing is read on the host.
//
//   embed_rows_k    x[b, t] = tok[clamp(id)] + pos[clamp(positions[b] + t)], f32 sum, one rounding.
//                   A token id outside [0, vocab) is clamped: it never becomes an address.
//                   Without a position table (pos_w null) it is the clamped token row alone.
#include "common.h"
#include "tbamd.h"

namespace tbamd {
namespace {

constexpr int kRowsWaves = 4;

__device__ __forceinline__ void rows_unpack8(const uint4& r, float (&v)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 rows_pack8(const float (&v)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(v[2 * i]) | ((uint32_t)f2bf(v[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void rows_load8f(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// Sum each of the first N values of v over the 64 lanes.  While N > 1 a stage sends half of the
// values to the partner lane and keeps the other half (a + b is b + a bit for bit, so the kept
// value is what a plain butterfly would hold); afterwards lane l holds value fold_index<NV>(l) in
// v[0], replicated over the 64 / NV lanes that differ from l in the low bits only.
template <int NV, int N, int O>
__device__ __forceinline__ void fold_sum(float (&v)[NV], int lane) {
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
      fold_sum<NV, h, O / 2>(v, lane);
    } else {
      v[0] += __shfl_xor(v[0], O, 64);
      fold_sum<NV, 1, O / 2>(v, lane);
    }
  }
}
template <int NV>
__device__ __forceinline__ int fold_index(int lane) {
  int idx = 0;
#pragma unroll
  for (int n = NV, o = 32; n > 1; n >>= 1, o >>= 1) idx += (lane & o) ? n / 2 : 0;
  return idx;
}

// MB: rows the accumulators are laid out for (M <= MB); CW: weight rows a wave walks at a time;
// GLU: the SwiGLU epilogue (CW / 2 output columns per walk)
template <int MB, int CW, bool GLU>
__global__ __launch_bounds__(64 * kRowsWaves) void rows_linear_k(RowsLinearArgs a) {
  extern __shared__ uint4 xs[];  // [M][K / 8] chunks of 8 bf16
  constexpr int NV = MB * CW;
  constexpr int CO = GLU ? CW / 2 : CW;  // output columns per walk
  static_assert(NV <= 64, "one lane per (column, row) in the epilogue");
  static_assert(!GLU || CW >= 2, "a gate and an up row per output column");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nv = a.K >> 3;

  // ---- the M rows into LDS, raw
  for (int i = tid; i < a.M * nv; i += 64 * kRowsWaves) {
    const int m = i / nv, v = i - m * nv;
    uint4 r = make_uint4(0, 0, 0, 0);
    if (TB_BOUNDS_OK(m < a.M && v * 8 + 8 <= a.K, kBndGemmSrc))
      r = *reinterpret_cast<const uint4*>(a.x + (int64_t)m * a.sx + v * 8);
    xs[i] = r;
  }
  __syncthreads();
  // ---- LayerNorm / RMSNorm prologue: one wave per row, each lane rewrites only the chunks it read
  if (a.gamma && a.rms) {  // workgroup-uniform
    const float inv = 1.f / (float)a.K;
    for (int m = wid; m < a.M; m += kRowsWaves) {
      uint4* row = xs + m * nv;
      float s = 0.f;
      for (int v = lane; v < nv; v += 64) {
        float f[8];
        rows_unpack8(row[v], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) s += f[k] * f[k];
      }
      const float rs = rsqrtf(wave_sum(s) * inv + a.eps);
      for (int v = lane; v < nv; v += 64) {
        float f[8], g[8];
        rows_unpack8(row[v], f);
        rows_load8f(a.gamma + v * 8, g);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = f[k] * rs * g[k];
        row[v] = rows_pack8(f);
      }
    }
    __syncthreads();
  } else if (a.gamma) {
    const float inv = 1.f / (float)a.K;
    for (int m = wid; m < a.M; m += kRowsWaves) {
      uint4* row = xs + m * nv;
      float s = 0.f;
      for (int v = lane; v < nv; v += 64) {
        float f[8];
        rows_unpack8(row[v], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) s += f[k];
      }
      const float mu = wave_sum(s) * inv;
      s = 0.f;
      for (int v = lane; v < nv; v += 64) {
        float f[8];
        rows_unpack8(row[v], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = f[k] - mu;
          s += d * d;
        }
      }
      const float rs = rsqrtf(wave_sum(s) * inv + a.eps);
      for (int v = lane; v < nv; v += 64) {
        float f[8], g[8], b[8];
        rows_unpack8(row[v], f);
        rows_load8f(a.gamma + v * 8, g);
        rows_load8f(a.beta + v * 8, b);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = (f[k] - mu) * rs * g[k] + b[k];
        row[v] = rows_pack8(f);
      }
    }
    __syncthreads();
  }

  // ---- this wave's columns
  const int64_t col0 = ((int64_t)blockIdx.x * kRowsWaves + wid) * a.cpw;
  const int64_t cend = col0 + a.cpw < (int64_t)a.Q ? col0 + a.cpw : (int64_t)a.Q;
  const int nr = (nv + 63) >> 6;  // 16-B chunks per lane and column
  for (int64_t c0 = col0; c0 < cend; c0 += CO) {
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    for (int r0 = 0; r0 < nr; r0 += 2) {
      uint4 wq[2][CW];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int v = lane + 64 * (r0 + u);
#pragma unroll
        for (int c = 0; c < CW; ++c) {
          wq[u][c] = make_uint4(0, 0, 0, 0);
          // a column past the wave's range or a chunk past K never forms an address
          if constexpr (GLU) {  // walk slot c: gate row of output column c0 + c, or up row of c0 + c - CO
            const int64_t oc = c0 + (c < CO ? c : c - CO);
            const int64_t wr = c < CO ? oc : (int64_t)a.Q + oc;
            if (v < nv && oc < cend && TB_BOUNDS_OK(oc < a.Q && wr < 2 * (int64_t)a.Q && v * 8 + 8 <= a.K, kBndGemmSrc))
              wq[u][c] = *reinterpret_cast<const uint4*>(a.w + wr * a.K + v * 8);
          } else {
            if (v < nv && c0 + c < cend && TB_BOUNDS_OK(c0 + c < a.Q && v * 8 + 8 <= a.K, kBndGemmSrc))
              wq[u][c] = *reinterpret_cast<const uint4*>(a.w + (c0 + c) * a.K + v * 8);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int v = lane + 64 * (r0 + u);
        if (v < nv) {
          float wf[CW][8];
#pragma unroll
          for (int c = 0; c < CW; ++c) rows_unpack8(wq[u][c], wf[c]);
#pragma unroll
          for (int m = 0; m < MB; ++m) {
            if (m < a.M) {  // wave-uniform
              float xf[8];
              rows_unpack8(xs[m * nv + v], xf);
#pragma unroll
              for (int c = 0; c < CW; ++c) {
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[c * MB + m] = fmaf(xf[k], wf[c][k], acc[c * MB + m]);
              }
            }
          }
        }
      }
    }
    fold_sum<NV, NV, 32>(acc, lane);
    const int idx = fold_index<NV>(lane);
    const int c = idx / MB, m = idx - c * MB;
    const int64_t col = c0 + c;
    if constexpr (GLU) {
      // walk slots c and c + CO are values idx and idx + NV / 2: fold_index puts them in lanes l and l ^ 32
      const float up = __shfl_xor(acc[0], 32, 64);
      if ((lane & (64 / NV - 1)) == 0 && c < CO && m < a.M && col < cend) {
        float g = acc[0], u = up;
        if (a.bias) {
          g += bf2f(a.bias[col]);
          u += bf2f(a.bias[(int64_t)a.Q + col]);
        }
        const int64_t o = (int64_t)m * a.Q + col;
        if (TB_BOUNDS_OK(o < (int64_t)a.M * a.Q, kBndGemmDst)) a.y[o] = f2bf(silu_f(g) * u);
      }
    } else if ((lane & (64 / NV - 1)) == 0 && m < a.M && col < cend) {
      float z = acc[0];
      if (a.bias) z += bf2f(a.bias[col]);
      if (a.epi == kRowsGelu) z = gelu_f(z);
      else if (a.epi == kRowsResidual) z += bf2f(a.res[(int64_t)m * a.sres + col]);
      const int64_t o = (int64_t)m * a.Q + col;
      if (TB_BOUNDS_OK(o < (int64_t)a.M * a.Q, kBndGemmDst)) a.y[o] = f2bf(z);
    }
  }
}

// one lane per 16 B of the output: (row = b * T + t, chunk)
__global__ __launch_bounds__(256) void embed_rows_k(EmbedRowsArgs a) {
  const int nv = a.D >> 3;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)a.B * a.T * nv) return;
  const int v = (int)(id % nv);
  const int64_t row = id / nv;
  const int t = (int)(row % a.T);
  const int b = (int)(row / a.T);
  int64_t tk = a.tokens[b * a.stok[0] + t * a.stok[1]];
  tk = tk < 0 ? 0 : (tk >= a.vocab ? (int64_t)a.vocab - 1 : tk);  // never an address out of range
  int64_t p = (a.pos ? (int64_t)a.pos[b] : 0) + t;
  p = p < 0 ? 0 : (p >= a.max_len ? (int64_t)a.max_len - 1 : p);
  const uint4 tw = *reinterpret_cast<const uint4*>(a.tok_w + tk * a.D + v * 8);
  const bool ok = TB_BOUNDS_OK(row * a.D + v * 8 + 8 <= (int64_t)a.B * a.T * a.D, kBndGemmDst);
  if (!a.pos_w) {  // no learned positions (kernel-uniform): the clamped token row, bit for bit
    if (ok) *reinterpret_cast<uint4*>(a.y + row * a.D + v * 8) = tw;
    return;
  }
  float e[8], q[8];
  rows_unpack8(tw, e);
  rows_unpack8(*reinterpret_cast<const uint4*>(a.pos_w + p * a.D + v * 8), q);
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] += q[k];
  if (ok) *reinterpret_cast<uint4*>(a.y + row * a.D + v * 8) = rows_pack8(e);
}

template <int MB, int CW, bool GLU>
void rows_launch(const RowsLinearArgs& a, int grid, size_t lds, hipStream_t st) {
  // up to 16 x 4096 bf16 = 128 KiB of the CU's 160 KiB: above the default limit of a launch, raised
  // once per device at the first launch there (the warm-up step, ahead of any capture)
  static bool raised[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev >= 0 && dev < 64 && !raised[dev]) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rows_linear_k<MB, CW, GLU>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 16 * 4096 * 2);
    raised[dev] = true;
  }
  hipLaunchKernelGGL((rows_linear_k<MB, CW, GLU>), dim3(grid), dim3(64 * kRowsWaves), lds, st, a);
}

template <int CW, bool GLU = false>
void rows_dispatch(const RowsLinearArgs& a, int grid, size_t lds, hipStream_t st) {
  if (a.M <= 1) rows_launch<1, CW, GLU>(a, grid, lds, st);
  else if (a.M <= 2) rows_launch<2, CW, GLU>(a, grid, lds, st);
  else if (a.M <= 4) rows_launch<4, CW, GLU>(a, grid, lds, st);
  else if (a.M <= 8) rows_launch<8, CW, GLU>(a, grid, lds, st);
  else rows_launch<16, CW, GLU>(a, grid, lds, st);
}

}  // namespace

// Columns per wave, from Q alone (the grid must not depend on M: row invariance is tested across
// it, and a captured step replays any batch it was captured for).  The aim is about two workgroups
// per CU so that every CU streams: Q = 768 is one column per wave, 192 workgroups; the vocabulary
// head (50257) is 16 per wave, 786 workgroups of 64 columns, which also bounds how often the
// LayerNorm prologue is repeated.
int rows_linear_cols_per_wave(int Q) {
  const int want = (Q + kRowsWaves * 512 - 1) / (kRowsWaves * 512);
  return want <= 1 ? 1 : want <= 2 ? 2 : want <= 4 ? 4 : want <= 8 ? 8 : 16;
}

// SwiGLU: a wave streams two weight rows per output column, so it takes half the columns a plain
// product over the 2F weight rows would give it (at least one): F = 2048 at K = 768 is one column,
// two rows, per wave and 512 workgroups, the grid of a plain Q = 4096.  A function of F alone.
int rows_swiglu_cols_per_wave(int F) {
  const int c = rows_linear_cols_per_wave(2 * F) / 2;
  return c < 1 ? 1 : c;
}

void rows_linear(const RowsLinearArgs& a_, hipStream_t st) {
  RowsLinearArgs a = a_;
  const bool glu = a.epi == kRowsSwiglu;
  a.cpw = glu ? rows_swiglu_cols_per_wave(a.Q) : rows_linear_cols_per_wave(a.Q);
  const int per_wg = a.cpw * kRowsWaves;
  const int grid = (a.Q + per_wg - 1) / per_wg;
  const size_t lds = (size_t)a.M * a.K * 2;
  if (glu) {  // one or two output columns per walk
    if (a.cpw == 1) rows_dispatch<2, true>(a, grid, lds, st);
    else rows_dispatch<4, true>(a, grid, lds, st);
  } else if (a.cpw == 1) rows_dispatch<1>(a, grid, lds, st);
  else if (a.cpw == 2) rows_dispatch<2>(a, grid, lds, st);
  else rows_dispatch<4>(a, grid, lds, st);
}

void embed_rows(const EmbedRowsArgs& a, hipStream_t st) {
  const int64_t total = (int64_t)a.B * a.T * (a.D / 8);
  if (total == 0) return;
  hipLaunchKernelGGL(embed_rows_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace tbamd
