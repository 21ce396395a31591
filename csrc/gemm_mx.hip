// Dense GEMM on an MXFP4 weight, gfx950 MFMA (v_mfma_f32_16x16x32_bf16), 512-thread workgroups:
//
//   Y[p][q] = epi( sum_k X[p][k] * deq(W)[q][k] )      p < P (rows), q < Q (out features)
//   deq(W)[q][k] = e2m1(code) * f32_from_bits(scale << 23)
//
// Not in the reference.  X bf16 [P][K] (row stride ldx), codes uint8 [Q][K / 2] (element 2i in the
// low nibble of byte i), scales uint8 [Q][K / 32] (e8m0, one per block of 32 inputs), Y bf16 [P][Q].
// Weight-only quantisation: the activations stay bf16, the accumulator is f32, and the bf16 weight
// exists in LDS only.  It is the many-row partner of csrc/rows_gemm_mx.hip (1 .. 16 rows).
//
// Orientation (csrc/gemm.hip): the MFMA computes D[q][p], weight rows as the A operand and X rows
// as the B operand, so a lane's 4 accumulator rows are 4 consecutive output features of one row p.
//
// Tiling: BP x BQ outputs per workgroup, a k-tile of 128 (4 MX blocks per weight row), 8 waves in a
// WP x WQ grid, two LDS stages.  A stage holds the k-tile as two 64-deep halves, each half in
// gemm.hip's row-read layout: 128-B rows, the 16-B chunk XORed by (row >> 1) & 7, read with
// ds_read_b128.
//   X   global -> LDS directly (global_load_lds, 16 B per lane, 1 KiB per wave instruction), the
//       swizzle applied to the global source address; rows past P and chunks past K read the
//       zero page.
//   W   global -> registers -> LDS.  Thread i of the first 4 BQ threads owns MX block i & 3 of
//       weight row i >> 2: one 16-B load of 32 codes and one scale byte.  16
//       v_cvt_scalef32_pk_bf16_fp4 turn them into 32 bf16 (exact: the scale is a power of two),
//       written with four ds_write_b128 into the swizzled layout.  Rows past Q and blocks past K
//       are not loaded and are written as zeros.
// Schedule per k-tile t: issue the X loads and the code / scale loads of t + 1, run the MFMAs of t,
// then decode t + 1 into the other stage; one vmcnt(0) + barrier.  With the 128-row tile a code is
// decoded once per 128 rows of X (16 conversions against 32 MFMAs per wave and k-tile).
//
// Two instantiations, chosen on the host from P alone: 128 x 128 (waves 4P x 2Q) above kMxShortRows
// rows, and 64 x 32 (4P x 2Q, one MFMA tile per wave) up to it, where the product is bound by the
// weight stream and the narrow Q tile spreads it over more CUs.  Workgroups are remapped so one
// XCD runs contiguous tile ids (q fastest).  The grid is a function of (P, Q); no atomics, no
// split-K, no workspace, nothing read on the host: capturable and bit-deterministic, and row p has
// the same bits for every P served by the same instantiation.
//
// Scale bytes 0 and 255 (never produced by ops.linear.mx_quantize) read as a zero scale and +inf,
// the rule of mx_decode8: the block converts at scale 1 and is multiplied on a side path.
//
// Tails: any P, Q >= 1 (a lane stores 8 B when Q and the residual stride are multiples of 4, else
// element by element), K % 32 == 0, K >= 32, K not necessarily a multiple of 128.
#include "common.h"
#include "tbamd.h"

namespace tbamd {
namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

constexpr int kThreads = 512;
constexpr int kBK = 128;           // k-tile: 4 MX blocks
constexpr int kMxShortRows = 128;  // up to this many rows: the 64 x 32 tile

__device__ __attribute__((aligned(64))) uint4 g_gemm_mx_zero[64];  // 1 KiB of zeros

__device__ __forceinline__ void glds16(const void* src, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ int swz_r(int row) { return (row >> 1) & 7; }

// eight codes (one dword) of a block with scale byte sb -> 8 bf16 (one 16-B chunk)
__device__ __forceinline__ void decode8(uint32_t w, float cs, uint32_t (&o)[4]) {
  o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, cs, 0));
  o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, cs, 1));
  o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, cs, 2));
  o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, cs, 3));
}

template <int BP, int BQ, int WP>
__global__ __launch_bounds__(kThreads, 2) void gemm_mx_k(GemmMxArgs a) {
  constexpr int WQ = 8 / WP;
  constexpr int PW = BP / WP, QW = BQ / WQ;  // per-wave tile
  constexpr int TP = PW / 16, TQ = QW / 16;
  static_assert(TP >= 1 && TQ >= 1 && BP % 32 == 0 && BQ % 16 == 0, "tile");
  constexpr int WH_U4 = BQ * 8, XH_U4 = BP * 8;  // uint4 per 64-deep half
  constexpr int STAGE = 2 * (WH_U4 + XH_U4);     // [W half 0 | W half 1 | X half 0 | X half 1]
  constexpr int NXI = BP / 32;                   // X glds instructions per wave per stage
  constexpr int NWB = (BQ * 4 + kThreads - 1) / kThreads;  // MX blocks per thread per k-tile
  __shared__ __attribute__((aligned(16))) uint4 lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave / WQ, wq = wave % WQ;
  const int ntp = (a.P + BP - 1) / BP, ntq = (a.Q + BQ - 1) / BQ;
  const int nwg = ntp * ntq;
  int bid = blockIdx.x;
  {
    const int q8 = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
    bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  }
  const int tq = bid % ntq, tp = bid / ntq;
  const int p0 = tp * BP, q0 = tq * BQ;
  const int nb = a.K >> 5;  // MX blocks per weight row
  const int KT = (a.K + kBK - 1) / kBK;

  // ---- X staging sources: instruction n = wave + 8 j covers rows 8 g .. 8 g + 7 of half h
  const uint16_t* xsrc[NXI];
  int xk[NXI];  // k of this lane's chunk within the k-tile
#pragma unroll
  for (int j = 0; j < NXI; ++j) {
    const int n = wave + 8 * j, h = n / (BP / 8), g = n % (BP / 8);
    const int row = 8 * g + (lane >> 3), p = p0 + row;
    const int ch = (lane & 7) ^ swz_r(row);
    xk[j] = 64 * h + 8 * ch;
    xsrc[j] = p < a.P ? a.X + (int64_t)p * a.ldx + xk[j] : nullptr;
  }
  const void* zpage = pin_sgpr(g_gemm_mx_zero);
  auto issue_x = [&](int kt, int buf) {
    uint4* base = lds + buf * STAGE + 2 * WH_U4;
    const int64_t k0 = (int64_t)kt * kBK;
#pragma unroll
    for (int j = 0; j < NXI; ++j) {
      bool ok = xsrc[j] != nullptr && k0 + xk[j] < a.K;
      ok = ok && TB_BOUNDS_OK(xsrc[j] + k0 + 8 <= a.X + (int64_t)(a.P - 1) * a.ldx + a.K, kBndGemmSrc);
      const void* s = ok ? (const void*)(xsrc[j] + k0) : zpage;
      glds16(s, base + (wave + 8 * j) * 64);
    }
  };

  // ---- W blocks of this thread: block i = tid + 512 j is (row i >> 2, block i & 3 of the k-tile)
  const uint8_t* csrc[NWB];
  const uint8_t* ssrc[NWB];
#pragma unroll
  for (int j = 0; j < NWB; ++j) {
    const int i = tid + kThreads * j, row = i >> 2, kb = i & 3;
    const int64_t q = (int64_t)q0 + row;
    const bool in = i < BQ * 4 && q < a.Q;
    csrc[j] = in ? a.codes + q * (a.K >> 1) + kb * 16 : nullptr;
    ssrc[j] = in ? a.scales + q * nb + kb : nullptr;
  }
  uint4 cd[NWB];
  uint32_t sb[NWB];
  auto load_w = [&](int kt) {
#pragma unroll
    for (int j = 0; j < NWB; ++j) {
      const int b = kt * 4 + ((tid + kThreads * j) & 3);
      cd[j] = make_uint4(0, 0, 0, 0);
      sb[j] = 127u;
      // a row past Q or a block past K never forms an address; its codes are +0
      if (csrc[j] != nullptr && b < nb &&
          TB_BOUNDS_OK(csrc[j] + (int64_t)kt * 64 + 16 <= a.codes + (int64_t)a.Q * (a.K >> 1), kBndGemmSrc)) {
        cd[j] = *reinterpret_cast<const uint4*>(csrc[j] + (int64_t)kt * 64);
        sb[j] = ssrc[j][(int64_t)kt * 4];
      }
    }
  };
  auto store_w = [&](int buf) {
    uint4* Wt = lds + buf * STAGE;
#pragma unroll
    for (int j = 0; j < NWB; ++j) {
      const int i = tid + kThreads * j, row = i >> 2, kb = i & 3;
      if (i < BQ * 4) {  // wave-uniform
        const uint32_t cw[4] = {cd[j].x, cd[j].y, cd[j].z, cd[j].w};
        const bool plain = sb[j] - 1u < 254u;
        const float scale = __uint_as_float(sb[j] << 23);
        const float cs = plain ? scale : 1.f;
        uint4* dst = Wt + (kb >> 1) * WH_U4 + row * 8;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          uint32_t o[4];
          decode8(cw[c], cs, o);
          if (!plain) {  // scale byte 0 or 255: the rule's zero / +inf scale, in f32, rounded once
#pragma unroll
            for (int e = 0; e < 4; ++e)
              o[e] = (uint32_t)f2bf(__uint_as_float(o[e] << 16) * scale) |
                     ((uint32_t)f2bf(__uint_as_float(o[e] & 0xffff0000u) * scale) << 16);
          }
          dst[((kb & 1) * 4 + c) ^ swz_r(row)] = make_uint4(o[0], o[1], o[2], o[3]);
        }
      }
    }
  };

  f32x4_t acc[TQ][TP];
#pragma unroll
  for (int i = 0; i < TQ; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fg = lane >> 4;
  auto compute = [&](int buf) {
    const uint4* Wt = lds + buf * STAGE;
    const uint4* Xt = Wt + 2 * WH_U4;
#pragma unroll
    for (int ks = 0; ks < kBK / 32; ++ks) {
      const int h = ks >> 1, ch = (ks & 1) * 4 + fg;
      bf16x8_t af[TQ], bf[TP];
#pragma unroll
      for (int i = 0; i < TQ; ++i) {
        const int row = wq * QW + 16 * i + fr;
        af[i] = __builtin_bit_cast(bf16x8_t, Wt[h * WH_U4 + row * 8 + (ch ^ swz_r(row))]);
      }
#pragma unroll
      for (int j = 0; j < TP; ++j) {
        const int row = wp * PW + 16 * j + fr;
        bf[j] = __builtin_bit_cast(bf16x8_t, Xt[h * XH_U4 + row * 8 + (ch ^ swz_r(row))]);
      }
#pragma unroll
      for (int i = 0; i < TQ; ++i)
#pragma unroll
        for (int j = 0; j < TP; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  // ---- main loop: the loads of k-tile t + 1 fly under the MFMAs of t, its decode follows them
  issue_x(0, 0);
  load_w(0);
  store_w(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < KT;
    if (more) {
      issue_x(kt + 1, cur ^ 1);
      load_w(kt + 1);
    }
    asm volatile("" ::: "memory");  // the loads are issued before the MFMAs
    compute(cur);
    asm volatile("" ::: "memory");
    if (more) store_w(cur ^ 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: lane holds q = q0 + wq*QW + 16 i + 4 fg + (0..3), p = p0 + wp*PW + 16 j + fr
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    const int q = q0 + wq * QW + 16 * i + 4 * fg;
    if (q >= a.Q) continue;
    const int nq = a.Q - q < 4 ? a.Q - q : 4;  // 4 whenever a.vec
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < nq) bv[e] = bf2f(a.bias[q + e]);
    }
#pragma unroll
    for (int j = 0; j < TP; ++j) {
      const int p = p0 + wp * PW + 16 * j + fr;
      if (p >= a.P) continue;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + bv[e];
      if (a.epi == kRowsGelu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_f(v[e]);
      } else if (a.epi == kRowsResidual) {
        const uint16_t* r = a.res + (int64_t)p * a.ldres + q;
        if (a.vec) {
          const uint2 r2 = *reinterpret_cast<const uint2*>(r);
          v[0] += bf2f((uint16_t)(r2.x & 0xffff));
          v[1] += bf2f((uint16_t)(r2.x >> 16));
          v[2] += bf2f((uint16_t)(r2.y & 0xffff));
          v[3] += bf2f((uint16_t)(r2.y >> 16));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < nq) v[e] += bf2f(r[e]);
        }
      }
      const int64_t o = (int64_t)p * a.Q + q;
      if (!TB_BOUNDS_OK(o + nq <= (int64_t)a.P * a.Q, kBndGemmDst)) continue;
      if (a.vec) {
        *reinterpret_cast<uint2*>(a.Y + o) = make_uint2((uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16),
                                                        (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < nq) a.Y[o + e] = f2bf(v[e]);
      }
    }
  }
}

template <int BP, int BQ, int WP>
void launch(const GemmMxArgs& a, hipStream_t st) {
  const int64_t nwg = (int64_t)((a.P + BP - 1) / BP) * ((a.Q + BQ - 1) / BQ);
  gemm_mx_k<BP, BQ, WP><<<dim3((unsigned)nwg), kThreads, 0, st>>>(a);
}

}  // namespace

// rows per workgroup of the instantiation that serves P rows (a function of P alone)
int gemm_mx_tile_rows(int P) { return P <= kMxShortRows ? 64 : 128; }

void gemm_mx(const GemmMxArgs& a_, hipStream_t st) {
  GemmMxArgs a = a_;
  if (a.P <= 0 || a.Q <= 0) return;
  // 8-B stores (and residual loads) when every lane's quad is whole and 8-B aligned
  a.vec = a.Q % 4 == 0 && reinterpret_cast<uintptr_t>(a.Y) % 8 == 0 &&
          (a.res == nullptr || (a.ldres % 4 == 0 && reinterpret_cast<uintptr_t>(a.res) % 8 == 0));
  if (gemm_mx_tile_rows(a.P) == 64) launch<64, 32, 4>(a, st);
  else launch<128, 128, 4>(a, st);
}

}  // namespace tbamd
