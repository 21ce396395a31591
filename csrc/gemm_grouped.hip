// Grouped bf16 GEMM on gfx950 MFMA (v_mfma_f32_16x16x32_bf16) for mixture-of-experts MLPs: one
// launch multiplies expert-sorted rows by their experts' weights, the group boundaries read from
// device memory.  Three orientations, the ones a Linear needs:
//
//   grouped_nt   Y[r][q]     = sum_k X[r][k]  W[e(r)][q][k]          W [E][Q][K]   (forward)
//   grouped_nn   dX[r][q]    = sum_k dY[r][k] W[e(r)][k][q]          W [E][K][Q]   (input gradient: the
//                                                                    same weight read transposed from LDS)
//   grouped_tn   dW[e][p][q] = sum_{r in group e} dY[r][p] X[r][q]   dW [E][P][Q]  (weight gradient: both
//                                                                    operands read transposed from LDS)
//
// Groups.  offsets is int32 [E + 1] in device memory.  Boundary b_0 = 0 and
// b_i = max(b_{i-1}, clamp(offsets[i], 0, R)) for i = 1 .. E: expert e owns rows [b_e, b_{e+1}).  The
// running maximum makes a decreasing pair an empty group and keeps the groups disjoint, so whatever
// offsets holds, every row index a kernel forms lies in [0, R) and every output element has exactly one
// writer.  offsets[0] is not read.  Rows [b_E, R) belong to no expert: the row kernels write them as
// zeros, the weight gradient does not read them.
//
// Grids are functions of shapes alone (hipGraph capture; a replay follows in-place changes of offsets):
//   rows    (ceil(R / 128) + E) row tiles x ceil(Q / BQ) column tiles.  The E + 1 groups (the experts and
//           the zero tail) split into at most that many 128-row tiles: ceil(a) + ceil(b) <= ceil(a + b) + 1.
//           A workgroup walks the boundaries once (wave-uniform, scalar loads) to find its (group, tile);
//           a tile never spans two groups, rows past the group's end read the zero page and are not
//           stored, and a workgroup whose tile index is past the last used tile exits.
//   tn      ceil(P / 128) x ceil(Q / BQ) tiles x E.  The reduction runs over the expert's own rows in
//           64-row k-tiles that start at b_e: in this orientation a k index is an LDS row, so a range may
//           start and end at any row.  No split-K: no atomics, no workspace, every element written once
//           (exact zeros for an expert without rows), bit-deterministic.
//
// Tile: 128 x 128 (waves 4 x 2, 32 x 64 each) or 128 x 64 for Q <= 64 (waves 8 x 1, 16 x 64), BK = 64,
// 512 threads.  Staging is the dense engine's (csrc/gemm.hip): direct-to-LDS loads of 16 B per lane,
// two LDS stages (the loads of k-tile t + 1 are issued before the MFMAs of tile t), 128-B LDS rows with
// the XOR swizzles applied to the global source address, a zero page for everything out of range.
// The MFMA computes D[q][p], so a lane's 4 accumulator rows are 4 consecutive columns of one output row.
//
// Needs K % 8 == 0 and Q % 8 == 0 (P % 8 == 0 for tn), contiguous rows, 16-B aligned bases.
#include "common.h"
#include "tbamd.h"

namespace tbamd {
namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short i16x4_t __attribute__((ext_vector_type(4)));
typedef short i16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;
typedef __attribute__((address_space(3))) i16x4_t lds_i16x4_t;

constexpr int kThreads = 512;
constexpr int kBK = 64;
constexpr int kBP = 128;

__device__ __attribute__((aligned(64))) uint4 g_grouped_zero[64];  // 1 KiB of zeros

__device__ __forceinline__ void glds16(const void* src, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ int swz_r(int row) { return (row >> 1) & 7; }  // row-read tiles
__device__ __forceinline__ int swz_t(int row) { return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1; }  // transposed

enum : int { kNT = 0, kNN = 1, kTN = 2 };

struct GroupedArgs {
  const uint16_t* X;  // nt / nn: rows [R][K];   tn: dY [R][P]
  const uint16_t* W;  // nt: [E][Q][K]  nn: [E][K][Q];  tn: X [R][Q]
  uint16_t* Y;        // nt / nn: [R][Q];        tn: dW [E][P][Q]
  const int* off;     // [E + 1]
  int R, E;
  int P, Q, K;        // P: tn only (output rows); K: nt / nn only (reduction length)
};

// boundary i (1 <= i <= E) given the one before it
__device__ __forceinline__ int next_bound(const int* off, int i, int prev, int R) {
  return max(prev, min(max(off[i], 0), R));
}

template <int BQ, int WP, int MODE>
__global__ __launch_bounds__(kThreads, 2) void grouped_k(GroupedArgs a) {
  constexpr bool TX = MODE == kTN, TW = MODE != kNT;
  constexpr int BP = kBP, WQ = 8 / WP;
  constexpr int PW = BP / WP, QW = BQ / WQ;  // per-wave tile
  constexpr int TP = PW / 16, TQ = QW / 16;
  static_assert(TP >= 1 && TQ >= 1 && BQ % 64 == 0, "tile");
  constexpr int W_U4 = BQ * kBK / 8, X_U4 = BP * kBK / 8;
  constexpr int STAGE = W_U4 + X_U4;  // uint4 per stage
  constexpr int NI = (BP + BQ) / 64;  // glds instructions per wave per stage
  __shared__ __attribute__((aligned(16))) uint4 lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave / WQ, wq = wave % WQ;
  const int ntq = (a.Q + BQ - 1) / BQ;
  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {  // one XCD runs contiguous tile ids (q fastest: the column tiles of one row panel share its L2)
    const int q8 = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
    bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  }
  const int tq = bid % ntq;
  int tp = bid / ntq;
  const int q0 = tq * BQ;

  // ---- this workgroup's group: rows [lo, hi) of the row operands, expert e
  int e, lo, hi, p0, pend, kred;
  if constexpr (MODE == kTN) {
    e = blockIdx.y;
    lo = 0;
    for (int i = 1; i <= e; ++i) lo = next_bound(a.off, i, lo, a.R);
    hi = next_bound(a.off, e + 1, lo, a.R);
    p0 = tp * BP, pend = a.P;
    kred = hi - lo;  // the reduction: the expert's rows
  } else {
    e = -1;
    int prev = 0;
    for (int i = 0; i <= a.E; ++i) {  // group E = the zero tail [b_E, R)
      const int b = i < a.E ? next_bound(a.off, i + 1, prev, a.R) : a.R;
      const int nt = (b - prev + BP - 1) / BP;
      if (tp < nt) {
        e = i, lo = prev + tp * BP, hi = b;
        break;
      }
      tp -= nt;
      prev = b;
    }
    if (e < 0) return;  // past the last used tile
    p0 = lo, pend = hi;
    kred = e < a.E ? a.K : 0;  // the tail multiplies nothing: zeros
  }
  const int KT = (kred + kBK - 1) / kBK;

  // operand bases: the W-side operand feeds the MFMA's A (q) rows, the X-side its B (p) rows
  const uint16_t* Wb;
  const uint16_t* Xb;
  if constexpr (MODE == kTN) {
    Wb = a.W + (int64_t)lo * a.Q;  // X rows of the expert: [kred][Q]
    Xb = a.X + (int64_t)lo * a.P;  // dY rows of the expert: [kred][P]
  } else {
    Wb = a.W + (int64_t)(e < a.E ? e : 0) * a.Q * a.K;
    Xb = a.X;
  }

  // ---- per-lane staging sources (NI wave-instructions of 8 rows x 128 B)
  // instruction j of wave w covers combined rows 8 * (w + 8 j) .. + 7 ([W rows | X rows])
  const uint16_t* src[NI];
  int kofs[NI];      // the k this lane's chunk starts at (row-read) or its row stands for (transposed)
  int64_t kstr[NI];  // per-k-tile advance (elements)
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int crow = 8 * (wave + 8 * j) + (lane >> 3);
    const int pos = lane & 7;
    if (crow < BQ) {
      if constexpr (!TW) {
        const int row = crow, q = q0 + row;
        const int ch = pos ^ swz_r(row);
        src[j] = q < a.Q ? Wb + (int64_t)q * a.K + ch * 8 : nullptr;
        kofs[j] = ch * 8;
        kstr[j] = kBK;
      } else {
        // subtile st covers columns q0 + 64 st .. + 63; row = k within the tile
        const int st = crow >> 6, row = crow & 63;
        const int ch = pos ^ swz_t(row);
        const int q = q0 + 64 * st + ch * 8;
        src[j] = q < a.Q ? Wb + (int64_t)row * a.Q + q : nullptr;
        kofs[j] = row;
        kstr[j] = (int64_t)kBK * a.Q;
      }
    } else if constexpr (!TX) {
      const int row = crow - BQ, p = p0 + row;
      const int ch = pos ^ swz_r(row);
      src[j] = p < pend ? Xb + (int64_t)p * a.K + ch * 8 : nullptr;
      kofs[j] = ch * 8;
      kstr[j] = kBK;
    } else {
      const int xrow = crow - BQ, st = xrow >> 6, row = xrow & 63;
      const int ch = pos ^ swz_t(row);
      const int p = p0 + 64 * st + ch * 8;
      src[j] = p < pend ? Xb + (int64_t)row * a.P + p : nullptr;
      kofs[j] = row;
      kstr[j] = (int64_t)kBK * a.P;
    }
  }

  const void* zpage = pin_sgpr(g_grouped_zero);
  auto issue = [&](int kt, int buf) {
    uint4* base = lds + buf * STAGE;
    const int k0 = kt * kBK;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      bool ok = src[j] != nullptr && (k0 + kofs[j] < kred);
      // extent of the operand this instruction reads
      ok = ok && TB_BOUNDS_OK(
                     src[j] + (int64_t)kt * kstr[j] + 8 <=
                         (j * 8 * 8 + wave * 8 < BQ
                              ? a.W + (MODE == kTN ? (int64_t)a.R * a.Q : (int64_t)a.E * a.Q * a.K)
                              : a.X + (int64_t)a.R * (MODE == kTN ? a.P : a.K)),
                     kBndGemmSrc);
      const void* s = ok ? (const void*)(src[j] + (int64_t)kt * kstr[j]) : zpage;
      glds16(s, base + (wave + 8 * j) * 64);
    }
  };

  f32x4_t acc[TQ][TP];
#pragma unroll
  for (int i = 0; i < TQ; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fg = lane >> 4;
  // transposed operand fragment: tile = [64 k][64 cols] subtiles (128-B rows, swz_t);
  // lane -> column (16-aligned block + fr), k = 32 ks + 8 fg + (0..7)
  auto tr_read = [&](const uint4* tile, int cblk, int ks) -> bf16x8_t {
    const int st = cblk >> 6, c = (cblk & 63) + 4 * (fr & 3);  // lane 4qq+pp supplies (row qq, col 4pp)
    const int r0 = 32 * ks + 8 * fg + (fr >> 2);
    const char* tb = reinterpret_cast<const char*>(tile + st * 512);
    const int ch = c >> 3, b8 = (c & 4) ? 8 : 0;
    const char* a0 = tb + r0 * 128 + ((ch ^ swz_t(r0)) << 4) + b8;
    const char* a1 = tb + (r0 + 4) * 128 + ((ch ^ swz_t(r0 + 4)) << 4) + b8;
    const i16x4_t l = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t*)a0);
    const i16x4_t h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_t*)a1);
    const i16x8_t v = {l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
    return __builtin_bit_cast(bf16x8_t, v);
  };
  auto compute = [&](int buf) {
    const uint4* Wt = lds + buf * STAGE;
    const uint4* Xt = Wt + W_U4;
#pragma unroll
    for (int ks = 0; ks < kBK / 32; ++ks) {
      bf16x8_t af[TQ], bf[TP];
#pragma unroll
      for (int i = 0; i < TQ; ++i) {
        const int qr = wq * QW + 16 * i;  // first column of this 16-block (tile-local)
        if constexpr (!TW) {
          const int row = qr + fr, ch = ks * 4 + fg;
          af[i] = __builtin_bit_cast(bf16x8_t, Wt[row * 8 + (ch ^ swz_r(row))]);
        } else {
          af[i] = tr_read(Wt, qr, ks);
        }
      }
#pragma unroll
      for (int j = 0; j < TP; ++j) {
        if constexpr (!TX) {
          const int row = wp * PW + 16 * j + fr, ch = ks * 4 + fg;
          bf[j] = __builtin_bit_cast(bf16x8_t, Xt[row * 8 + (ch ^ swz_r(row))]);
        } else {
          bf[j] = tr_read(Xt, wp * PW + 16 * j, ks);
        }
      }
#pragma unroll
      for (int i = 0; i < TQ; ++i)
#pragma unroll
        for (int j = 0; j < TP; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  // ---- main loop: prefetch t + 1 while multiplying t; one drain + barrier per k-tile
  if (KT > 0) issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) issue(kt + 1, cur ^ 1);
    compute(cur);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: lane holds q = q0 + wq*QW + 16 i + 4 fg + (0..3), p = p0 + wp*PW + 16 j + fr
  uint16_t* Yb = a.Y;
  int64_t yrows = a.R;
  if constexpr (MODE == kTN) {
    Yb += (int64_t)e * a.P * a.Q;
    yrows = a.P;
  }
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    const int q = q0 + wq * QW + 16 * i + 4 * fg;
    if (q >= a.Q) continue;  // Q % 8 == 0 is required by the host
#pragma unroll
    for (int j = 0; j < TP; ++j) {
      const int p = p0 + wp * PW + 16 * j + fr;
      if (p >= pend) continue;
      const int64_t o = (int64_t)p * a.Q + q;
      if (TB_BOUNDS_OK(p >= 0 && o + 4 <= yrows * a.Q, kBndGemmDst))
        *reinterpret_cast<uint2*>(Yb + o) =
            make_uint2((uint32_t)f2bf(acc[i][j][0]) | ((uint32_t)f2bf(acc[i][j][1]) << 16),
                       (uint32_t)f2bf(acc[i][j][2]) | ((uint32_t)f2bf(acc[i][j][3]) << 16));
    }
  }
}

template <int MODE>
void launch(const GroupedArgs& a, int ntp, int gy, hipStream_t st) {
  if (a.Q > 64) {
    const dim3 grid(ntp * ((a.Q + 127) / 128), gy);
    grouped_k<128, 4, MODE><<<grid, kThreads, 0, st>>>(a);
  } else {
    const dim3 grid(ntp, gy);
    grouped_k<64, 8, MODE><<<grid, kThreads, 0, st>>>(a);
  }
}

}  // namespace

// Y [R][Q] = rows of X [R][K] times their experts' W: [E][Q][K] (tw = false) or [E][K][Q] (tw = true)
void grouped_rows_bf16(const void* X, const void* W, bool tw, const int* offsets, void* Y, int R, int E, int Q, int K,
                       hipStream_t st) {
  if (R <= 0 || Q <= 0 || E <= 0) return;
  GroupedArgs a{(const uint16_t*)X, (const uint16_t*)W, (uint16_t*)Y, offsets, R, E, 0, Q, K};
  const int ntp = (R + kBP - 1) / kBP + E;
  if (tw) launch<kNN>(a, ntp, 1, st);
  else launch<kNT>(a, ntp, 1, st);
}

// dW [E][P][Q] = per expert, dY[rows]^T X[rows] with dY [R][P], X [R][Q]
void grouped_tn_bf16(const void* dY, const void* X, const int* offsets, void* dW, int R, int E, int P, int Q,
                     hipStream_t st) {
  if (P <= 0 || Q <= 0 || E <= 0) return;
  GroupedArgs a{(const uint16_t*)dY, (const uint16_t*)X, (uint16_t*)dW, offsets, R, E, P, Q, 0};
  launch<kTN>(a, (P + kBP - 1) / kBP, E, st);
}

}  // namespace tbamd
