// Rolling KV cache: the slot arithmetic shared by csrc/attention_decode.hip and csrc/attention_extend.hip.
//
// A rolling cache layer is [B, Hkv, R, 64] used as a ring: logical row j (the j-th token of the
// sequence) lives in slot j mod R, and positions / lengths keep counting tokens, not slots.  With an
// upper limit n >= 1 (len of a decode, L(b, T - 1) of an extend) slot p holds logical row j(p), the
// largest j = p (mod R) with j < n.  The kernels never form j(p); they use its distance back from the
// newest row,
//
//     d(p) = n - 1 - j(p) = (pm - p) mod R  in [0, R),      pm = (n - 1) mod R  (the newest row's slot),
//
// which needs one division per wave (ring_newest: n - 1 < 2^32, unsigned 32-bit) and a compare and an
// add per slot (ring_back).  j(p) < 0, a slot that was never written, is d(p) >= n.  A query with limit
// L <= n and window W sees max(0, L - W) <= j(p) < L, that is
//
//     n - L <= d(p) < min(n, n - L + W),
//
// small non-negative numbers: a decode has L = n, an extend n - L <= T - 1, and the host guarantees
// T - 1 + W <= R, so the bounds never pass R and no two logical rows of one query's window share a slot.
//
// In slot space the slots with dlo <= d(p) < dhi are the cyclic interval that ends at slot pm - dlo and
// holds dhi - dlo slots: up to two intervals of [0, R).  ring_any tells whether a range of slots [s, e)
// meets it, the chunk-level / split-level "empty" decision.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

namespace tbamd {

// the slot of logical row n - 1; n in [1, 2^32)
__device__ __forceinline__ int ring_newest(int64_t n, int R) { return (int)((uint32_t)(n - 1) % (uint32_t)R); }

// d(p) for a slot 0 <= p < R
__device__ __forceinline__ int ring_back(int pm, int p, int R) {
  const int d = pm - p;
  return d < 0 ? d + R : d;
}

// does [s, e), 0 <= s < e <= R, hold a slot with dlo <= d(p) < dhi?  (0 <= dlo < dhi <= R)
__device__ __forceinline__ bool ring_any(int pm, int dlo, int dhi, int s, int e, int R) {
  int a = pm - dhi + 1;  // the interval's first slot, in (-R, R)
  if (a < 0) a += R;
  const int b = a + (dhi - dlo);  // one past its last, unwrapped: <= 2R - 1
  return (s < (b < R ? b : R) && e > a) || (b > R && s < b - R);
}

}  // namespace tbamd
