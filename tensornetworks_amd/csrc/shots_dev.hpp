// The pick rule of the finite-shot sampler (kernels_shots.hip), host- and device-callable so that
// a host driver can execute the kernel's own text (tests/test_shots_host.py).
//
// Rule R.  cdf[0..blk) are the block's inclusive prefix sums as the draw kernel forms them, pos its positivity mask
// (bit i & 31 of word i >> 5 is set iff entry i is > 0; (blk >> 5) + 1 words, every bit at or above blk zero, so that
// index blk itself can be looked up), last the block's last positive entry (-1 if there is none) and
// x = u * cdf[blk - 1].  With lo0 the first index whose cdf exceeds x, the outcome is the first index i >= lo0 whose
// VALUE is positive; if there is none, it is `last`; a block without a positive entry counts nothing (-1).
//
// Why the mask: the kernel's cdf is not one running sum.  Thread t's last entry is fl(pre_t + run_t) and the next entry
// starts from pre_(t+1), the same real number rounded along another path of the scan, so a zero entry at a thread
// boundary can get cdf[i] > cdf[i-1] and own an interval of x (about 2^-53 of the total wide).  On a cdf in which zero
// entries never rise (every dyadic row, any sequential sum) lo0 is already positive and R is "first i with cdf[i] > x".
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace bornvi {

constexpr int SHOTS_BLOCK_BITS = 12, SHOTS_BLOCK = 1 << SHOTS_BLOCK_BITS;   // entries per block of the hierarchy
constexpr int SHOTS_MASK_WORDS = SHOTS_BLOCK / 32 + 1;                      // 4096 bits = 512 B, and the zero word of bit 4096

// N draws of one block at once (the kernel takes the two of a Philox call): the N bisections advance in lock step, so
// their LDS reads are in flight together; each makes the probes of "lo = 0, hi = blk; while (lo < hi) { mid = (lo + hi)
// >> 1; if (cdf[mid] > x) hi = mid; else lo = mid + 1; }" and no others, so on a cdf that is not monotone to the last bit
// the result is that loop's too.  An interval of z entries shrinks to at most z / 2: floor(log2 blk) + 1 steps suffice.
template <int N>
__host__ __device__ __forceinline__ void shots_pick(const double* cdf, const uint32_t* pos, int blk, int last,
                                                    const double (&x)[N], int (&out)[N]) {
  int lo[N], hi[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    lo[k] = 0;
    hi[k] = blk;
  }
  for (int s = 32 - __builtin_clz((unsigned)blk); s > 0; --s) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool open = lo[k] < hi[k];        // a finished search reads cdf[0] and keeps its bounds
      const int mid = (lo[k] + hi[k]) >> 1;   // open: lo <= mid < hi <= blk
      const bool gt = cdf[open ? mid : 0] > x[k];
      hi[k] = open && gt ? mid : hi[k];
      lo[k] = open && !gt ? mid + 1 : lo[k];
    }
  }
  const int nw = (blk + 31) >> 5;
  uint32_t bits[N];                           // lo[k] = lo0: the mask from entry lo0 to the end of its word, read for all N first
#pragma unroll
  for (int k = 0; k < N; ++k) bits[k] = pos[lo[k] >> 5] & (~0u << (lo[k] & 31));      // lo0 == blk reads zero bits: see pos
#pragma unroll
  for (int k = 0; k < N; ++k) {               // the first positive entry at or after lo0: almost always lo0 itself
    int w = lo[k] >> 5;
    while (bits[k] == 0u && ++w < nw) bits[k] = pos[w];
    out[k] = bits[k] ? (w << 5) + __builtin_ctz(bits[k]) : last;
  }
}

}  // namespace bornvi
