// Finite-shot measurement: S exact multinomial draws from each of B Born-distribution rows -> frequencies counts / S
// (bornvi_shots_histogram).
//
// Draws are a pure function of (seed, epoch, global circuit id, level, block, draw index) through a counter-based
// Philox4x32-10 (Random123's round function and constants, restated here; no rocRAND):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (m, (level << 24) | block, circuit id, epoch & 0xffffffff) -> 4 words w0..w3;
//   draws 2m and 2m + 1 of that (level, block) take u = ((w1:w0) >> 11) 2^-53 and u = ((w3:w2) >> 11) 2^-53, in [0, 1).
// A row of 2^n outcomes is cut into blocks of 2^12; the block masses form the row of the next level (2^(n-12) entries,
// cut again while longer than one block).  The top level holds one block and gets all S draws; a block with m draws
// (its count at the level above) draws m outcomes from its own contents by rule R (shots_dev.hpp): with cdf the block's
// inclusive prefix sums in the scan's order and lo0 the first i with cdf[i] > u cdf[last], the outcome is the first
// i >= lo0 whose value is positive, or the block's last positive entry if there is none; a block without a positive
// entry counts nothing.  (Where zero entries never raise the cdf -- dyadic rows, any single running sum -- this is
// "first i with cdf[i] > u cdf[last]".  The scan is not one running sum: at a thread boundary a zero entry's cdf can
// exceed its predecessor's by an ulp, and only the positivity mask keeps such an entry, or a zero-mass block, undrawn.)
// Given the counts of the level above, the draws inside a block are conditionally i.i.d. from the block's normalised
// contents, so the level-0 counts are one exact multinomial sample of the row: no normal or Poisson approximation.
// A probability-0 outcome is never drawn, so every row with a positive entry sums to exactly S; a row whose entries are
// all zero yields zeros.
//
// Traffic: the mass kernel reads every row once, the draw kernel reads it once more and writes the frequencies
// (in place allowed: a workgroup reads its whole block into LDS before it writes it): 3 B 2^n 8 bytes.
// Counts are integers kept in LDS per block and written once: no global atomics, deterministic.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "philox_dev.hpp"
#include "reduce_dev.hpp"
#include "shots_dev.hpp"

namespace bornvi {

namespace {
constexpr int SH_BLOCK_BITS = SHOTS_BLOCK_BITS, SH_BLOCK = SHOTS_BLOCK;
constexpr int SH_THREADS = 512, SH_EPT = SH_BLOCK / SH_THREADS;     // draw kernel: 8 consecutive entries per thread in the scan
constexpr int SM_THREADS = 256, SM_EPT = SH_BLOCK / SM_THREADS;     // mass kernel

// global circuit id of batch row r in the layout of bornvi_paramshift_probs_strided: base = 0, +p = 2p + 1, -p = 2p + 2
__device__ __forceinline__ uint32_t circuit_id(long long r, int include_base, int p_begin, int p_stride) {
  if (include_base) {
    if (r == 0) return 0u;
    --r;
  }
  const long long p = p_begin + (r >> 1) * (long long)p_stride;
  return (uint32_t)(2 * p + 1 + (r & 1));
}

// masses[row][b] = sum of block b of row `row` of src ([B][len], len = nblk * 2^12); grid = nblk * B workgroups
__global__ __launch_bounds__(SM_THREADS) void shots_mass_kernel(const double* __restrict__ src, long long len, long long nblk,
                                                                double* __restrict__ masses) {
  __shared__ double part[SM_THREADS / 64];
  const long long g = blockIdx.x;
  const double* __restrict__ p = src + (g / nblk) * len + (g % nblk) * SH_BLOCK;
  const int t = threadIdx.x;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < SM_EPT; ++i) s += p[t + i * SM_THREADS];
  s = wave_sum(s);
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < SM_THREADS / 64; ++w) tot += part[w];
    masses[g] = tot;
  }
}

// One workgroup per (row, block of `blk` entries): draws the block's m outcomes (m = counts_in[row][b], or `shots` at the
// top level) and writes either frequencies count / shots (level 0, into freq) or integer counts (into counts_out).
__global__ __launch_bounds__(SH_THREADS) void shots_draw_kernel(const double* src, long long len, int blk, long long nblk,
                                                                const int* __restrict__ counts_in, double* freq,
                                                                int* __restrict__ counts_out, int shots, uint32_t seed_lo,
                                                                uint32_t seed_hi, const long long* __restrict__ epoch_dev,
                                                                int level, int include_base, int p_begin, int p_stride) {
  __shared__ double cdf[SH_BLOCK];
  __shared__ int hist[SH_BLOCK];
  __shared__ double tsum[2][SH_THREADS];
  __shared__ uint32_t pos[SHOTS_MASK_WORDS];      // bit i: entry i is positive; thread t owns byte t (its 8 entries)
  __shared__ int lastnz;
  const int t = threadIdx.x;
  const long long g = blockIdx.x;
  const long long row = g / nblk, b = g % nblk;
  const long long base = row * len + b * (long long)blk;
  const int m = counts_in ? counts_in[g] : shots;

  for (int i = t; i < blk; i += SH_THREADS) {
    cdf[i] = src[base + i];
    hist[i] = 0;
  }
  if (t == 0) {
    lastnz = -1;
    pos[SHOTS_MASK_WORDS - 1] = 0u;
  }
  __syncthreads();
  // inclusive scan: 8 consecutive entries per thread, then a scan of the 512 thread totals
  const int c0 = t * SH_EPT, c1 = min(c0 + SH_EPT, blk);
  double run = 0.0;
  int nz = -1;
  uint32_t mybits = 0u;
  for (int i = c0; i < c1; ++i) {
    const double v = cdf[i];
    if (v > 0.0) {
      nz = i;
      mybits |= 1u << (i - c0);
    }
    run += v;
    cdf[i] = run;
  }
  reinterpret_cast<unsigned char*>(pos)[t] = (unsigned char)mybits;     // little-endian: bit (8t + k) & 31 of word t >> 2
  if (nz >= 0) atomicMax(&lastnz, nz);
  tsum[0][t] = run;
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < SH_THREADS; off <<= 1) {
    const double v = tsum[cur][t] + (t >= off ? tsum[cur][t - off] : 0.0);
    tsum[cur ^ 1][t] = v;
    cur ^= 1;
    __syncthreads();
  }
  if (t > 0 && c0 < c1) {
    const double pre = tsum[cur][t - 1];
    for (int i = c0; i < c1; ++i) cdf[i] = pre + cdf[i];
  }
  __syncthreads();

  const int last = lastnz;
  if (m > 0 && last >= 0) {
    const double total = cdf[blk - 1];
    const uint32_t cid = circuit_id(row, include_base, p_begin, p_stride);
    const uint32_t ep = (uint32_t)(unsigned long long)(*epoch_dev);
    const uint32_t lb = ((uint32_t)level << 24) | (uint32_t)b;
    const int npairs = (int)(((long long)m + 1) >> 1);
    for (int pr = t; pr < npairs; pr += SH_THREADS) {
      const uint4 w = philox4x32_10(make_uint4((uint32_t)pr, lb, cid, ep), seed_lo, seed_hi);
      const double x[2] = {unit53(w.x, w.y) * total, unit53(w.z, w.w) * total};
      int pick[2];                            // both draws of the call are searched together; an odd m drops the last
      shots_pick<2>(cdf, pos, blk, last, x, pick);
      atomicAdd(&hist[pick[0]], 1);
      if (2 * pr + 1 < m) atomicAdd(&hist[pick[1]], 1);
    }
  }
  __syncthreads();
  if (counts_out) {
    for (int i = t; i < blk; i += SH_THREADS) counts_out[base + i] = hist[i];
  } else {
    const double S = (double)shots;
    for (int i = t; i < blk; i += SH_THREADS) freq[base + i] = (double)hist[i] / S;
  }
}

// entries of every level above level 0: 2^(n-12), 2^(n-24), ... while the level below is longer than one block
int shot_levels(int n, long long* lens) {
  int L = 0;
  long long len = 1ll << n;
  lens[L++] = len;
  while (len > SH_BLOCK) {
    len >>= SH_BLOCK_BITS;
    lens[L++] = len;
  }
  return L;
}
}  // namespace

size_t shots_workspace_bytes(int n, long long B) {
  long long lens[8];
  const int L = shot_levels(n, lens);
  size_t bytes = 256;
  for (int l = 1; l < L; ++l) bytes += (size_t)B * lens[l] * (sizeof(double) + sizeof(int)) + 256;
  return bytes;
}

hipError_t launch_shots_histogram(int n, long long B, const double* probs, double* freq, int shots, unsigned long long seed,
                                  const long long* epoch_dev, int include_base, int p_begin, int p_stride, void* ws,
                                  hipStream_t st) {
  if (B == 0) return hipSuccess;
  long long lens[8];
  const int L = shot_levels(n, lens);
  double* masses[8] = {nullptr};
  int* counts[8] = {nullptr};
  char* w = ws_align(ws);
  for (int l = 1; l < L; ++l) {
    masses[l] = (double*)w;
    counts[l] = (int*)(w + (size_t)B * lens[l] * sizeof(double));
    w += ws_round((size_t)B * lens[l] * (sizeof(double) + sizeof(int)));
  }
  const uint32_t slo = (uint32_t)seed, shi = (uint32_t)(seed >> 32);
  for (int l = 0; l + 1 < L; ++l) {
    const long long nblk = lens[l] >> SH_BLOCK_BITS;
    hipLaunchKernelGGL(shots_mass_kernel, dim3((unsigned)(nblk * B)), dim3(SM_THREADS), 0, st, l ? masses[l] : probs, lens[l],
                       nblk, masses[l + 1]);
  }
  for (int l = L - 1; l >= 0; --l) {
    const int blk = (int)(lens[l] < SH_BLOCK ? lens[l] : SH_BLOCK);
    const long long nblk = lens[l] / blk;
    hipLaunchKernelGGL(shots_draw_kernel, dim3((unsigned)(nblk * B)), dim3(SH_THREADS), 0, st, l ? masses[l] : probs, lens[l],
                       blk, nblk, l + 1 < L ? counts[l + 1] : nullptr, l ? nullptr : freq, l ? counts[l] : nullptr, shots,
                       slo, shi, epoch_dev, l, include_base, p_begin, p_stride);
  }
  return hipGetLastError();
}

}  // namespace bornvi
