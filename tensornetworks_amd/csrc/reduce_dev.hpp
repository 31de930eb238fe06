// The kernels' one definition of their fixed-order reductions, of the chunk geometry their partials
// come from, and of the bond-dimension padding of the MPS kernels.  Host- and device-includable, so that a host driver can
// execute the geometry's own text (tests/test_reduce_host.py).
//
// The rule.  A long sum is: each thread's elements in index order; a butterfly over the 64 lanes of a wave (offsets 32 down
// to 1: every lane ends with the same bits); the wave totals, through LDS, in wave order; and where more than one workgroup
// takes part, one partial per workgroup in the workspace, added the same way by a finishing step.  No atomics: two calls are
// bitwise equal.  The Python mirrors and the extended-precision bounds of the tests restate exactly this order.
//
// Not here, on purpose: the circuit pass kernels' butterflies (inside hand-scheduled macros), syrk::sum_partials (a serial
// sum per output element), block_softmax_stats (a (max, sum) pair) and the per-lane fma chains of the MPS sweeps.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace bornvi {

// ---- chunk geometry ---------------------------------------------------------------------------------------------
// `count` elements over G workgroups of `chunk` consecutive elements each: about per_wg elements per workgroup, at most
// max_wg workgroups (longer chunks then), the chunk rounded up to a multiple of `align`, no empty workgroup.  count >= 1.
struct ChunkGeom {
  long long chunk;   // elements per workgroup (a multiple of align)
  int G;             // workgroups = partials
};

__host__ __device__ inline ChunkGeom chunk_geom(long long count, long long per_wg, long long max_wg, int align) {
  long long G = (count + per_wg - 1) / per_wg;
  if (G > max_wg) G = max_wg;
  if (G < 1) G = 1;
  long long chunk = (count + G - 1) / G;
  chunk = (chunk + align - 1) / align * align;
  G = (count + chunk - 1) / chunk;
  return {chunk, (int)G};
}

// ---- bond dimension ---------------------------------------------------------------------------------------------
// The MPS kernels are instantiated for the padded bond dimensions DP = 2, 4, 8, 16, 32; a D x D matrix is zero-padded to DP x DP.
__host__ __device__ inline int bond_dp(int D) { return D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }

// CALL with `DP` a constant expression equal to DPV (= bond_dp(D))
#define BOND_DISPATCH(DPV, CALL)                      \
  switch (DPV) {                                      \
    case 2: { constexpr int DP = 2; CALL; } break;    \
    case 4: { constexpr int DP = 4; CALL; } break;    \
    case 8: { constexpr int DP = 8; CALL; } break;    \
    case 16: { constexpr int DP = 16; CALL; } break;  \
    default: { constexpr int DP = 32; CALL; } break;  \
  }

// ---- within a wave ----------------------------------------------------------------------------------------------
// Sum over the 64 lanes, butterfly offsets 32 .. 1: every lane gets the same bits.  (stein_pairs_kernel's sum over the 16 lanes
// of a row, offsets 8 .. 1, stays written out there: as a call of a width-templated wave_sum its instruction stream differs,
// profiles/reduce_core_isa.txt, so this function has no width parameter.)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// fmax: a NaN is DROPPED where the other operand is a number
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// the maximum that KEEPS a NaN: NaN if either operand is one
__device__ __forceinline__ double max_nan(double a, double b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }

__device__ __forceinline__ double wave_max_nan(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max_nan(v, __shfl_xor(v, off));
  return v;
}

// ---- within a workgroup of WAVES waves --------------------------------------------------------------------------
// lds: WAVES doubles.  Called by every thread (barriers inside); every thread gets the same bits.  The leading barrier is
// there because lds may still be read by the reduction before this one (two sums in a row share the array).
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* lds) {
  v = wave_sum(v);
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) lds[t >> 6] = v;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) tot += lds[i];
  return tot;
}

// NaN-keeping maximum of magnitudes (v >= 0 or NaN: the wave totals are folded into 0), same shape as block_sum
template <int WAVES>
__device__ __forceinline__ double block_max_nan(double v, double* lds) {
  v = wave_max_nan(v);
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) lds[t >> 6] = v;
  __syncthreads();
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) m = max_nan(m, lds[i]);
  return m;
}

// part[0 .. count): thread t adds the elements t, t + THREADS, ... in index order, then block_sum.  The same bits in every
// workgroup that asks.  No stride: the strided or offset loops that could have used one keep their own code, the two of
// kernels_born_table.hip (row_stats, the entropy kernel) because through this function their kernels' instruction counts
// change and born_table_probs at n = 3 then missed the timing criterion by 0.1 us (profiles/reduce_core_ab.jsonl), the
// finishing loops that add two partials at once because that is another shape.
template <int THREADS, int WAVES = THREADS / 64>
__device__ __forceinline__ double sum_partials(const double* part, int count, double* lds) {
  static_assert(THREADS == 64 * WAVES, "whole waves");
  double v = 0.0;
  for (int k = threadIdx.x; k < count; k += THREADS) v += part[k];
  return block_sum<WAVES>(v, lds);
}

}  // namespace bornvi
