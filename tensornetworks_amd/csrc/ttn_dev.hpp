// The tree-tensor-network kernels' shared device functions (kernels_ttn.hip): the tree's geometry, the
// live entries of a node's tensor, a node's tensor in LDS and the one definition of x_v, so that the sampler's logq and the
// score call's are the same bits because they are the same code.  Host- and device-includable for the geometry.
//
// Vectors: one sample per lane, DP doubles (DP = bond_dp(D) = 2, 4, 8 >= D, zero padded) in registers.  A node's tensor is
//   zero-padded to DP x DP x DP in LDS, Ts[(p DP + a) DP + b], with its dead entries read as 0.0 whatever they hold.
// A vector that waits between two nodes lives in a slot [entry][lane] (TT_LANES doubles per entry), in LDS or in the
//   workgroup's slice of the workspace: coalesced over the wave either way.
#pragma once
#include <hip/hip_runtime.h>

#include "mps_sample_dev.hpp"

namespace bornvi {

constexpr int TT_LANES = 64;      // one wave per workgroup: a tile of 64 samples
constexpr int TT_MAX_H = 6;       // L = 2^h <= 64

__host__ __device__ inline int ttn_height(int n) {
  int h = 1;
  while ((1 << h) < n) ++h;
  return h;
}

// the entries that enter psi: not the root at p >= 1, not a bottom node at a >= 2 or b >= 2 or at the value 1 of a padding child
__host__ __device__ inline bool ttn_live(int v, int p, int a, int b, int L, int n) {
  if (v == 1 && p != 0) return false;
  if (2 * v >= L) {
    const int j = 2 * v - L;      // the left child's position
    if (a >= 2 || b >= 2) return false;
    if (a == 1 && j >= n) return false;
    if (b == 1 && j + 1 >= n) return false;
  }
  return true;
}

__device__ __forceinline__ double ttn_core(const double* cores, int v, int p, int a, int b, int D, int L, int n) {
  return ttn_live(v, p, a, b, L, n) ? cores[(((long long)(v - 1) * D + p) * D + a) * D + b] : 0.0;
}

// T_v zero-padded and masked into Ts (DP^3 doubles), and optionally a [D, D, D] array M the same way (unmasked) into Ms
template <int DP>
__device__ __forceinline__ void ttn_load_node(const double* cores, int v, int D, int L, int n, double* Ts, const double* M, double* Ms) {
  for (int i = threadIdx.x; i < DP * DP * DP; i += TT_LANES) {
    const int p = i / (DP * DP), a = (i / DP) % DP, b = i % DP;
    const bool in = p < D && a < D && b < D;
    Ts[i] = in ? ttn_core(cores, v, p, a, b, D, L, n) : 0.0;
    if (M) Ms[i] = in ? M[(p * D + a) * D + b] : 0.0;
  }
}

// the value of position j in the index word z (0 for padding) as the one-hot leaf vector
template <int DP>
__device__ __forceinline__ void ttn_leaf(double (&x)[DP], unsigned long long z, int j, int n) {
  const int bit = j < n ? (int)((z >> (n - 1 - j)) & 1ull) : 0;
#pragma unroll
  for (int a = 0; a < DP; ++a) x[a] = a == bit ? 1.0 : 0.0;
}

template <int DP>
__device__ __forceinline__ void ttn_leaf_bit(double (&x)[DP], bool bit) {
#pragma unroll
  for (int a = 0; a < DP; ++a) x[a] = a == (bit ? 1 : 0) ? 1.0 : 0.0;
}

// x_v = (T x_l) x_r: M[p][b] = sum_a T[p, a, b] x_l[a], one fma chain over a, then x[p] = sum_b M[p][b] x_r[b], one chain over b;
// then times 2^-e, e returned
template <int DP>
__device__ __forceinline__ int ttn_node_up(const double* Ts, const double (&xl)[DP], const double (&xr)[DP], double (&x)[DP]) {
#pragma unroll
  for (int p = 0; p < DP; ++p) {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < DP; ++b) {
      double m = 0.0;
#pragma unroll
      for (int a = 0; a < DP; ++a) m = fma(Ts[(p * DP + a) * DP + b], xl[a], m);
      acc = fma(m, xr[b], acc);
    }
    x[p] = acc;
  }
  return ms_rescale<DP>(x);
}

template <int DP>
__device__ __forceinline__ void ttn_slot_load(const double* slot, int lane, double (&x)[DP]) {
#pragma unroll
  for (int a = 0; a < DP; ++a) x[a] = slot[a * TT_LANES + lane];
}

template <int DP>
__device__ __forceinline__ void ttn_slot_store(double* slot, int lane, const double (&x)[DP]) {
#pragma unroll
  for (int a = 0; a < DP; ++a) slot[a * TT_LANES + lane] = x[a];
}

}  // namespace bornvi
