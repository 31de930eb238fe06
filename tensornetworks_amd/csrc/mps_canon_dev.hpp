// The one definition of the one-workgroup Jacobi factorisation, its rank rule and the cut rule of DESIGN.md section 6n, shared by
// kernels_mps_canon.hip (canonical form) and kernels_mps_twosite.hip (two-site sweeps): the same text, so the same singular
// values, the same exact zeros and the same kept ranks in both.  Every routine is called by all MC_THREADS = 256 threads of a
// workgroup.
//
// mc_jacobi: one-sided (Hestenes) Jacobi on the columns of a matrix of rows <= 64 and D <= 32 columns in LDS (column-major, pitch
//   64), rotations accumulated in V (column-major, pitch 32).  Pairs in round-robin tournament order (mc_pair: the circle method
//   on D rounded up to even players): D / 2 disjoint pairs per round, D - 1 rounds a sweep (D rounds, one column idle in each,
//   for odd D); pair p of a round is rotated by the 16 lanes 16 p .. 16 p + 15, lane l owning the rows l, l + 16, l + 32, l + 48.
//   a = |g_i|^2, b = |g_j|^2, c = g_i . g_j are fixed-order sums by the rule of reduce_dev.hpp: each lane's rows in index order
//   (an fma chain), then a butterfly over the group's 16 lanes, offsets 8 .. 1 (every lane ends with the same bits, so the
//   group decides as one; written out as stein_pairs_kernel writes its own: wave_sum has no width parameter).  The pair rotates
//   when |c| > rows EPS64 sqrt(a) sqrt(b).  At most MC_MAX_SWEEPS sweeps; a sweep without a rotation ends the loop: the
//   decision is one flag in LDS that every lane reads after the sweep's last barrier, so the exit is workgroup-uniform.
//
// THE RANK RULE.  A pair is skipped when either column's squared norm is <= (D EPS64)^2 times the largest squared column norm
//   of the matrix as it was given to the routine, and such a column's singular value is reported as exactly 0.0.
//
// THE CUT (mc_cut), of D values sorted descending: cumulative squares from the small end; the values behind D_out go, then
//   more from the small end for as long as the dropped squares' normalised sum stays <= cutoff; one value always stays.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "mps_sample_dev.hpp"

namespace bornvi {

constexpr int MC_THREADS = 256;
constexpr int MC_GROUP = 16;              // lanes per column pair
constexpr int MC_ROWS = 64;               // pitch of the matrix (2 MS_DMAX rows)
constexpr int MC_MAX_SWEEPS = 30;         // a cap, not a tuning: the tests' largest count is in DESIGN.md section 6n
constexpr double MC_EPS = 2.220446049250313e-16;

__device__ __forceinline__ double mc_group_sum(double v) {
#pragma unroll
  for (int off = MC_GROUP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// pair p of round r among m (even) players: the circle method, player m - 1 fixed; i < j on return
__device__ __forceinline__ void mc_pair(int m, int r, int p, int& i, int& j) {
  int x, y;
  if (p == 0) {
    x = m - 1;
    y = r;
  } else {
    x = (r + p) % (m - 1);
    y = (r - p + (m - 1)) % (m - 1);
  }
  i = x < y ? x : y;
  j = x < y ? y : x;
}

// squared norms of the D columns of G into nrm2[0 .. D): group g takes the columns g and g + 16.  Ends on a barrier.
__device__ __forceinline__ void mc_col_norms(int rows, int D, const double* G, double* nrm2) {
  const int t = threadIdx.x, g = t / MC_GROUP, l = t % MC_GROUP;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int col = g + h * MC_GROUP;
    double a = 0.0;
    if (col < D)
      for (int row = l; row < rows; row += MC_GROUP) {
        const double x = G[col * MC_ROWS + row];
        a = fma(x, x, a);
      }
    a = mc_group_sum(a);
    if (col < D && l == 0) nrm2[col] = a;
  }
  __syncthreads();
}

// G [rows x D] (LDS, column-major, pitch MC_ROWS) -> orthogonal columns, V [D x D] (pitch MS_DMAX) the rotations' product,
// sigma[0 .. D) the singular values (the rank rule's exact zeros).  Begins and ends on a barrier; every lane returns the
// sweep count, negated when the last allowed sweep still rotated.
__device__ __forceinline__ int mc_jacobi(int rows, int D, double* G, double* V, double* sigma, double* nrm2, int* flag) {
  const int t = threadIdx.x, g = t / MC_GROUP, l = t % MC_GROUP;
  __syncthreads();
  for (int i = t; i < D * MS_DMAX; i += MC_THREADS) V[i] = (i / MS_DMAX == i % MS_DMAX) ? 1.0 : 0.0;
  mc_col_norms(rows, D, G, nrm2);
  double mx = 0.0;
  for (int c = 0; c < D; ++c) mx = fmax(mx, nrm2[c]);
  const double thr = (D * MC_EPS) * (D * MC_EPS) * mx;
  const double tol = rows * MC_EPS;
  const int m = D + (D & 1), npairs = m / 2;
  int sweeps = 0;
  bool more = true;
  while (more && sweeps < MC_MAX_SWEEPS) {
    ++sweeps;
    if (t == 0) *flag = 0;
    __syncthreads();
    for (int r = 0; r < m - 1; ++r) {
      int i = 0, j = 0;
      bool live = g < npairs;
      if (live) {
        mc_pair(m, r, g, i, j);
        live = j < D;                      // odd D: the pair with the dummy player idles
      }
      double a = 0.0, b = 0.0, c = 0.0;
      if (live)
        for (int row = l; row < rows; row += MC_GROUP) {
          const double x = G[i * MC_ROWS + row], y = G[j * MC_ROWS + row];
          a = fma(x, x, a);
          b = fma(y, y, b);
          c = fma(x, y, c);
        }
      a = mc_group_sum(a);
      b = mc_group_sum(b);
      c = mc_group_sum(c);
      if (live && a > thr && b > thr && fabs(c) > tol * sqrt(a) * sqrt(b)) {
        const double zeta = (b - a) / (2.0 * c);
        const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
        for (int row = l; row < rows; row += MC_GROUP) {
          const double x = G[i * MC_ROWS + row], y = G[j * MC_ROWS + row];
          G[i * MC_ROWS + row] = cs * x - sn * y;
          G[j * MC_ROWS + row] = sn * x + cs * y;
        }
        for (int row = l; row < D; row += MC_GROUP) {
          const double x = V[i * MS_DMAX + row], y = V[j * MS_DMAX + row];
          V[i * MS_DMAX + row] = cs * x - sn * y;
          V[j * MS_DMAX + row] = sn * x + cs * y;
        }
        if (l == 0) *flag = 1;
      }
      __syncthreads();
    }
    more = *flag != 0;                     // the same word in every lane: the round loop ended on a barrier
    __syncthreads();                       // nobody clears the flag before everybody has read it
  }
  mc_col_norms(rows, D, G, nrm2);
  if (t < D) sigma[t] = nrm2[t] > thr ? sqrt(nrm2[t]) : 0.0;
  __syncthreads();
  return more ? -sweeps : sweeps;
}

// M 2^-e in place, e = ilogb of the largest magnitude of the rows x D matrix (ms_exponent: 0 when it is 0 or not finite)
__device__ __forceinline__ int mc_rescale(int rows, int D, double* G, double* red) {
  const int t = threadIdx.x;
  double mx = 0.0;
  for (int i = t; i < rows * D; i += MC_THREADS) mx = max_nan(mx, fabs(G[(i / rows) * MC_ROWS + i % rows]));
  mx = block_max_nan<MC_THREADS / 64>(mx, red);
  const int e = ms_exponent(mx);
  for (int i = t; i < rows * D; i += MC_THREADS) {
    const int at = (i / rows) * MC_ROWS + i % rows;
    G[at] = ldexp(G[at], -e);
  }
  return e;
}

// the cut of sorted[0 .. D) (descending, in LDS, published by a barrier), by every lane alike: the kept rank is returned,
// total = the sum of all squares, dropped = the sum of the squares of sorted[rank ..], ksum = that of sorted[.. rank)
__device__ __forceinline__ int mc_cut(int D, int Do, double cutoff, const double* sorted, double& total_out, double& dropped_out,
                                      double& ksum_out) {
  double cum = 0.0;
  for (int i = D - 1; i >= 0; --i) cum = fma(sorted[i], sorted[i], cum);
  const double total = cum;
  int r = D;
  double dropped = 0.0;                                // cumulative squares of sorted[r ..]
  for (int i = D - 1; i >= 1; --i) {
    const double next = fma(sorted[i], sorted[i], dropped);
    if (i >= Do || next / total <= cutoff) {
      dropped = next;
      r = i;
    } else {
      break;
    }
  }
  double ksum = 0.0;
  for (int i = r - 1; i >= 0; --i) ksum = fma(sorted[i], sorted[i], ksum);
  total_out = total;
  dropped_out = dropped;
  ksum_out = ksum;
  return r;
}

}  // namespace bornvi
