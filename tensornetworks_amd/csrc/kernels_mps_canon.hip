// Canonical form, bond spectra and truncation of an MPS.  Conventions of kernels_mps_sample.hip: cores
// [n, 2, D, D] float64, 1 <= n <= 63, 1 <= D <= 32, psi(z) = e0^T A_1[z_1] .. A_n[z_n] e0; only row 0 of the first core and column
// 0 of the last enter psi.  bornvi_mps_canonicalise is one workgroup of MC_THREADS = 256 that walks the chain twice:
//
//   left, k = 1 .. n - 1:   M = [C A_k[0]; C A_k[1]] (2 D x D), C_0 = e0 e0^T;  M 2^-e = Q (S V^T) by mc_jacobi;  Q_k[s] = the
//                           blocks of Q, kept in the workspace;  C = S V^T / |S V^T|_F;  log += log |S V^T|_F + e ln 2.
//                           Then T_n[s] = C A_n[s] beside the Q_k.
//   right, k = n .. 2:      M = [T_k[0] R, T_k[1] R] (D x 2 D), T_k = Q_k for k < n, R_n = e0 e0^T;  M^T 2^-e = G V^T by mc_jacobi,
//                           so M = V S W with the rows of W the normalised columns of G;  sigma sorted descending, ties by
//                           index;  schmidt[k - 2] = sigma / |sigma|;  the cut: cumulative squares from the small end, the
//                           values behind D_out go, then more from the small end for as long as the dropped squares'
//                           normalised sum stays <= cutoff, one value always stays;  A_k[s] = the kept rows of W's blocks;
//                           R = (V S)[:, kept] / |S[kept]|.  At k = n:  log += log |sigma| + e ln 2.
//   last:                   A_1[s] = Q_1[s] R;  log_norm = 2 log.  n = 1: the one core over its norm.
//   e is ilogb of M's largest magnitude (an exact scaling), so cores of any representable scale neither overflow nor vanish.
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
//   of the matrix as it was given to the routine, and such a column's singular value is reported as exactly 0.0 (its column of
//   Q, or row of W, as zeros).  Without it two columns of pure rounding noise never pass the rotation test, and rank deficiency
//   is the normal case here (bond k has rank <= min(2^k, 2^(n-k)); zero-padded and expanded models have null columns).
//
// Status: 1 when the input holds a non-finite entry (decided before any sweep) or log Z is not finite (cores_out, log_norm
//   NaN); 4 when a factorisation used all MC_MAX_SWEEPS sweeps and still rotated.  The workspace's first int keeps the largest
//   sweep count of the call's factorisations.  Every index is a function of (n, D, D_out, k, lane) except the sort's
//   permutation, whose entries are masked to 0 .. 31 and address LDS arrays of 32.
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "mps_sample_dev.hpp"

namespace bornvi {

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_GROUP = 16;              // lanes per column pair
constexpr int MC_ROWS = 64;               // pitch of the matrix (2 MS_DMAX rows)
constexpr int MC_MAX_SWEEPS = 30;         // a cap, not a tuning: the tests' largest count is in DESIGN.md section 6n
constexpr double MC_EPS = 2.220446049250313e-16;

struct McLayout {
  size_t hdr, T, total;
};

McLayout mc_layout(int n, int D) {
  McLayout S;
  size_t o = 0;
  S.hdr = o; o += 256;                                                  // int 0: the largest sweep count
  S.T = o;   o += ws_round((size_t)n * 2 * D * D * sizeof(double));     // Q_1 .. Q_{n-1}, T_n
  S.total = o;
  return S;
}

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

__global__ __launch_bounds__(MC_THREADS) void mps_canon_kernel(const double* __restrict__ cores, int n, int D, int Do, double cutoff,
                                                              double* __restrict__ out, double* __restrict__ schmidt,
                                                              double* __restrict__ discarded, int* __restrict__ rank,
                                                              double* __restrict__ log_norm, int* __restrict__ status,
                                                              double* Tws, int* __restrict__ hdr) {
  __shared__ double G[MS_DMAX * MC_ROWS];          // 16 KB: the matrix under factorisation
  __shared__ double V[MS_DMAX * MS_DMAX];          //  8 KB: the rotations
  __shared__ double Cm[MS_DMAX * MS_DMAX];         //  8 KB: the carry, row-major, pitch D
  __shared__ double As[2 * MS_DMAX * MS_DMAX];     // 16 KB: the site's two matrices, pitch D
  __shared__ double sigma[MS_DMAX], nrm2[MS_DMAX], sorted[MS_DMAX];
  __shared__ double red[MC_THREADS / 64];
  __shared__ int perm[MS_DMAX];
  __shared__ int flag;
  const int t = threadIdx.x, DD = D * D;
  const long long total_in = (long long)n * 2 * DD, total_out = (long long)n * 2 * Do * Do;
  const double nan = __builtin_nan("");

  // a non-finite entry anywhere: status 1, before any sweep
  double bad = 0.0;
  for (long long i = t; i < total_in; i += MC_THREADS) bad = max_nan(bad, isfinite(cores[i]) ? 0.0 : nan);
  bad = block_max_nan<MC_THREADS / 64>(bad, red);
  if (bad != bad) {                                // uniform: block_max_nan gives every lane the same bits
    for (long long i = t; i < total_out; i += MC_THREADS) out[i] = nan;
    for (int i = t; i < (n - 1) * D; i += MC_THREADS) schmidt[i] = nan;
    for (int i = t; i < n - 1; i += MC_THREADS) {
      discarded[i] = nan;
      rank[i] = 0;
    }
    if (t == 0) {
      *log_norm = nan;
      *status = 1;
      hdr[0] = 0;
    }
    return;
  }

  int st = 0, max_sweeps = 0;
  double logacc = 0.0;
  for (int i = t; i < DD; i += MC_THREADS) Cm[i] = i == 0 ? 1.0 : 0.0;

  // ---- left sweep ----  (site loads and C A_k[s] stay written out, not ms_load_site_wg's: profiles/mps_env_core_isa.txt)
  for (int k = 1; k < n; ++k) {
    __syncthreads();
    for (int i = t; i < 2 * DD; i += MC_THREADS) As[i] = cores[(long long)(k - 1) * 2 * DD + i];
    __syncthreads();
    for (int i = t; i < 2 * DD; i += MC_THREADS) {       // M[s D + a][b] = sum_e C[a][e] A[s][e][b]
      const int s = i / DD, a = (i % DD) / D, b = i % D;
      double acc = 0.0;
      for (int e = 0; e < D; ++e) acc = fma(Cm[a * D + e], As[s * DD + e * D + b], acc);
      G[b * MC_ROWS + s * D + a] = acc;
    }
    __syncthreads();
    const int ex = mc_rescale(2 * D, D, G, red);
    const int sw = mc_jacobi(2 * D, D, G, V, sigma, nrm2, &flag);
    if (sw < 0) st |= 4;
    max_sweeps = max(max_sweeps, sw < 0 ? -sw : sw);
    for (int i = t; i < 2 * DD; i += MC_THREADS) {       // Q_k[s][a][j]
      const int s = i / DD, a = (i % DD) / D, j = i % D;
      const double sg = sigma[j];
      Tws[(long long)(k - 1) * 2 * DD + i] = sg > 0.0 ? G[j * MC_ROWS + s * D + a] / sg : 0.0;
    }
    double part = 0.0;
    for (int i = t; i < DD; i += MC_THREADS) {           // C[j][b] = sigma_j V[b][j]
      const int j = i / D, b = i % D;
      const double v = sigma[j] * V[j * MS_DMAX + b];
      Cm[i] = v;
      part = fma(v, v, part);
    }
    const double nrm = sqrt(block_sum<MC_THREADS / 64>(part, red));
    for (int i = t; i < DD; i += MC_THREADS) Cm[i] = Cm[i] / nrm;
    logacc += log(nrm) + ex * MS_LN2;
  }
  // T_n[s] = C A_n[s]
  __syncthreads();
  for (int i = t; i < 2 * DD; i += MC_THREADS) As[i] = cores[(long long)(n - 1) * 2 * DD + i];
  __syncthreads();
  for (int i = t; i < 2 * DD; i += MC_THREADS) {
    const int s = i / DD, a = (i % DD) / D, b = i % D;
    double acc = 0.0;
    for (int e = 0; e < D; ++e) acc = fma(Cm[a * D + e], As[s * DD + e * D + b], acc);
    Tws[(long long)(n - 1) * 2 * DD + i] = acc;
  }
  __syncthreads();                                       // Cm becomes R; Tws is read back by the threads that wrote it or after a barrier
  for (int i = t; i < DD; i += MC_THREADS) Cm[i] = i == 0 ? 1.0 : 0.0;

  // ---- right sweep ----
  for (int k = n; k >= 2; --k) {
    __syncthreads();
    for (int i = t; i < 2 * DD; i += MC_THREADS) As[i] = Tws[(long long)(k - 1) * 2 * DD + i];
    __syncthreads();
    for (int i = t; i < 2 * DD; i += MC_THREADS) {       // M^T[s D + b][a] = sum_e T[s][a][e] R[e][b]
      const int s = i / DD, a = (i % DD) / D, b = i % D;
      double acc = 0.0;
      for (int e = 0; e < D; ++e) acc = fma(As[s * DD + a * D + e], Cm[e * D + b], acc);
      G[a * MC_ROWS + s * D + b] = acc;
    }
    __syncthreads();
    const int ex = mc_rescale(2 * D, D, G, red);
    const int sw = mc_jacobi(2 * D, D, G, V, sigma, nrm2, &flag);
    if (sw < 0) st |= 4;
    max_sweeps = max(max_sweeps, sw < 0 ? -sw : sw);
    // descending, ties by index: the place of a value is the count of those in front of it
    if (t < D) perm[t] = t;
    __syncthreads();
    if (t < D) {
      const double mine = sigma[t];
      int pos = 0;
      for (int c = 0; c < D; ++c) {
        const double o = sigma[c];
        pos += (o > mine || (o == mine && c < t)) ? 1 : 0;
      }
      perm[pos & (MS_DMAX - 1)] = t;
      sorted[pos & (MS_DMAX - 1)] = mine;
    }
    __syncthreads();
    // the cut, by every lane alike from LDS
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
    const double snorm = sqrt(total), knorm = sqrt(ksum);
    if (t < D) schmidt[(long long)(k - 2) * D + t] = sorted[t] / snorm;
    if (t == 0) {
      discarded[k - 2] = r < D ? dropped / total : 0.0;
      rank[k - 2] = r;
    }
    if (k == n) logacc += log(snorm) + ex * MS_LN2;
    for (int i = t; i < 2 * Do * Do; i += MC_THREADS) {  // A_k[s][j'][b] = W[p(j')][s D + b]
      const int s = i / (Do * Do), jp = (i / Do) % Do, b = i % Do;
      double v = 0.0;
      if (jp < r && !(k == n && b > 0)) {
        const int j = perm[jp] & (MS_DMAX - 1);
        const double sg = sigma[j];
        if (sg > 0.0) v = G[j * MC_ROWS + s * D + b] / sg;
      }
      out[(long long)(k - 1) * 2 * Do * Do + i] = v;
    }
    __syncthreads();                                     // the product above is done with Cm
    for (int i = t; i < DD; i += MC_THREADS) {           // R[a][j'] = V[a][p(j')] sigma_p(j') / |S[kept]|
      const int a = i / D, jp = i % D;
      double v = 0.0;
      if (jp < r) {
        const int j = perm[jp] & (MS_DMAX - 1);
        v = V[j * MS_DMAX + a] * sigma[j] / knorm;
      }
      Cm[i] = v;
    }
  }

  // ---- site 1 ----
  __syncthreads();
  for (int i = t; i < 2 * DD; i += MC_THREADS) As[i] = Tws[i];
  __syncthreads();
  if (n == 1) {
    const double a0 = As[0], a1 = As[DD];
    const double nrm = sqrt(fma(a1, a1, a0 * a0));
    logacc += log(nrm);
    for (int i = t; i < 2 * Do * Do; i += MC_THREADS) out[i] = i == 0 ? a0 / nrm : i == Do * Do ? a1 / nrm : 0.0;
  } else {
    for (int i = t; i < 2 * Do * Do; i += MC_THREADS) {
      const int s = i / (Do * Do), a = (i / Do) % Do, b = i % Do;
      double acc = 0.0;
      if (a == 0)
        for (int e = 0; e < D; ++e) acc = fma(As[s * DD + e], Cm[e * D + b], acc);
      out[i] = acc;
    }
  }
  const double ln = 2.0 * logacc;
  if (!isfinite(ln)) {                                   // Z is not positive and finite; the same bits in every lane
    st |= 1;
    __syncthreads();
    for (long long i = t; i < total_out; i += MC_THREADS) out[i] = nan;
  }
  if (t == 0) {
    *log_norm = isfinite(ln) ? ln : nan;
    *status = st;
    hdr[0] = max_sweeps;
  }
}

}  // namespace

size_t mps_canon_workspace_bytes(int n, int D) { return mc_layout(n, D).total + 256; }

hipError_t launch_mps_canonicalise(int n, int D, int D_out, double cutoff, const double* cores, double* cores_out, double* schmidt,
                                   double* discarded, int* rank, double* log_norm, int* status, void* ws, hipStream_t st) {
  const McLayout S = mc_layout(n, D);
  char* base = ws_align(ws);
  mps_canon_kernel<<<1, MC_THREADS, 0, st>>>(cores, n, D, D_out, cutoff, cores_out, schmidt, discarded, rank, log_norm, status,
                                            (double*)(base + S.T), (int*)(base + S.hdr));
  return hipGetLastError();
}

}  // namespace bornvi
