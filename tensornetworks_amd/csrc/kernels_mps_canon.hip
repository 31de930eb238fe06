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
// mc_jacobi, mc_rescale and the cut (mc_cut) are mps_canon_dev.hpp's, shared with the two-site sweeps, and stated there.
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
#include "mps_canon_dev.hpp"
#include "mps_sample_dev.hpp"

namespace bornvi {

namespace {

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
    double total, dropped, ksum;
    const int r = mc_cut(D, Do, cutoff, sorted, total, dropped, ksum);
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
