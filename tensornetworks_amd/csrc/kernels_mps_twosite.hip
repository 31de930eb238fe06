// Two-site (DMRG-style) sweeps of the sampled MPS Born machine.  Conventions of kernels_mps_sample.hip and
// kernels_mps_canon.hip: cores [n, 2, D, D] float64, psi(z) = e0^T A_1[z_1] .. A_n[z_n] e0, z_k = bit n - k of the index word;
// here 2 <= n <= 63, 1 <= D <= 16, 1 <= B <= 2^20.
//
// ON ENTRY the sites 2 .. n are right-canonical and Z = 1 (what bornvi_mps_canonicalise writes).  Samples idx [B], weights w [B]
// (NULL: 1 / B each).  One call is a ROUND TRIP: the bonds k = 1 .. n - 1 left to right, then n - 1 .. 1 right to left; the
// output has the entry gauge again.  AT BOND (k, k + 1), visited as the j-th, j = 0 .. 2 (n - 1) - 1:
//   M[s, t] = A_k[s] A_{k+1}[t], four D x D blocks; in this gauge Z = |M|_F^2.
//   psi_b = l_b^T M[s_b, t_b] r_b,  l_b = e0^T A_1 .. A_{k-1},  r_b = A_{k+2} .. A_n e0 of the sample's own bits: one fma chain
//     over a (outer) and c (inner),  acc = fma(l[a] r[c], M[a][c], acc).
//   A sample COUNTS at this bond when psi_b is finite and not 0; W = the sum of the w_b that count.
//   L = W log |M|^2 - sum_b w_b log psi_b^2,   dL/dM = 2 (W M / |M|^2 - sum_b (w_b / psi_b) l_b r_b^T at block [s_b, t_b]).
//   `steps` plain descent steps, each  M <- M - lr dL/dM,  M <- M / |M|_F;  loss[j] = L after the last one.
//   The split: M unfolded to 2 D x 2 D, rows (s, a), columns (t, c); M 2^-e = G V^T by mc_jacobi on its columns (e = ilogb of the
//     largest magnitude), so M = U S V^T with U the normalised columns of G; sigma sorted descending, ties by index; the cut is
//     mc_cut with D_keep and cutoff (the rank rule's exact zeros go first: they add nothing to the dropped sum); with
//     s_j = sigma_j / |sigma_kept|:   going right  A_k = U_kept, A_{k+1} = s V_kept^T;   going left  A_k = U_kept s, A_{k+1} = V_kept^T.
//     Everything beyond the kept rank is exactly 0.0, and so are the first core's rows >= 1 and the last core's columns >= 1.
//   The samples' vectors advance through the new core:  l_b <- l_b A_k[s_b] (going right),  r_b <- A_{k+1}[t_b] r_b (going left).
//   On the return pass: schmidt[k - 1] = the kept s_j, descending, then 0.0; rank[k - 1]; discarded[k - 1] = the dropped squares over all.
// No exponents are tracked: in canonical gauge every vector has norm <= 1 and psi_b^2 = q(z_b).
//
// THE VECTORS live in the workspace for the whole call: slot j = 1 .. n of B' = 64 ceil(B / 64) samples, entry a of sample b at
//   ((j - 1) D + a) B' + b (64-bit), so that one sample per lane reads and writes 64 consecutive doubles.  Slot j holds
//   l_j = e0^T A_1 .. A_j where the sweep has passed and r_j = A_j .. A_n e0 where it has not.  mts_right_kernel builds r_n .. r_3
//   once; bond (k, k + 1) reads slot k - 1 (e0 at k = 1) and slot k + 2 (e0 at k = n - 1); the advance overwrites slot k (going
//   right) or slot k + 1 (going left).
//
// KERNELS, all on the caller's stream in one chain:  the status clear;  mts_init_kernel (a non-finite core entry: the bad flag;
//   the header's words);  mts_right_kernel;  mts_bond_kernel FORM of bond 1;  then per bond  `steps` x (mts_accum_kernel,
//   mts_bond_kernel STEP),  mts_accum_kernel,  mts_bond_kernel SPLIT (which also forms the next bond's M),  mts_advance_kernel
//   (its own launch; none after the last bond of either pass).
//   mts_accum_kernel: at most MT_MAX_WG workgroups of one wave, workgroup g walks the 64-sample tiles g, g + G, ...; one sample
//     per lane; psi_b as above with M's four blocks zero-padded in LDS; the four blocks sum_b (w_b / psi_b) l_b r_b^T run on
//     v_mfma_f64_16x16x4_f64 as mps_score_kernel's dA_k does (X[b][a] = (w_b / psi_b) l_b[a] and r_b through LDS, 16 steps of 4
//     samples a tile, block q = 2 s + t selected by zeroing the A operand), accumulated over the workgroup's tiles in registers;
//     the workgroup writes its own partial blocks, sum w log psi^2 and sum w (per tile a butterfly over the 64 lanes, tiles in order).
//   mts_bond_kernel: one workgroup of 256.  The partials are added in workgroup order (the rule of reduce_dev.hpp); |M|^2 is each
//     thread's entries in index order, then block_sum.  After the last step: the unfolding into LDS, mc_rescale, mc_jacobi, the
//     sort, mc_cut, both cores and the bond's outputs.
// No index depends on data except the sort's permutation, masked to 0 .. 31 (LDS arrays of 32).
//
// STATUS: 1 a non-finite core entry or a |M| that is not finite and positive (every output NaN from that bond on; with a
//   non-finite entry on entry, all of them);  2 some psi_b was 0 or not finite (the sample is left out at that bond);  4 a
//   factorisation still rotated in its last allowed sweep;  8 at some bond as formed | |M|^2 - 1 | > 2^-20.  The bits gather in
//   the workspace's header (int 1: the bond kernel's, int 2: the accumulate kernels', every writer storing the same value; int
//   0: the largest sweep count; int 3: the bad flag) and the last bond kernel writes the status word.
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "mps_canon_dev.hpp"
#include "mps_sample_dev.hpp"

namespace bornvi {

namespace {

constexpr int MT_MAX_WG = 256;             // accumulate kernel: workgroups (= partials) at most
constexpr int MT_DMAX = 16;                // the merged 2 D x 2 D matrix must fit mc_jacobi's 64 x 32
constexpr int MT_FORM = 0, MT_STEP = 1, MT_SPLIT = 2;
constexpr int MT_HDR_SWEEPS = 0, MT_HDR_STATUS = 1, MT_HDR_PSI = 2, MT_HDR_BAD = 3;

typedef double mt_d4 __attribute__((ext_vector_type(4)));

struct MtLayout {
  int DP, G;
  long long tiles, Bp;
  size_t hdr, M, blocks, lpart, wpart, vec, total;      // byte offsets from the aligned base
};

MtLayout mt_layout(int n, int D, long long B) {
  MtLayout S;
  S.DP = bond_dp(D);
  S.tiles = (B + MS_LANES - 1) / MS_LANES;
  S.Bp = S.tiles * MS_LANES;
  S.G = (int)(S.tiles < MT_MAX_WG ? S.tiles : MT_MAX_WG);
  size_t o = 0;
  S.hdr = o;    o += 256;
  S.M = o;      o += ws_round((size_t)4 * D * D * sizeof(double));             // the merged tensor [s][t][a][c]
  S.blocks = o; o += ws_round((size_t)S.G * 4 * D * D * sizeof(double));       // one partial per workgroup
  S.lpart = o;  o += ws_round((size_t)MT_MAX_WG * sizeof(double));
  S.wpart = o;  o += ws_round((size_t)MT_MAX_WG * sizeof(double));
  S.vec = o;    o += ws_round((size_t)n * D * (size_t)S.Bp * sizeof(double));  // slot j = 1 .. n
  S.total = o;
  return S;
}

__device__ __forceinline__ size_t mt_slot(int j, int D, long long Bp) { return (size_t)(j - 1) * D * (size_t)Bp; }

// ---- a non-finite core entry; the header ------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void mts_init_kernel(const double* __restrict__ cores, int n, int D, int* __restrict__ hdr) {
  __shared__ double red[MC_THREADS / 64];
  const int t = threadIdx.x;
  const long long total = (long long)n * 2 * D * D;
  const double nan = __builtin_nan("");
  double bad = 0.0;
  for (long long i = t; i < total; i += MC_THREADS) bad = max_nan(bad, isfinite(cores[i]) ? 0.0 : nan);
  bad = block_max_nan<MC_THREADS / 64>(bad, red);
  if (t == 0) {
    hdr[MT_HDR_SWEEPS] = 0;
    hdr[MT_HDR_STATUS] = bad != bad ? 1 : 0;
    hdr[MT_HDR_PSI] = 0;
    hdr[MT_HDR_BAD] = bad != bad ? 1 : 0;
  }
}

// ---- r_n .. r_3 -------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(MS_LANES) void mts_right_kernel(const double* __restrict__ cores, int n, int D, long long B, long long Bp,
                                                             const long long* __restrict__ idx, double* __restrict__ vec) {
  __shared__ double As[2 * DP * DP];
  __shared__ double Rn[DP * MS_LANES];       // the new vector, [a][lane]: the row loop is not unrolled (unrolled in a site loop, the
                                             // compiler puts all of A_k in flight and spills at DP = 16), so its index is a run-time one
  const int lane = threadIdx.x;
  const long long b = (long long)blockIdx.x * MS_LANES + lane;
  const bool active = b < B;
  const unsigned long long z = active ? (unsigned long long)idx[b] : 0ull;
  double r[DP];
  ms_fill<DP>(r, 1.0);
#pragma unroll 1
  for (int k = n; k >= 3; --k) {
    __syncthreads();
    ms_load_site<DP>(cores, k, D, As, nullptr, nullptr);
    __syncthreads();
    const double* A = As + ms_bit(z, n, k) * DP * DP;
    double* dst = vec + mt_slot(k, D, Bp) + b;
#pragma unroll 1
    for (int a = 0; a < DP; ++a, dst += Bp) {
      const double v = ms_dot_col<DP>(A, a, r, 0.0);
      Rn[a * MS_LANES + lane] = v;           // read back by the lane that wrote it
      if (active && a < D) *dst = v;
    }
#pragma unroll
    for (int a = 0; a < DP; ++a) r[a] = Rn[a * MS_LANES + lane];
  }
}

// ---- the samples' vectors through the new core ------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(MS_LANES) void mts_advance_kernel(const double* __restrict__ cores, int n, int D, int k, int dir,
                                                               long long B, long long Bp, const long long* __restrict__ idx,
                                                               double* vec) {
  __shared__ double As[2 * DP * DP];
  const long long b = (long long)blockIdx.x * MS_LANES + threadIdx.x;
  const bool active = b < B;
  const unsigned long long z = active ? (unsigned long long)idx[b] : 0ull;
  const int site = dir > 0 ? k : k + 1;
  ms_load_site<DP>(cores, site, D, As, nullptr, nullptr);
  __syncthreads();
  const double* A = As + ms_bit(z, n, site) * DP * DP;
  const int src = dir > 0 ? k - 1 : k + 2, dstj = dir > 0 ? k : k + 1;
  double v[DP], vn[DP];
  ms_fill<DP>(v, 1.0);
  if (src >= 1 && src <= n) {
    const double* p = vec + mt_slot(src, D, Bp) + b;
#pragma unroll
    for (int a = 0; a < DP; ++a) v[a] = (active && a < D) ? p[(size_t)a * Bp] : 0.0;
  }
#pragma unroll
  for (int a = 0; a < DP; ++a) vn[a] = dir > 0 ? ms_row_dot<DP>(v, A, a, 0.0) : ms_dot_col<DP>(A, a, v, 0.0);
  double* dst = vec + mt_slot(dstj, D, Bp) + b;
#pragma unroll
  for (int a = 0; a < DP; ++a)
    if (active && a < D) dst[(size_t)a * Bp] = vn[a];
}

// ---- psi_b, the loss terms and the four blocks sum_b (w_b / psi_b) l_b r_b^T -------------------------------------
template <int DP>
__global__ __launch_bounds__(MS_LANES) void mts_accum_kernel(int n, int D, int k, long long B, long long Bp, long long ntiles,
                                                             const long long* __restrict__ idx, const double* __restrict__ wgt,
                                                             const double* __restrict__ Mws, const double* __restrict__ vec,
                                                             double* __restrict__ blocks, double* __restrict__ lpart,
                                                             double* __restrict__ wpart, int* hdr) {
  constexpr int XP = 17;                     // row pitch of X and R in LDS (odd: the lanes' rows start in different banks)
  __shared__ double Ms[4 * DP * DP];
  __shared__ double Xs[MS_LANES * XP];
  __shared__ double Rs[MS_LANES * XP];
  __shared__ int Qs[MS_LANES];
  if (hdr[MT_HDR_BAD]) return;               // the same word in every lane of the launch: the bond kernels before it wrote it
  const int lane = threadIdx.x, fr = lane & 15, fk = lane >> 4, DD = D * D;
  for (int i = lane; i < 4 * DP * DP; i += MS_LANES) {
    const int q = i / (DP * DP), a = (i / DP) % DP, c = i % DP;
    Ms[i] = (a < D && c < D) ? Mws[q * DD + a * D + c] : 0.0;
  }
  const double w_each = 1.0 / (double)B;
  const bool has_l = k >= 2, has_r = k + 2 <= n;
  const double* lsrc = vec + (has_l ? mt_slot(k - 1, D, Bp) : 0);
  const double* rsrc = vec + (has_r ? mt_slot(k + 2, D, Bp) : 0);
  mt_d4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = (mt_d4){0.0, 0.0, 0.0, 0.0};
  double lacc = 0.0, wacc = 0.0;
#pragma unroll 1
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long b = tile * MS_LANES + lane;
    const bool active = b < B;
    const unsigned long long z = active ? (unsigned long long)idx[b] : 0ull;
    const int q = 2 * ms_bit(z, n, k) + ms_bit(z, n, k + 1);
    const double wv = active ? (wgt ? wgt[b] : w_each) : 0.0;
    double l[DP], r[DP];
    ms_fill<DP>(l, active ? 1.0 : 0.0);
    ms_fill<DP>(r, 1.0);
    if (has_l) {
#pragma unroll
      for (int a = 0; a < DP; ++a) l[a] = (active && a < D) ? lsrc[(size_t)a * Bp + b] : 0.0;
    }
    if (has_r) {
#pragma unroll
      for (int c = 0; c < DP; ++c) r[c] = (active && c < D) ? rsrc[(size_t)c * Bp + b] : 0.0;
    }
    __syncthreads();                         // Ms is loaded; the tile before is done with Xs, Rs, Qs
    const double* Mq = Ms + q * DP * DP;
    double psi = 0.0;
#pragma unroll
    for (int a = 0; a < DP; ++a)
#pragma unroll
      for (int c = 0; c < DP; ++c) psi = fma(l[a] * r[c], Mq[a * DP + c], psi);
    const bool good = active && psi != 0.0 && isfinite(psi);
    if (active && !good) hdr[MT_HDR_PSI] = 2;
    const double g = good ? wv / psi : 0.0;
    const double lt = good ? wv * (2.0 * log(fabs(psi))) : 0.0;
    lacc += wave_sum(lt);
    wacc += wave_sum(good ? wv : 0.0);
#pragma unroll
    for (int a = 0; a < DP; ++a) {
      Xs[lane * XP + a] = g * l[a];
      Rs[lane * XP + a] = r[a];
    }
    Qs[lane] = q;
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < MS_LANES / 4; ++kk) {
      const int bb = 4 * kk + fk;
      const int qb = Qs[bb];
      const double av = fr < DP ? Xs[bb * XP + fr] : 0.0;
      const double bv = fr < DP ? Rs[bb * XP + fr] : 0.0;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) acc[qq] = __builtin_amdgcn_mfma_f64_16x16x4f64(qb == qq ? av : 0.0, bv, acc[qq], 0, 0, 0);
    }
  }
  // D[row = fk + 4 i][col = fr]: entry (a = fk + 4 i, c = fr) of block q
  double* part = blocks + (size_t)blockIdx.x * 4 * DD;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ar = fk + 4 * i, bc = fr;
      if (ar < D && bc < D) part[(q * D + ar) * D + bc] = acc[q][i];
    }
  if (lane == 0) {
    lpart[blockIdx.x] = lacc;
    wpart[blockIdx.x] = wacc;
  }
}

// ---- the merged tensor: formed, stepped, split --------------------------------------------------------------------
// M[s, t] = A_k[s] A_{k+1}[t] into Ms (LDS, pitch D) and Mws; As: 4 D D doubles of LDS.  Returns |M|^2 (block_sum: barriers inside).
__device__ __forceinline__ double mt_form(const double* cores, int k, int D, double* As, double* Ms, double* Mws, double* red) {
  const int t = threadIdx.x, DD = D * D;
  __syncthreads();
  for (int i = t; i < 4 * DD; i += MC_THREADS) As[i] = cores[(long long)(k - 1) * 2 * DD + i];      // sites k and k + 1 are neighbours
  __syncthreads();
  double part = 0.0;
  for (int i = t; i < 4 * DD; i += MC_THREADS) {
    const int s = i / (2 * DD), tt = (i / DD) & 1, a = (i % DD) / D, c = i % D;
    double acc = 0.0;
    for (int e = 0; e < D; ++e) acc = fma(As[s * DD + a * D + e], As[(2 + tt) * DD + e * D + c], acc);
    Ms[i] = acc;
    Mws[i] = acc;
    part = fma(acc, acc, part);
  }
  return block_sum<MC_THREADS / 64>(part, red);
}

// the header after a bond was formed: the bad flag, bits 1 and 8 (thread 0)
__device__ __forceinline__ void mt_formed_status(double nrm2, int* hdr) {
  if (threadIdx.x != 0) return;
  if (!(nrm2 > 0.0 && isfinite(nrm2))) {
    hdr[MT_HDR_BAD] = 1;
    hdr[MT_HDR_STATUS] |= 1;
  } else if (fabs(nrm2 - 1.0) > 0x1p-20) {
    hdr[MT_HDR_STATUS] |= 8;
  }
}

__global__ __launch_bounds__(MC_THREADS) void mts_bond_kernel(double* cores, int n, int D, int k, int mode, int dir, int G, double lr,
                                                             int Dk, double cutoff, int j, int knext, int last,
                                                             const double* __restrict__ blocks, const double* __restrict__ lpart,
                                                             const double* __restrict__ wpart, double* Mws, double* __restrict__ loss,
                                                             double* __restrict__ schmidt, double* __restrict__ discarded,
                                                             int* __restrict__ rank, int* __restrict__ status, int* hdr) {
  __shared__ double Gm[MS_DMAX * MC_ROWS];         // 16 KB: the unfolded matrix under factorisation
  __shared__ double V[MS_DMAX * MS_DMAX];          //  8 KB: the rotations
  __shared__ double Ms[4 * MT_DMAX * MT_DMAX];     //  8 KB: the merged tensor, pitch D
  __shared__ double As[4 * MT_DMAX * MT_DMAX];     //  8 KB: the two sites' matrices, pitch D
  __shared__ double sigma[MS_DMAX], cn2[MS_DMAX], sorted[MS_DMAX];
  __shared__ double red[MC_THREADS / 64];
  __shared__ int perm[MS_DMAX];
  __shared__ int flag;
  const int t = threadIdx.x, DD = D * D, N2 = 2 * D;
  const double nan = __builtin_nan("");
  const bool bad = hdr[MT_HDR_BAD] != 0;           // written by an earlier launch: the same word in every lane

  if (mode == MT_FORM) {
    if (bad) return;
    mt_formed_status(mt_form(cores, k, D, As, Ms, Mws, red), hdr);
    return;
  }

  if (mode == MT_STEP) {
    if (bad) return;
    const double W = sum_partials<MC_THREADS>(wpart, G, red);
    double m[4], gs[4], part = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = t + MC_THREADS * u;
      m[u] = gs[u] = 0.0;
      if (i < 4 * DD) {
        m[u] = Mws[i];
        double sum = 0.0;
#pragma unroll 16                                // sixteen loads in flight; the additions keep the workgroups' order
        for (int g = 0; g < G; ++g) sum += blocks[(size_t)g * 4 * DD + i];
        gs[u] = sum;
        part = fma(m[u], m[u], part);
      }
    }
    const double nrm2 = block_sum<MC_THREADS / 64>(part, red);
    part = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double gr = 2.0 * (W * m[u] / nrm2 - gs[u]);
      m[u] = m[u] - lr * gr;
      part = fma(m[u], m[u], part);          // the entries past 4 D D are 0
    }
    const double nn = block_sum<MC_THREADS / 64>(part, red);
    const double nrm = sqrt(nn);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = t + MC_THREADS * u;
      if (i < 4 * DD) Mws[i] = m[u] / nrm;
    }
    if (t == 0 && !(nn > 0.0 && isfinite(nn))) {
      hdr[MT_HDR_BAD] = 1;
      hdr[MT_HDR_STATUS] |= 1;
    }
    return;
  }

  // ---- MT_SPLIT ----
  double* Ak = cores + (long long)(k - 1) * 2 * DD;      // A_k, then A_{k+1}
  if (bad) {
    for (int i = t; i < 4 * DD; i += MC_THREADS) Ak[i] = nan;
    if (dir < 0)
      for (int i = t; i < D; i += MC_THREADS) schmidt[(long long)(k - 1) * D + i] = nan;
    if (t == 0) {
      loss[j] = nan;
      if (dir < 0) {
        discarded[k - 1] = nan;
        rank[k - 1] = 0;
      }
      if (last) *status = hdr[MT_HDR_STATUS] | hdr[MT_HDR_PSI] | 1;
    }
    return;
  }
  const double Lsum = sum_partials<MC_THREADS>(lpart, G, red);
  const double W = sum_partials<MC_THREADS>(wpart, G, red);
  double part = 0.0;
  for (int i = t; i < 4 * DD; i += MC_THREADS) {
    const double v = Mws[i];
    Ms[i] = v;
    part = fma(v, v, part);
  }
  const double nrm2 = block_sum<MC_THREADS / 64>(part, red);      // its barriers publish Ms
  if (t == 0) loss[j] = W * log(nrm2) - Lsum;
  for (int i = t; i < 4 * DD; i += MC_THREADS) {                   // rows (s, a), columns (t, c)
    const int s = i / (2 * DD), tt = (i / DD) & 1, a = (i % DD) / D, c = i % D;
    Gm[(tt * D + c) * MC_ROWS + s * D + a] = Ms[i];
  }
  __syncthreads();
  mc_rescale(N2, N2, Gm, red);
  const int sw = mc_jacobi(N2, N2, Gm, V, sigma, cn2, &flag);
  // descending, ties by index: the place of a value is the count of those in front of it
  if (t < N2) perm[t] = t;
  __syncthreads();
  if (t < N2) {
    const double mine = sigma[t];
    int pos = 0;
    for (int c = 0; c < N2; ++c) {
      const double o = sigma[c];
      pos += (o > mine || (o == mine && c < t)) ? 1 : 0;
    }
    perm[pos & (MS_DMAX - 1)] = t;
    sorted[pos & (MS_DMAX - 1)] = mine;
  }
  __syncthreads();
  double total, dropped, ksum;
  const int r = mc_cut(N2, Dk, cutoff, sorted, total, dropped, ksum);
  const double knorm = sqrt(ksum);
  if (dir < 0) {
    if (t < D) schmidt[(long long)(k - 1) * D + t] = t < r ? sorted[t] / knorm : 0.0;
    if (t == 0) {
      discarded[k - 1] = dropped / total;
      rank[k - 1] = r;
    }
  }
  for (int i = t; i < 2 * DD; i += MC_THREADS) {                   // A_k[s][a][j'] = U[(s, a)][p(j')]  (times s_j' going left)
    const int s = i / DD, a = (i % DD) / D, jp = i % D;
    double v = 0.0;
    if (jp < r && !(k == 1 && a > 0)) {
      const int jj = perm[jp] & (MS_DMAX - 1);
      const double sg = sigma[jj];
      if (sg > 0.0) {
        v = Gm[jj * MC_ROWS + s * D + a] / sg;
        if (dir < 0) v = v * (sg / knorm);
      }
    }
    Ak[i] = v;
  }
  for (int i = t; i < 2 * DD; i += MC_THREADS) {                   // A_{k+1}[t][j'][c] = V[(t, c)][p(j')]  (times s_j' going right)
    const int tt = i / DD, jp = (i % DD) / D, c = i % D;
    double v = 0.0;
    if (jp < r && !(k + 1 == n && c > 0)) {
      const int jj = perm[jp] & (MS_DMAX - 1);
      v = V[jj * MS_DMAX + tt * D + c];
      if (dir > 0) v = (sigma[jj] / knorm) * v;
    }
    Ak[2 * DD + i] = v;
  }
  if (t == 0) {
    const int used = sw < 0 ? -sw : sw;
    if (used > hdr[MT_HDR_SWEEPS]) hdr[MT_HDR_SWEEPS] = used;
    if (sw < 0) hdr[MT_HDR_STATUS] |= 4;
  }
  if (knext > 0) {                                                 // the next bond's M from the cores as just written (mt_form begins on a barrier)
    __threadfence_block();
    mt_formed_status(mt_form(cores, knext, D, As, Ms, Mws, red), hdr);
  }
  if (last && t == 0) *status = hdr[MT_HDR_STATUS] | hdr[MT_HDR_PSI];
}

// CALL with `DP` a constant expression equal to DPV (= bond_dp(D) <= 16)
#define MT_DISPATCH(DPV, CALL)                        \
  switch (DPV) {                                      \
    case 2: { constexpr int DP = 2; CALL; } break;    \
    case 4: { constexpr int DP = 4; CALL; } break;    \
    case 8: { constexpr int DP = 8; CALL; } break;    \
    default: { constexpr int DP = 16; CALL; } break;  \
  }

}  // namespace

size_t mps_twosite_workspace_bytes(int n, int D, long long B) { return mt_layout(n, D, B).total + 256; }

hipError_t launch_mps_twosite_sweep(int n, int D, long long B, double* cores, const long long* idx, const double* w, double lr,
                                    int steps, int D_keep, double cutoff, double* loss, double* schmidt, double* discarded, int* rank,
                                    int* status, void* ws, hipStream_t st) {
  const MtLayout S = mt_layout(n, D, B);
  char* base = ws_align(ws);
  int* hdr = (int*)(base + S.hdr);
  double* Mws = (double*)(base + S.M);
  double* blocks = (double*)(base + S.blocks);
  double* lpart = (double*)(base + S.lpart);
  double* wpart = (double*)(base + S.wpart);
  double* vec = (double*)(base + S.vec);
  const unsigned tiles = (unsigned)S.tiles;
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  mts_init_kernel<<<1, MC_THREADS, 0, st>>>(cores, n, D, hdr);
  if (n >= 3) MT_DISPATCH(S.DP, (mts_right_kernel<DP><<<tiles, MS_LANES, 0, st>>>(cores, n, D, B, S.Bp, idx, vec)));
  mts_bond_kernel<<<1, MC_THREADS, 0, st>>>(cores, n, D, 1, MT_FORM, 1, S.G, lr, D_keep, cutoff, 0, 0, 0, blocks, lpart, wpart, Mws, loss,
                                           schmidt, discarded, rank, status, hdr);
  const int bonds = n - 1;
  for (int j = 0; j < 2 * bonds; ++j) {
    const int dir = j < bonds ? 1 : -1;
    const int k = dir > 0 ? j + 1 : 2 * bonds - j;
    const int last = j == 2 * bonds - 1;
    const int knext = last ? 0 : (j == bonds - 1 ? k : k + dir);
    for (int it = 0; it <= steps; ++it) {
      MT_DISPATCH(S.DP, (mts_accum_kernel<DP><<<(unsigned)S.G, MS_LANES, 0, st>>>(n, D, k, B, S.Bp, S.tiles, idx, w, Mws, vec, blocks,
                                                                                lpart, wpart, hdr)));
      mts_bond_kernel<<<1, MC_THREADS, 0, st>>>(cores, n, D, k, it < steps ? MT_STEP : MT_SPLIT, dir, S.G, lr, D_keep, cutoff, j, knext,
                                               last, blocks, lpart, wpart, Mws, loss, schmidt, discarded, rank, status, hdr);
    }
    // the advance: slot k from slot k - 1 going right, slot k + 1 from slot k + 2 going left; not after a pass's last bond
    if (!last && j != bonds - 1)
      MT_DISPATCH(S.DP, (mts_advance_kernel<DP><<<tiles, MS_LANES, 0, st>>>(cores, n, D, k, dir, B, S.Bp, idx, vec)));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

}  // namespace bornvi
