// Sampled matrix-product-state Born machine: nothing here touches 2^n of anything.
//   q(z) = psi(z)^2 / Z,  psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0,  cores [n, 2, D, D] float64, 1 <= n <= 63, 1 <= D <= 32.
//
// bornvi_mps_environments:  E_n = e0 e0^T,  E_{k-1} = sum_s A_k[s] E_k A_k[s]^T,  Z = E_0[0, 0];
//                           L_0 = e0 e0^T,  L_k = sum_s A_k[s]^T L_{k-1} A_k[s].
//   One launch of two workgroups (0: the right environments, 1: the left ones), n dependent steps each.  A step is two
//   D x D x D products through LDS, T_s = A_s X (A_s^T X on the left) and X' = sum_s T_s A_s^T (T_s A_s), every entry one
//   fma chain in index order (c, then s outer / d inner).  After every step the matrix is multiplied by 2^-e, e = ilogb of
//   its largest magnitude (exact), and the running sum of the e's is stored beside it:  true E_k = E^_k 2^eE[k].
//   log Z = log E^_0[0, 0] + eE[0] ln 2.
//
// The lanes' vectors l^, r^, their steps and exponents, the right-to-left sweep, the amplitude test, the site factor and the
// environment term mu are defined in mps_sample_dev.hpp, once, and named here by the helper that computes them.
//
// bornvi_mps_sample: one sample per lane, one wave per workgroup; l^ in registers, A_k[0], A_k[1], E^_k zero-padded in LDS
//   and read as broadcasts.  For k = 1 .. n:
//     u_s = l A_k[s] (ms_row_dot's chain, the two s in one loop),  m_s = u_s E^_k u_s^T = sum_d u_s[d] (sum_c u_s[c] E^_k[c][d]),  z_k = [U_k (m_0 + m_1) >= m_0],
//   then l = u_{z_k} rescaled (ms_rescale), the exponents summed in el.  The common factor 2^eE[k] of both m_s drops out.
//   (The loop is ms_sample_sweep: the clamped sampler of kernels_mps_query.hip runs the same one.)
//   U_k: Philox4x32-10 (philox_dev.hpp), key = (seed & 0xffffffff, seed >> 32),
//     counter = (b, ceil(k / 2) - 1, 0xffffffff, epoch & 0xffffffff) -> w0 .. w3;
//     odd k: U_k = ((w1:w0) >> 11) 2^-53,  even k: U_k = ((w3:w2) >> 11) 2^-53   (the call of k - 1).
//   (0xffffffff is no circuit id of the shots path: those are 0 .. 2 P + 2 for P circuit parameters.)  A draw depends on
//   (seed, epoch, b, k) and on the sample's own earlier bits only: not on B, the grid or the tiling.
//   If m_0 + m_1 is 0 or not finite the status word becomes 1, the sample's remaining bits are 0 and its logq is NaN.
//   logq = ms_logq(l^_n[0], el).
//
// bornvi_mps_score_vjp: grad = sum_b w_b grad log q(z_b) = sum_b (2 w_b / psi_b) l_{b,k-1}^T (x) r_{b,k}^T at [k, z_{b,k}]
//                              - (sum_b w_b) mu[k].
//   mps_score_kernel: one wave per workgroup and a tile of 64 samples at a time, one sample per lane; at most MS_MAX_WG
//   workgroups, each walking the tiles wg, wg + G, ...  ms_right_sweep with MsSliceStore: r^_1 .. r^_{n-1} and their exponents
//   go to the workgroup's slice of the workspace; logq = ms_logq(r^_0[0], er_0).  Left to right (ms_left_step):
//   X[b][a] = cf l^_{k-1}[a], cf = ms_site_factor with g = 2 w_b / r^_0[0], goes to LDS and
//   dA_k[s] += X_s^T R_k (X_s: the rows with z_{b,k} = s, others 0) runs on v_mfma_f64_16x16x4_f64, 16 steps of 4 samples,
//   the B operand read straight from the slice ([sample][DS], 16 consecutive doubles of 4 rows per step, the layout of
//   kernels_mps.hip's dA_k); the workgroup adds the tile into its own partial [n, 2, D, D] (first tile: stores).
//   mps_score_finish_kernel, one workgroup per site: the partials in workgroup order, sum_b w_b (per tile a butterfly over the
//   64 lanes, tiles in order, then the workgroups' totals: 64-lane butterflies of lane-strided sums, waves in order) and
//   mu[k] by ms_env_stage and ms_env_entry.
//   A sample that fails ms_amplitude_ok gets logq = -inf (NaN), weight 0 in the first term, and sets the status word to 2.
//
// bornvi_mps_score_rows: the per-sample score rows of the sampled Fisher estimate,
//   o_b[k, s, a, c] = 2 [z_{b,k} = s] l_{b,k-1}[a] r_{b,k}[c] / psi_b - mu[k, s, a, c],
//   rows[k - 1 - k_begin][(s D + a) D + c][b], leading dimension ld (a power of two >= max(B, 64): what the Gram takes).
//   mps_score_mu_kernel, one workgroup per site: mu by ms_env_stage and ms_env_entry into the workspace.
//   mps_score_rows_kernel: one sample per lane, one wave per workgroup, workgroup g walks the 64-column tiles g, g + G, ... of
//   the ld columns; ms_right_sweep with MsSliceStore; left to right (ms_left_step) l^_{k-1} and r^_k of the lane's sample go
//   to LDS ([a][lane]: conflict free) and for the sites k_begin < k <= k_begin + k_count the lane writes its 2 D^2 entries
//     (cf l^[a]) r^[c] - mu  (z = s),   0 - mu  (z != s),   cf = ms_site_factor with g = 2 / r^_0[0],
//   each store contiguous over the 64 lanes.  A sample that fails ms_amplitude_ok gets an all-zero column and status 2;
//   the columns B .. ld - 1 are written as 0.0.  Sites outside the range are swept and not written.
//
// bornvi_mps_score_jvp: the per-sample directional derivative of log q along v [n, 2, D, D],
//   t_b = scale <grad log q(z_b), v> = scale (2 dpsi_b / psi_b - c),   dpsi_b = sum_k l_{b,k-1}^T V_k[z_bk] r_{b,k},   c = sum_k <mu_k, V_k>.
//   mps_score_mu_kernel forms mu into the workspace; mps_jvp_dot_kernel, one workgroup per site, adds the site's 2 D^2
//   products mu V in index order (one fma chain) into wpart[k - 1]; every workgroup of the sweep adds the n partials in site
//   order.  mps_score_jvp_kernel has mps_score_kernel's grid and tiles and one sweep, left to right, of the pair (l, dl):
//     dl <- dl A_k[z] + l V_k[z]  (one fma chain per entry: the D terms of dl A, then the D terms of l V),   l <- l A_k[z],
//   ms_row_dot's chain written out so that l A and dl A share one loop and each A entry is read once for both,
//   A_k[.] and V_k[.] zero-padded in LDS, each lane reading the matrices of its own z (at most two addresses per read); after
//   every site l is rescaled (ms_rescale) and dl *= 2^-e with the same e, so 2 dl_n[0] / l_n[0] carries no exponent.
//   No right vector, no slice of the workspace.  t_b depends on (cores, v, scale, z_b) only.  A sample that fails
//   ms_amplitude_ok (on l^_n[0]) gets t_b = 0.0 and sets the status word to 2.
//
// bornvi_bn_logjoint_samples: logp_b = sum_v log max(CPT_v[parents][value], p_floor), one lane per sample, nodes in order.
// bornvi_bn_sample: exact ancestral draws from the network itself, stated above bn_sample_kernel.
//
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.  The status word is cleared
// by a one-lane kernel in front of the launch (a kernel node like the others when the calls are captured into a graph, so
// every replay clears it in stream order) and set by plain stores (every writer of a launch stores the same value).
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "mps_sample_dev.hpp"
#include "philox_dev.hpp"

namespace bornvi {

namespace {
constexpr int MS_MAX_WG = 256;             // score kernel: workgroups (= workspace slices and partials) at most

typedef double ms_d4 __attribute__((ext_vector_type(4)));

struct MsLayout {
  int DP, DS, G;
  size_t hdr, E, L, eE, eL, r, er, parts, wpart, mu, total;   // byte offsets from the aligned base
};

MsLayout ms_layout(int n, int D, long long B) {
  MsLayout S;
  S.DP = bond_dp(D);
  S.DS = (D + 1) & ~1;
  const long long tiles = (B + MS_LANES - 1) / MS_LANES;
  S.G = (int)(tiles < MS_MAX_WG ? tiles : MS_MAX_WG);
  size_t o = 0;
  S.hdr = o;   o += 256;                                                     // log Z, E^_0[0, 0], eE[0]
  S.E = o;     o += ws_round((size_t)(n + 1) * D * D * sizeof(double));
  S.L = o;     o += ws_round((size_t)(n + 1) * D * D * sizeof(double));
  S.eE = o;    o += ws_round((size_t)(n + 1) * sizeof(int));
  S.eL = o;    o += ws_round((size_t)(n + 1) * sizeof(int));
  S.r = o;     o += ws_round((size_t)S.G * n * MS_LANES * S.DS * sizeof(double));   // slot k of a slice: r^_k, k = 1 .. n - 1
  S.er = o;    o += ws_round((size_t)S.G * n * MS_LANES * sizeof(int));
  S.parts = o; o += ws_round((size_t)S.G * n * 2 * D * D * sizeof(double));
  S.wpart = o; o += ws_round((size_t)MS_MAX_WG * sizeof(double));
  S.mu = o;    o += ws_round((size_t)n * 2 * D * D * sizeof(double));               // score rows: the exact mean mu[k, s, a, c]
  S.total = o;
  return S;
}

// ---- environments ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_ENV_THREADS) void mps_env_kernel(const double* __restrict__ cores, int n, int D, double* __restrict__ E,
                                                              double* __restrict__ L, int* __restrict__ eE, int* __restrict__ eL,
                                                              double* __restrict__ hdr, double* __restrict__ logZ_out) {
  __shared__ double As[2 * MS_DMAX * MS_DMAX];
  __shared__ double X[MS_DMAX * MS_DMAX];
  __shared__ double T[2 * MS_DMAX * MS_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  const bool right = blockIdx.x == 0;
  double* out = right ? E : L;
  int* eo = right ? eE : eL;
  const int DD = D * D, t = threadIdx.x;
  for (int i = t; i < DD; i += MS_ENV_THREADS) {
    X[i] = i == 0 ? 1.0 : 0.0;
    out[(long long)(right ? n : 0) * DD + i] = X[i];
  }
  if (t == 0) eo[right ? n : 0] = 0;
  int ex = 0;
  for (int step = 0; step < n; ++step) {            // its own text, not ms_env_sweep: the direction is a run-time value (profiles/mps_env_core_isa.txt)
    const int k = right ? n - step : step + 1;       // the site whose matrices this step uses
    const int dst = right ? k - 1 : k;
    __syncthreads();
    for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) As[i] = cores[(long long)(k - 1) * 2 * DD + i];
    __syncthreads();
    ex += ms_env_step<true>(right, D, 3, As, X, T, red, out + (long long)dst * DD);
    if (t == 0) eo[dst] = ex;
  }
  __syncthreads();
  if (right && t == 0) {
    const double Zh = X[0];
    const double lz = log(Zh) + (double)ex * MS_LN2;
    hdr[0] = lz;
    hdr[1] = Zh;
    hdr[2] = (double)ex;
    if (logZ_out) logZ_out[0] = lz;
  }
}

// ---- status word -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ms_clear_status_kernel(int* status) {
  if (threadIdx.x == 0) *status = 0;
}

// ---- sampler ---------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(MS_LANES) void mps_sample_kernel(const double* __restrict__ cores, int n, int D, long long B,
                                                              const double* __restrict__ E, const double* __restrict__ hdr,
                                                              uint32_t seed_lo, uint32_t seed_hi,
                                                              const long long* __restrict__ epoch_dev, long long* __restrict__ idx,
                                                              double* __restrict__ logq, int* status) {
  __shared__ double As[2 * DP * DP];
  __shared__ double Es[DP * DP];
  const long long b = (long long)blockIdx.x * MS_LANES + threadIdx.x;
  const bool active = b < B;
  const uint32_t ep = (uint32_t)(unsigned long long)(*epoch_dev);
  double l[DP];
  int el;
  unsigned long long z;
  bool dead;
  ms_sample_sweep<DP, false>(cores, n, D, b, active, E, seed_lo, seed_hi, ep, 0ull, 0ull, As, Es, z, l, el, dead, status);
  if (active) {
    idx[b] = (long long)z;
    logq[b] = dead ? __builtin_nan("") : ms_logq(l[0], el, hdr[1], hdr[2]);
  }
}

// ---- score gradient --------------------------------------------------------------------------------------------
// ms_right_sweep's store of the score and rows kernels: r^_k and er_k into slot k of the workgroup's slice, k = 1 .. n - 1
template <int DP>
struct MsSliceStore {
  double* rsl;
  int* esl;
  int n, DS, lane;
  __device__ __forceinline__ void operator()(int k, const double (&r)[DP], int er) const {
    if (k >= n) return;
    double* dst = rsl + ((size_t)k * MS_LANES + lane) * DS;
#pragma unroll
    for (int a = 0; a < DP; ++a)
      if (a < DS) dst[a] = r[a];
    esl[k * MS_LANES + lane] = er;
  }
};

template <int DP>
__global__ __launch_bounds__(MS_LANES) void mps_score_kernel(const double* __restrict__ cores, int n, int D, int DS, long long B,
                                                             long long ntiles, const long long* __restrict__ idx,
                                                             const double* __restrict__ wgt, const double* __restrict__ hdr,
                                                             double* __restrict__ logq, int* status, double* rws, int* erws,
                                                             double* parts, double* __restrict__ wpart) {
  constexpr int NT = DP > 16 ? 2 : 1;
  constexpr int XP = 16 * NT + 1;            // row pitch of X in LDS (odd: the lanes' rows start in different banks)
  __shared__ double As[2 * DP * DP];
  __shared__ double Xs[MS_LANES * XP];
  __shared__ int Zs[MS_LANES];
  const int lane = threadIdx.x, fr = lane & 15, fk = lane >> 4;
  double* rsl = rws + (size_t)blockIdx.x * n * MS_LANES * DS;
  int* esl = erws + (size_t)blockIdx.x * n * MS_LANES;
  double* part = parts + (size_t)blockIdx.x * n * 2 * D * D;
  const double Zh = hdr[1], eE0 = hdr[2];
  const bool Zok = ms_norm_ok(Zh);
  double wacc = 0.0;
  bool first = true;
#pragma unroll 1
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x, first = false) {
    const long long b = tile * MS_LANES + lane;
    const bool active = b < B;
    const unsigned long long z = active ? (unsigned long long)idx[b] : 0ull;
    const double wv = active ? wgt[b] : 0.0;
    wacc += wave_sum(wv);
    // right to left: r^_1 .. r^_{n-1} and their exponents into the slice
    double r[DP];
    const int er0 = ms_right_sweep<DP>(cores, n, D, z, As, r, MsSliceStore<DP>{rsl, esl, n, DS, lane});
    const double r0 = r[0];
    const bool good = ms_amplitude_ok(r0, Zok);
    if (active) {
      logq[b] = ms_logq(r0, er0, Zh, eE0);
      if (!good) *status = 2;
    }
    const double g = good ? (wv + wv) / r0 : 0.0;
    // left to right
    double l[DP];
    ms_fill<DP>(l, 1.0);
    int el = 0;
#pragma unroll 1
    for (int k = 1; k <= n; ++k) {
      __syncthreads();
      ms_load_site<DP>(cores, k, D, As, nullptr, nullptr);
      const int s = ms_bit(z, n, k);
      const int erk = k < n ? esl[k * MS_LANES + lane] : 0;
      const double cf = ms_site_factor(g, el, erk, er0);
#pragma unroll
      for (int a = 0; a < DP; ++a) Xs[lane * XP + a] = cf * l[a];
      Zs[lane] = s;
      __syncthreads();
      ms_d4 acc[2][NT][NT];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
          for (int tb = 0; tb < NT; ++tb) acc[q][ta][tb] = (ms_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
      for (int kk = 0; kk < MS_LANES / 4; ++kk) {
        const int bb = 4 * kk + fk;
        const int sb = Zs[bb];
        double av[NT], bv[NT];
#pragma unroll
        for (int ta = 0; ta < NT; ++ta) {
          const int col = ta * 16 + fr;
          av[ta] = col < D ? Xs[bb * XP + col] : 0.0;
        }
#pragma unroll
        for (int tb = 0; tb < NT; ++tb) {
          const int col = tb * 16 + fr;
          if (k < n) bv[tb] = col < D ? rsl[((size_t)k * MS_LANES + bb) * DS + col] : 0.0;
          else bv[tb] = col == 0 ? 1.0 : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int ta = 0; ta < NT; ++ta)
#pragma unroll
            for (int tb = 0; tb < NT; ++tb)
              acc[q][ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(sb == q ? av[ta] : 0.0, bv[tb], acc[q][ta][tb], 0, 0, 0);
      }
      // D[row = fk + 4 i][col = fr] of tile (ta, tb): entry (a = 16 ta + fk + 4 i, b = 16 tb + fr)
      double* pk = part + (size_t)(k - 1) * 2 * D * D;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
          for (int tb = 0; tb < NT; ++tb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int ar = ta * 16 + fk + 4 * i, bc = tb * 16 + fr;
              if (ar < D && bc < D) {
                double* p = pk + (q * D + ar) * D + bc;
                *p = first ? acc[q][ta][tb][i] : *p + acc[q][ta][tb][i];
              }
            }
      el += ms_left_step<DP>(l, As + s * DP * DP);
    }
  }
  if (lane == 0) wpart[blockIdx.x] = wacc;
}

// grid n: grad[k - 1] = the workgroups' partials in order - (sum_b w_b) mu[k - 1] (ms_env_stage, ms_env_entry)
__global__ __launch_bounds__(MS_ENV_THREADS) void mps_score_finish_kernel(const double* __restrict__ cores, int n, int D, int G,
                                                                       const double* __restrict__ parts,
                                                                       const double* __restrict__ wpart, const double* __restrict__ E,
                                                                       const double* __restrict__ L, const int* __restrict__ eE,
                                                                       const int* __restrict__ eL, const double* __restrict__ hdr,
                                                                       double* __restrict__ grad) {
  __shared__ double As[2 * MS_DMAX * MS_DMAX];
  __shared__ double Em[MS_DMAX * MS_DMAX];
  __shared__ double Lm[MS_DMAX * MS_DMAX];
  __shared__ double T[2 * MS_DMAX * MS_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  const int k = blockIdx.x + 1, t = threadIdx.x, DD = D * D;
  double wv = 0.0;
  for (int i = t; i < G; i += MS_ENV_THREADS) wv += wpart[i];
  wv = wave_sum(wv);
  if ((t & 63) == 0) red[t >> 6] = wv;
  ms_env_stage(cores, k, D, E, L, As, Em, Lm, T);      // its barriers publish red too
  const double W = ((red[0] + red[1]) + red[2]) + red[3];
  const int ex = eL[k - 1] + eE[k] - eE[0];
  const double Zh = hdr[1];
  const size_t stride = (size_t)n * 2 * DD;
  for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {
    double sum = 0.0;
    const double* p = parts + (size_t)(k - 1) * 2 * DD + i;
    for (int g = 0; g < G; ++g) sum += p[g * stride];
    grad[(size_t)(k - 1) * 2 * DD + i] = sum - W * ms_env_entry(Lm, T, D, i, Zh, ex);
  }
}

// ---- score rows (sampled Fisher estimate) ----------------------------------------------------------------------
// grid n: mu[k - 1] = the environment term (ms_env_stage, ms_env_entry)
__global__ __launch_bounds__(MS_ENV_THREADS) void mps_score_mu_kernel(const double* __restrict__ cores, int D, const double* __restrict__ E,
                                                                   const double* __restrict__ L, const int* __restrict__ eE,
                                                                   const int* __restrict__ eL, const double* __restrict__ hdr,
                                                                   double* __restrict__ mu) {
  __shared__ double As[2 * MS_DMAX * MS_DMAX];
  __shared__ double Em[MS_DMAX * MS_DMAX];
  __shared__ double Lm[MS_DMAX * MS_DMAX];
  __shared__ double T[2 * MS_DMAX * MS_DMAX];
  const int k = blockIdx.x + 1, t = threadIdx.x, DD = D * D;
  ms_env_stage(cores, k, D, E, L, As, Em, Lm, T);
  const int ex = eL[k - 1] + eE[k] - eE[0];
  const double Zh = hdr[1];
  for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) mu[(size_t)(k - 1) * 2 * DD + i] = ms_env_entry(Lm, T, D, i, Zh, ex);
}

template <int DP>
__global__ __launch_bounds__(MS_LANES) void mps_score_rows_kernel(const double* __restrict__ cores, int n, int D, int DS, long long B,
                                                                  long long ntiles, const long long* __restrict__ idx,
                                                                  const double* __restrict__ hdr, const double* __restrict__ mu,
                                                                  int k_begin, int k_count, long long ld, double* __restrict__ rows,
                                                                  int* status, double* rws, int* erws) {
  __shared__ double As[2 * DP * DP];
  __shared__ double Mu[2 * DP * DP];         // mu[k] as stored: [s][a][c] with pitch D
  __shared__ double Ls[DP * MS_LANES];       // l^_{k-1}[a] of the lane's sample at [a][lane]
  __shared__ double Rs[DP * MS_LANES];       // r^_k[c]
  const int lane = threadIdx.x, DD = D * D, R = 2 * DD;
  double* rsl = rws + (size_t)blockIdx.x * n * MS_LANES * DS;
  int* esl = erws + (size_t)blockIdx.x * n * MS_LANES;
  const bool Zok = ms_norm_ok(hdr[1]);
#pragma unroll 1
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long b = tile * MS_LANES + lane;            // b < ld: the tiles cover the ld columns exactly
    if (tile * MS_LANES >= B) {                            // (uniform) a tile of padding columns
      for (int kk = 0; kk < k_count; ++kk)
        for (int j = 0; j < R; ++j) rows[((size_t)kk * R + j) * ld + b] = 0.0;
      continue;
    }
    const bool active = b < B;
    const unsigned long long z = active ? (unsigned long long)idx[b] : 0ull;
    // right to left: r^_1 .. r^_{n-1} and their exponents into the slice
    double r[DP];
    const int er0 = ms_right_sweep<DP>(cores, n, D, z, As, r, MsSliceStore<DP>{rsl, esl, n, DS, lane});
    const double r0 = r[0];
    const bool good = active && ms_amplitude_ok(r0, Zok);
    if (active && !good) *status = 2;
    const double g = good ? 2.0 / r0 : 0.0;
    // left to right
    double l[DP];
    ms_fill<DP>(l, 1.0);
    int el = 0;
#pragma unroll 1
    for (int k = 1; k <= n; ++k) {
      const bool wanted = k - 1 >= k_begin && k - 1 < k_begin + k_count;
      __syncthreads();
      ms_load_site<DP>(cores, k, D, As, nullptr, nullptr);
      const int s = ms_bit(z, n, k);
      if (wanted) {
        for (int i = lane; i < R; i += MS_LANES) Mu[i] = mu[(size_t)(k - 1) * R + i];
        const int erk = k < n ? esl[k * MS_LANES + lane] : 0;
        const double cf = ms_site_factor(g, el, erk, er0);
        const double* src = rsl + ((size_t)k * MS_LANES + lane) * DS;
#pragma unroll
        for (int a = 0; a < DP; ++a) {
          Ls[a * MS_LANES + lane] = cf * l[a];
          if (a < D) Rs[a * MS_LANES + lane] = k < n ? src[a] : (a == 0 ? 1.0 : 0.0);
        }
      }
      __syncthreads();
      if (wanted) {
        double* out = rows + (size_t)(k - 1 - k_begin) * R * ld + b;
        for (int q = 0; q < 2; ++q) {
          const bool on = good && q == s;
          for (int a = 0; a < D; ++a) {
            const double cl = Ls[a * MS_LANES + lane];
            for (int c = 0; c < D; ++c) {
              const double t = on ? cl * Rs[c * MS_LANES + lane] : 0.0;
              out[(size_t)((q * D + a) * D + c) * ld] = good ? t - Mu[(q * D + a) * D + c] : 0.0;
            }
          }
        }
      }
      el += ms_left_step<DP>(l, As + s * DP * DP);
    }
  }
}

// ---- score jvp (matrix-free natural gradient) --------------------------------------------------------------------
// grid n: cpart[k - 1] = sum_i mu[k - 1][i] v[k - 1][i], i = (s D + a) D + c in order: one fma chain of 2 D^2 terms
__global__ __launch_bounds__(MS_ENV_THREADS) void mps_jvp_dot_kernel(const double* __restrict__ mu, const double* __restrict__ v, int D,
                                                                  double* __restrict__ cpart) {
  __shared__ double Ms[2 * MS_DMAX * MS_DMAX];
  __shared__ double Vs[2 * MS_DMAX * MS_DMAX];
  const int R = 2 * D * D, t = threadIdx.x;
  const size_t off = (size_t)blockIdx.x * R;
  for (int i = t; i < R; i += MS_ENV_THREADS) {
    Ms[i] = mu[off + i];
    Vs[i] = v[off + i];
  }
  __syncthreads();
  if (t == 0) {
    double acc = 0.0;
    for (int i = 0; i < R; ++i) acc = fma(Ms[i], Vs[i], acc);
    cpart[blockIdx.x] = acc;
  }
}

template <int DP>
__global__ __launch_bounds__(MS_LANES) void mps_score_jvp_kernel(const double* __restrict__ cores, const double* __restrict__ vdir,
                                                                 int n, int D, long long B, long long ntiles,
                                                                 const long long* __restrict__ idx, const double* __restrict__ hdr,
                                                                 const double* __restrict__ cpart, double scale,
                                                                 double* __restrict__ tout, int* status) {
  __shared__ double As[2 * DP * DP];
  __shared__ double Vs[2 * DP * DP];
  const int lane = threadIdx.x;
  const bool Zok = ms_norm_ok(hdr[1]);
  double cdot = 0.0;                                       // (uniform) the sites in order
  for (int k = 0; k < n; ++k) cdot += cpart[k];
#pragma unroll 1
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long b = tile * MS_LANES + lane;
    const bool active = b < B;
    const unsigned long long z = active ? (unsigned long long)idx[b] : 0ull;
    double l[DP], dl[DP];
    ms_fill<DP>(l, 1.0);
    ms_fill<DP>(dl, 0.0);
#pragma unroll 1
    for (int k = 1; k <= n; ++k) {
      __syncthreads();
      ms_load_site<DP>(cores, k, D, As, nullptr, nullptr);
      ms_load_site<DP>(vdir, k, D, Vs, nullptr, nullptr);
      __syncthreads();
      const int s = ms_bit(z, n, k);
      const double* Az = As + s * DP * DP;
      const double* Vz = Vs + s * DP * DP;
      double ln[DP], dn[DP];           // ms_row_dot's chains, l A and dl A in one loop: see mps_sample_dev.hpp
#pragma unroll
      for (int c = 0; c < DP; ++c) {
        double a0 = 0.0, d0 = 0.0;
#pragma unroll
        for (int a = 0; a < DP; ++a) {
          const double av = Az[a * DP + c];
          a0 = fma(l[a], av, a0);
          d0 = fma(dl[a], av, d0);
        }
#pragma unroll
        for (int a = 0; a < DP; ++a) d0 = fma(l[a], Vz[a * DP + c], d0);
        ln[c] = a0;
        dn[c] = d0;
      }
#pragma unroll
      for (int a = 0; a < DP; ++a) l[a] = ln[a];           // ms_take's two lines: through the call the DP = 16 kernel waits
      const int e = ms_rescale<DP>(l);                     // on its LDS reads more often and is a quarter slower
#pragma unroll
      for (int a = 0; a < DP; ++a) dl[a] = ldexp(dn[a], -e);
    }
    const double p0 = l[0];
    const bool good = ms_amplitude_ok(p0, Zok);
    if (active) {
      tout[b] = good ? scale * ((dl[0] + dl[0]) / p0 - cdot) : 0.0;
      if (!good) *status = 2;
    }
  }
}

// ---- log joint of samples --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_logjoint_kernel(bornvi_bn_desc bn, int n, long long B, const long long* __restrict__ idx,
                                                          double p_floor, double* __restrict__ logp) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long z = (unsigned long long)idx[b];
  unsigned long long vals = 0;   // bit v = value of node v
  bool bad = false;
  for (int v = 0; v < bn.num_nodes; ++v) {
    const int role = bn.role[v];
    unsigned long long bit = 0ull;
    if (role >= 0 && role < n) bit = (z >> (n - 1 - role)) & 1ull;
    else if (role == -2) bit = 1ull;
    else if (role != -1) bad = true;           // a summed-out node: the host refuses it where it can look
    vals |= bit << v;
  }
  double sum = 0.0;
  for (int v = 0; v < bn.num_nodes; ++v) {
    int cfg = 0;
    const int np = bn.n_parents[v];
    for (int p = 0; p < np; ++p) cfg = cfg * 2 + (int)((vals >> bn.parents[v * bn.max_parents + p]) & 1ull);
    sum += log(fmax(bn.cpt[bn.cpt_off[v] + 2 * cfg + (int)((vals >> v) & 1ull)], p_floor));
  }
  logp[b] = bad ? __builtin_nan("") : sum;
}

// ---- exact ancestral draws from the network -------------------------------------------------
// One sample per lane, the values of all V <= 64 nodes in one 64-bit register (bit v = node v), nodes in descriptor order
// (topological: every parent index is below the node's own).  Node v:  t_s = CPT_v[parents][s] as stored,
// bit = U (t0 + t1) >= t0 (the MPS sampler's rule: a value of probability 0 is never drawn), U = unit53 of
// Philox4x32-10 with counter (b, v >> 1, BN_PHILOX_DOMAIN, epoch): even v the words (x, y), odd v (z, w).  logp is
// bn_logjoint_kernel's sum, the chosen factor unfloored.  role, n_parents, parents and cpt_off are the same for every lane
// (scalar loads); the CPT row is a gather from a table of at most a few KB that stays in cache.
constexpr uint32_t BN_PHILOX_DOMAIN = 0xfffffffeu;

__global__ __launch_bounds__(256) void bn_sample_kernel(bornvi_bn_desc bn, int n, long long B, uint32_t seed_lo, uint32_t seed_hi,
                                                        const long long* __restrict__ epoch_dev, long long* __restrict__ idx,
                                                        double* __restrict__ logp, int* status) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint32_t ep = (uint32_t)(unsigned long long)(*epoch_dev);
  unsigned long long vals = 0, z = 0;   // bit v = value of node v; the kept nodes' bits by tuple position
  bool bad = false, dead = false;
  double sum = 0.0;
  uint4 w = make_uint4(0, 0, 0, 0);
  for (int v = 0; v < bn.num_nodes; ++v) {
    if (!(v & 1)) w = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)(v >> 1), BN_PHILOX_DOMAIN, ep), seed_lo, seed_hi);
    const double U = (v & 1) ? unit53(w.z, w.w) : unit53(w.x, w.y);
    int cfg = 0;
    int np = bn.n_parents[v];
    if (np < 0 || np > bn.max_parents) { bad = true; np = 0; }
    for (int p = 0; p < np; ++p) {
      const int pa = bn.parents[v * bn.max_parents + p];
      if (pa < 0 || pa >= v) bad = true;       // not topological: the host refuses it where it can look
      cfg = cfg * 2 + (int)((vals >> (pa & 63)) & 1ull);
    }
    const double* row = bn.cpt + bn.cpt_off[v] + 2 * cfg;
    const double t0 = row[0], t1 = row[1];
    const double tot = t0 + t1;
    if (!(tot > 0.0 && isfinite(tot))) dead = true;
    const bool bit = !dead && (U * tot >= t0);
    vals |= (bit ? 1ull : 0ull) << v;
    sum += log(bit ? t1 : t0);
    const int role = bn.role[v];
    if (role >= 0 && role < n) z |= (bit ? 1ull : 0ull) << (n - 1 - role);
    else if (role != -3) bad = true;           // an observed node: the host refuses it where it can look
  }
  idx[b] = (long long)z;
  logp[b] = (bad || dead) ? __builtin_nan("") : sum;
  if (bad || dead) *status = 1;
}

}  // namespace

hipError_t launch_ms_clear_status(int* status, hipStream_t st) {
  ms_clear_status_kernel<<<1, 64, 0, st>>>(status);
  return hipGetLastError();
}

size_t mps_sample_workspace_bytes(int n, int D, long long B) { return ms_layout(n, D, B).total + 256; }

hipError_t launch_mps_environments(int n, int D, long long B, const double* cores, double* logZ_out, void* ws, hipStream_t st) {
  const MsLayout S = ms_layout(n, D, B);
  char* base = ws_align(ws);
  mps_env_kernel<<<2, MS_ENV_THREADS, 0, st>>>(cores, n, D, (double*)(base + S.E), (double*)(base + S.L), (int*)(base + S.eE),
                                           (int*)(base + S.eL), (double*)(base + S.hdr), logZ_out);
  return hipGetLastError();
}

// the same launch into a caller's own arrays (kernels_mps_query.hip keeps them in the query workspace)
hipError_t launch_mps_environments_into(int n, int D, const double* cores, double* E, double* L, int* eE, int* eL, double* hdr,
                                        hipStream_t st) {
  mps_env_kernel<<<2, MS_ENV_THREADS, 0, st>>>(cores, n, D, E, L, eE, eL, hdr, nullptr);
  return hipGetLastError();
}

hipError_t launch_mps_sample(int n, int D, long long B, const double* cores, unsigned long long seed, const long long* epoch_dev,
                             long long* idx, double* logq, int* status, void* ws, hipStream_t st) {
  const MsLayout S = ms_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((B + MS_LANES - 1) / MS_LANES);
  BOND_DISPATCH(S.DP, (mps_sample_kernel<DP><<<grid, MS_LANES, 0, st>>>(cores, n, D, B, (const double*)(base + S.E),
                                                                      (const double*)(base + S.hdr), (uint32_t)seed,
                                                                      (uint32_t)(seed >> 32), epoch_dev, idx, logq, status)));
  return hipGetLastError();
}

hipError_t launch_mps_score_vjp(int n, int D, long long B, const double* cores, const long long* idx, const double* w, double* logq,
                                double* grad_cores, int* status, void* ws, hipStream_t st) {
  const MsLayout S = ms_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const long long ntiles = (B + MS_LANES - 1) / MS_LANES;
  BOND_DISPATCH(S.DP, (mps_score_kernel<DP><<<(unsigned)S.G, MS_LANES, 0, st>>>(
                        cores, n, D, S.DS, B, ntiles, idx, w, (const double*)(base + S.hdr), logq, status, (double*)(base + S.r),
                        (int*)(base + S.er), (double*)(base + S.parts), (double*)(base + S.wpart))));
  mps_score_finish_kernel<<<(unsigned)n, MS_ENV_THREADS, 0, st>>>(cores, n, D, S.G, (const double*)(base + S.parts),
                                                              (const double*)(base + S.wpart), (const double*)(base + S.E),
                                                              (const double*)(base + S.L), (const int*)(base + S.eE),
                                                              (const int*)(base + S.eL), (const double*)(base + S.hdr), grad_cores);
  return hipGetLastError();
}

hipError_t launch_mps_score_rows(int n, int D, long long B, const double* cores, const long long* idx, int k_begin, int k_count,
                                 long long ld, double* rows, int* status, void* ws, hipStream_t st) {
  const MsLayout S = ms_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const double* hdr = nullptr;
  const double* mu = nullptr;
  e = launch_mps_score_mu(n, D, B, cores, ws, &hdr, &mu, st);
  if (e != hipSuccess) return e;
  BOND_DISPATCH(S.DP, (mps_score_rows_kernel<DP><<<(unsigned)S.G, MS_LANES, 0, st>>>(
                        cores, n, D, S.DS, B, ld / MS_LANES, idx, hdr, mu,
                        k_begin, k_count, ld, rows, status, (double*)(base + S.r), (int*)(base + S.er))));
  return hipGetLastError();
}

// after launch_mps_environments: mu into the workspace's mu region (launch_mps_score_mu), the n site partials of
// c = <mu, v> into its wpart region (MS_MAX_WG doubles >= n), then the tangent sweep
hipError_t launch_mps_score_jvp(int n, int D, long long B, const double* cores, const long long* idx, const double* v, double scale,
                                double* t, int* status, void* ws, hipStream_t st) {
  static_assert(MS_MAX_WG >= 63, "the site partials of c live in the wpart region");
  const MsLayout S = ms_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const double* hdr = nullptr;
  const double* mu = nullptr;
  e = launch_mps_score_mu(n, D, B, cores, ws, &hdr, &mu, st);
  if (e != hipSuccess) return e;
  double* cpart = (double*)(base + S.wpart);
  mps_jvp_dot_kernel<<<(unsigned)n, MS_ENV_THREADS, 0, st>>>(mu, v, D, cpart);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long ntiles = (B + MS_LANES - 1) / MS_LANES;
  BOND_DISPATCH(S.DP, (mps_score_jvp_kernel<DP><<<(unsigned)S.G, MS_LANES, 0, st>>>(cores, v, n, D, B, ntiles, idx, hdr, cpart, scale, t,
                                                                                 status)));
  return hipGetLastError();
}

// mu alone: the launch that the score rows, the jvp and kernels_mps_sample_gram.hip share, and where the header
// (log Z, E^_0[0, 0], eE[0]) and mu lie in the workspace
hipError_t launch_mps_score_mu(int n, int D, long long B, const double* cores, void* ws, const double** hdr, const double** mu,
                               hipStream_t st) {
  const MsLayout S = ms_layout(n, D, B);
  char* base = ws_align(ws);
  mps_score_mu_kernel<<<(unsigned)n, MS_ENV_THREADS, 0, st>>>(cores, D, (const double*)(base + S.E), (const double*)(base + S.L),
                                                          (const int*)(base + S.eE), (const int*)(base + S.eL),
                                                          (const double*)(base + S.hdr), (double*)(base + S.mu));
  *hdr = (const double*)(base + S.hdr);
  *mu = (const double*)(base + S.mu);
  return hipGetLastError();
}

hipError_t launch_bn_logjoint_samples(const bornvi_bn_desc& bn, int n, long long B, const long long* idx, double p_floor, double* logp,
                                      hipStream_t st) {
  bn_logjoint_kernel<<<(unsigned)((B + 255) / 256), 256, 0, st>>>(bn, n, B, idx, p_floor, logp);
  return hipGetLastError();
}

hipError_t launch_bn_sample(const bornvi_bn_desc& bn, int n, long long B, unsigned long long seed, const long long* epoch_dev,
                            long long* idx, double* logp, int* status, hipStream_t st) {
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  bn_sample_kernel<<<(unsigned)((B + 255) / 256), 256, 0, st>>>(bn, n, B, (uint32_t)seed, (uint32_t)(seed >> 32), epoch_dev, idx, logp,
                                                               status);
  return hipGetLastError();
}

}  // namespace bornvi
