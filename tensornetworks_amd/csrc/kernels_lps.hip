// Sampled matrix-product-state Born machine as a locally purified state (include/bornvi_lps.h).
//
// Parameter layout.  cores is float64 [n, 2, m, D, D], real: A_k[s, mu] in R^{D x D}, s the bit, mu = 0 .. m - 1 the
//   purification index that is summed out.  1 <= n <= 63, 1 <= D <= 16, 1 <= m <= 4, 1 <= B <= 2^24.  Bit order, index word
//   and boundary vectors e0 are section 6g's: z_k is bit n - k of the index word.
// Definitions.
//   Amplitude:  psi(z, mu) = e0^T A_1[z_1, mu_1] ... A_n[z_n, mu_n] e0.
//   Unnormalised mass:  T(z) = sum_{mu_1 .. mu_n} psi(z, mu)^2.   Normaliser and distribution:  Z = sum_z T(z),  q = T / Z.
//   Left density:  rho_0 = e0 e0^T,  rho_k = sum_mu A_k[z_k, mu]^T rho_{k-1} A_k[z_k, mu]  (symmetric, positive
//     semi-definite);  T(z) = rho_n[0, 0].
//   Right density:  R_n = e0 e0^T,  R_{k-1} = sum_mu A_k[z_k, mu] R_k A_k[z_k, mu]^T.
//   Environments:  E_n = e0 e0^T,  E_{k-1} = sum_{s,mu} A_k[s, mu] E_k A_k[s, mu]^T;   L_0 = e0 e0^T,
//     L_k = sum_{s,mu} A_k[s, mu]^T L_{k-1} A_k[s, mu];   Z = E_0[0, 0].
// Rescaling.  Every matrix (and the sampler's vector) is multiplied after every step by 2^-e, e the ilogb of its largest
//   magnitude (exact; 0 when that is 0 or not finite), and the running sum of the e's is carried beside it, as in section
//   6g.  The per-sample densities use the same rule: the largest magnitude of the 16 x 16 tile.
// Gradient of sum_b w_b log q(z_b).  Sample term: the block [k, z_{b,k}, mu] receives
//   (2 w_b / T_b) rho_{b,k-1} A_k[z_{b,k}, mu] R_{b,k}.   Environment term: every block [k, s, mu] loses
//   (sum_b w_b) 2 L_{k-1} A_k[s, mu] E_k / Z.   Entries of the first and last core that do not enter psi get exactly 0.0.
//
// lps_env_kernel: one launch of two workgroups (0: right, 1: left), n dependent steps each, one thread per entry (D D <= 256).
//   Section 6g's ms_env_step chain with j = (s, mu), s major, as the outer loop:  T_j = A_j X (left: A_j^T X), chain over c;
//   X'[a][b] = sum_j sum_d T_j[a][d] A_j[b][d] (left: A_j[d][b]), one fma chain, j outer / d inner; then times 2^-e.  At m = 1
//   these are mps_env_kernel's chains: the same bits.
// lps_sample_kernel<DP>: one sample per lane, one wave per workgroup; l (DP doubles) in registers, the site's 2 m matrices and
//   E^_k zero-padded in LDS.  For j = 0 .. 2 m - 1 in turn: u_j = l A_j (ms_row_dot), t[d] = sum_c u_j[c] E^_k[c][d],
//   m_j = sum_d t[d] u_j[d] (the real sampler's chains), kept in a lane-private LDS column.  M0, M1 ascending in mu, z_k and mu_k
//   as in the header; then l = u_{z_k,mu_k} 2^-e, computed again from the lane's own matrix (one product more, no 2 m vectors
//   in registers).  A sample whose M is 0 or not finite: status 1, remaining bits and mu's 0.
// lps_score_kernel<M>: at most G workgroups of LP_WAVES = 4 waves, each walking the tiles wg, wg + G, ... of LP_TILE = 16 samples;
//   a wave owns four consecutive samples of a tile and takes them one at a time, the site's matrices are shared in LDS.  A
//   density is one 16 x 16 accumulator tile of v_mfma_f64_16x16x4_f64: lane l holds, in register j, the entry
//   [row 4 j + (l >> 4)][col l & 15].  That register is the B operand of K-step j of a product X . (anything), and, for a
//   symmetric X, also the A operand of K-step j of (anything) . X -- the kernel uses the stored tile as its own transpose: the
//   recursion it runs is X -> sum_mu A^T X^T A, which agrees with the definition on symmetric X; the asymmetry of the
//   computed X is a rounding error like the others and is carried in the error bound, nothing is
//   symmetrised.  With a[j] = A_mu[4 j + (l >> 4)][l & 15] and aT[j] = A_mu[l & 15][4 j + (l >> 4)] read from LDS:
//     left step   Y = rho A_mu:  4 MFMAs (A operand rho[j], B operand a[j]);   rho' += A_mu^T Y:  4 MFMAs (a[j], Y[j])
//     right step  V = R A_mu^T:  4 MFMAs (R[j], aT[j]);                        R' += A_mu V:      4 MFMAs (aT[j], V[j])
//     gradient    W = A_mu R_k:  4 MFMAs (aT[j], R_k[j]);   G[s, mu] += (c_b rho_{k-1}) W:  4 MFMAs (c_b rho[j], W[j])
//   8 MFMAs per (sample, mu, site) for a density sweep, 16 for the left sweep with the gradient, and no cross-lane move but the
//   rescaling's maximum.  The sum over samples of a gradient block is the long-K product [c_1 rho_1 .. ][W_1; ..]: it stays in
//   one accumulator tile per (s, mu) and wave over the wave's samples in sample order, and the waves add theirs in wave order
//   (a barrier between two) into the workgroup's own partial [n, 2, m, D, D] (first tile, first wave: stores).  Between
//   sites a sample's density waits in LDS ([sample][register][lane]); the right densities R_1 .. R_{n-1} and their exponents
//   go to the workgroup's slice [n][16][D D] of the workspace.
//   c_b = 2 w_b / R^_0[0, 0] times 2^(e_rho_{k-1} + e_R_k - e_R_0) (0 when R^_0[0, 0] is 0 or not finite, or Z is).
//   logq_b = log rho^_n[0, 0] - log Z^ + (e_rho_n - eE[0]) ln 2, from the left sweep whether or not a gradient is asked for.
// lps_score_finish_kernel, one workgroup per site: the partials in workgroup order, sum_b w_b, and the environment term
//   2 L_{k-1} A_j E_k / Z as T_j = A_j E^_k (chain over c), M_j = L^_{k-1} T_j (chain over c), times
//   2^(eL[k-1] + eE[k] - eE[0]) / E^_0[0, 0]: section 6g's ms_env_stage / ms_env_entry over 2 m matrices.
//
// Workspace (lp_layout; every region 256-byte aligned): header (log Z, E^_0[0, 0], eE[0]); E^ [n + 1][D][D]; L^ the same; eE,
//   eL int [n + 1]; right densities [G][n][16][D D]; their exponents int [G][n][16]; partials [G][n, 2, m, D, D]; weight
//   totals [1024].  G = min(tiles, D <= 8 ? 1024 : 256): bounded in B, 0.74 GiB at (63, 4, 16) and at (63, 4, 8).
//
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.  The status word is cleared by
// the one-lane kernel of kernels_mps_sample.hip in front of the launch and set by plain stores.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bornvi_lps.h"
#include "kernels.hpp"
#include "mps_sample_dev.hpp"
#include "philox_dev.hpp"

namespace bornvi {

namespace {
constexpr int LP_DMAX = BORNVI_LPS_MAX_BOND;
constexpr int LP_MMAX = BORNVI_LPS_MAX_PURIFICATION;
constexpr int LP_TILE = BORNVI_LPS_SCORE_TILE;
constexpr int LP_PITCH = 17;               // row pitch of a site's matrices in the score kernel's LDS (odd: aT reads spread over the banks)
constexpr int LP_MAT = 16 * LP_PITCH;
constexpr int LP_WAVES = 4;                // score kernel: waves per workgroup, each owning LP_TILE / LP_WAVES samples of a tile
constexpr int LP_THREADS = 64 * LP_WAVES;
constexpr int LP_PER_WAVE = LP_TILE / LP_WAVES;
static_assert(LP_DMAX == 16, "one 16 x 16 matrix-core tile per density");

typedef double lp_d4 __attribute__((ext_vector_type(4)));

inline int lp_max_wg(int D) { return D > 8 ? BORNVI_LPS_MAX_WG_LARGE : BORNVI_LPS_MAX_WG_SMALL; }

struct LpLayout {
  int DP, G;
  size_t hdr, E, L, eE, eL, R, eR, parts, wpart, total;   // byte offsets from the aligned base
};

LpLayout lp_layout(int n, int m, int D, long long B) {
  LpLayout S;
  S.DP = bond_dp(D);
  const long long tiles = (B + LP_TILE - 1) / LP_TILE;
  S.G = (int)(tiles < lp_max_wg(D) ? tiles : lp_max_wg(D));
  size_t o = 0;
  S.hdr = o;   o += 256;
  S.E = o;     o += ws_round((size_t)(n + 1) * D * D * sizeof(double));
  S.L = o;     o += ws_round((size_t)(n + 1) * D * D * sizeof(double));
  S.eE = o;    o += ws_round((size_t)(n + 1) * sizeof(int));
  S.eL = o;    o += ws_round((size_t)(n + 1) * sizeof(int));
  S.R = o;     o += ws_round((size_t)S.G * n * LP_TILE * D * D * sizeof(double));   // slot k of a slice: R^_k, k = 1 .. n - 1
  S.eR = o;    o += ws_round((size_t)S.G * n * LP_TILE * sizeof(int));
  S.parts = o; o += ws_round((size_t)S.G * n * 2 * m * D * D * sizeof(double));
  S.wpart = o; o += ws_round((size_t)BORNVI_LPS_MAX_WG_SMALL * sizeof(double));
  S.total = o;
  return S;
}

// ---- environments ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_ENV_THREADS) void lps_env_kernel(const double* __restrict__ cores, int n, int m, int D,
                                                              double* __restrict__ E, double* __restrict__ L, int* __restrict__ eE,
                                                              int* __restrict__ eL, double* __restrict__ hdr,
                                                              double* __restrict__ logZ_out) {
  static_assert(LP_DMAX * LP_DMAX <= MS_ENV_THREADS, "one thread per entry");
  __shared__ double As[2 * LP_MMAX * LP_DMAX * LP_DMAX];
  __shared__ double T[2 * LP_MMAX * LP_DMAX * LP_DMAX];
  __shared__ double X[LP_DMAX * LP_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  const bool right = blockIdx.x == 0;
  double* out = right ? E : L;
  int* eo = right ? eE : eL;
  const int DD = D * D, S = 2 * m, t = threadIdx.x;
  if (t < DD) {
    X[t] = t == 0 ? 1.0 : 0.0;
    out[(long long)(right ? n : 0) * DD + t] = X[t];
  }
  if (t == 0) eo[right ? n : 0] = 0;
  int ex = 0;
  for (int step = 0; step < n; ++step) {
    const int k = right ? n - step : step + 1;       // the site whose matrices this step uses
    const int dst = right ? k - 1 : k;
    __syncthreads();
    for (int i = t; i < S * DD; i += MS_ENV_THREADS) As[i] = cores[(long long)(k - 1) * S * DD + i];
    __syncthreads();
    for (int i = t; i < S * DD; i += MS_ENV_THREADS) {      // T_j = A_j X (A_j^T X)
      const int j = i / DD, a = (i % DD) / D, d = i % D;
      double acc = 0.0;
      for (int c = 0; c < D; ++c) acc = fma(right ? As[j * DD + a * D + c] : As[j * DD + c * D + a], X[c * D + d], acc);
      T[i] = acc;
    }
    __syncthreads();
    double v = 0.0, mx = 0.0;
    if (t < DD) {
      const int a = t / D, b = t % D;
      for (int j = 0; j < S; ++j)
        for (int d = 0; d < D; ++d) v = fma(T[j * DD + a * D + d], right ? As[j * DD + b * D + d] : As[j * DD + d * D + b], v);
      mx = fabs(v);
    }
    mx = wave_max(mx);
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    const int e = ms_exponent(mx);
    if (t < DD) {
      const double x = ldexp(v, -e);
      X[t] = x;
      out[(long long)dst * DD + t] = x;
    }
    ex += e;
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

// ---- sampler ---------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(MS_LANES) void lps_sample_kernel(const double* __restrict__ cores, int n, int m, int D, long long B,
                                                              const double* __restrict__ E, uint32_t seed_lo, uint32_t seed_hi,
                                                              const long long* __restrict__ epoch_dev, long long* __restrict__ idx,
                                                              long long* __restrict__ aux, int* status) {
  __shared__ double As[2 * LP_MMAX * DP * DP];
  __shared__ double Es[DP * DP];
  __shared__ double Pm[2 * LP_MMAX * MS_LANES];      // m_j of the lane's sample: column `lane`
  const int lane = threadIdx.x, S = 2 * m;
  const long long b = (long long)blockIdx.x * MS_LANES + lane;
  const bool active = b < B;
  const uint32_t ep = (uint32_t)(unsigned long long)(*epoch_dev);
  double l[DP];
  ms_fill<DP>(l, 1.0);
  unsigned long long z = 0, a0 = 0, a1 = 0;
  bool dead = false;
  uint4 w = make_uint4(0, 0, 0, 0);
#pragma unroll 1
  for (int k = 1; k <= n; ++k) {
    __syncthreads();
    {
      const double* A = cores + (long long)(k - 1) * S * D * D;
      for (int i = lane; i < S * DP * DP; i += MS_LANES) {
        const int j = i / (DP * DP), a = (i / DP) % DP, c = i % DP;
        As[i] = (a < D && c < D) ? A[(j * D + a) * D + c] : 0.0;
      }
      const double* Ek = E + (long long)k * D * D;
      for (int i = lane; i < DP * DP; i += MS_LANES) {
        const int a = i / DP, c = i % DP;
        Es[i] = (a < D && c < D) ? Ek[a * D + c] : 0.0;
      }
    }
    __syncthreads();
    if (k & 1) w = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)((k + 1) / 2 - 1), MS_PHILOX_DOMAIN, ep), seed_lo, seed_hi);
    const double U = (k & 1) ? unit53(w.x, w.y) : unit53(w.z, w.w);
#pragma unroll 1
    for (int j = 0; j < S; ++j) {
      asm volatile("" ::: "memory");      // E^_k is read from LDS in every turn: hoisted out of the loop it takes DP DP registers
      const double* Aj = As + j * DP * DP;
      double u[DP];
#pragma unroll
      for (int c = 0; c < DP; ++c) u[c] = ms_row_dot<DP>(l, Aj, c, 0.0);
      double mj = 0.0;
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        double tt = 0.0;
#pragma unroll
        for (int c = 0; c < DP; ++c) tt = fma(u[c], Es[c * DP + d], tt);
        mj = fma(tt, u[d], mj);
      }
      Pm[j * MS_LANES + lane] = mj;
    }
    double M0 = Pm[lane], M1 = Pm[m * MS_LANES + lane];
    for (int mu = 1; mu < m; ++mu) {
      M0 += Pm[mu * MS_LANES + lane];
      M1 += Pm[(m + mu) * MS_LANES + lane];
    }
    const double tot = M0 + M1;
    if (!dead && !(tot > 0.0 && isfinite(tot))) {
      dead = true;
      if (active) *status = 1;
    }
    const bool bit = !dead && (U * tot >= M0);
    const double v = bit ? U * tot - M0 : U * tot;
    const int base = bit ? m : 0;
    int mu_k = 0;
    double cj = 0.0;
    for (int j = 0; j < m - 1; ++j) {
      const double pj = Pm[(base + j) * MS_LANES + lane];
      cj = j == 0 ? pj : cj + pj;
      if (!dead && v >= cj) ++mu_k;
    }
    z = (z << 1) | (bit ? 1ull : 0ull);
    if (k <= 32) a0 |= (unsigned long long)mu_k << (2 * (k - 1));
    else a1 |= (unsigned long long)mu_k << (2 * (k - 33));
    const double* Aj = As + (base + mu_k) * DP * DP;      // the lane's own matrix
    double ln[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) ln[c] = ms_row_dot<DP>(l, Aj, c, 0.0);
    ms_take<DP>(l, ln);
  }
  if (active) {
    idx[b] = (long long)z;
    if (aux) {
      aux[2 * b] = (long long)a0;
      aux[2 * b + 1] = (long long)a1;
    }
  }
}

// ---- densities on the matrix cores -----------------------------------------------------------------------------
__device__ __forceinline__ lp_d4 lp_zero() { return (lp_d4){0.0, 0.0, 0.0, 0.0}; }

// e0 e0^T as an accumulator tile: entry [0][0] is register 0 of lane 0
__device__ __forceinline__ lp_d4 lp_e0(int lane) { return (lp_d4){lane == 0 ? 1.0 : 0.0, 0.0, 0.0, 0.0}; }

// C + A B over K = 16: a[j], b[j] the lane's A and B operands of K-step j
__device__ __forceinline__ lp_d4 lp_mma(const lp_d4 a, const lp_d4 b, lp_d4 c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], b[j], c, 0, 0, 0);
  return c;
}

// x <- x 2^-e, e = ilogb of the tile's largest magnitude, returned (the same e in every lane)
__device__ __forceinline__ int lp_rescale(lp_d4& x) {
  const double mx = wave_max(fmax(fmax(fabs(x[0]), fabs(x[1])), fmax(fabs(x[2]), fabs(x[3]))));
  const int e = ms_exponent(mx);
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = ldexp(x[j], -e);
  return e;
}

// the site's 2 M matrices zero-padded to 16 x 16, pitch LP_PITCH: As[j][row][col]
template <int M>
__device__ __forceinline__ void lp_load_site(const double* cores, int k, int D, double* As) {
  const double* A = cores + (long long)(k - 1) * 2 * M * D * D;
  for (int i = threadIdx.x; i < 2 * M * 256; i += LP_THREADS) {
    const int j = i >> 8, a = (i >> 4) & 15, c = i & 15;
    As[j * LP_MAT + a * LP_PITCH + c] = (a < D && c < D) ? A[(j * D + a) * D + c] : 0.0;
  }
}

__device__ __forceinline__ lp_d4 lp_lds_tile(const double* p, int lane) {
  return (lp_d4){p[lane], p[64 + lane], p[128 + lane], p[192 + lane]};
}
__device__ __forceinline__ void lp_lds_store(double* p, int lane, const lp_d4 x) {
#pragma unroll
  for (int j = 0; j < 4; ++j) p[64 * j + lane] = x[j];
}

template <int M>
__global__ __launch_bounds__(LP_THREADS) void lps_score_kernel(const double* __restrict__ cores, int n, int D, long long B,
                                                             long long ntiles, const long long* __restrict__ idx,
                                                             const double* __restrict__ wgt, const double* __restrict__ hdr,
                                                             double* __restrict__ logq, int* status, double* Rws, int* eRws,
                                                             double* parts, double* __restrict__ wpart, int want_grad) {
  __shared__ double As[2 * M * LP_MAT];
  __shared__ double Rho[LP_TILE * 256];      // a sample's density between sites: [sample][register][lane]
  __shared__ unsigned long long Zs[LP_TILE];
  __shared__ double Ws[LP_TILE], Gc[LP_TILE];
  __shared__ int Ex[LP_TILE], Er0[LP_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4, DD = D * D;
  const int t0 = wave * LP_PER_WAVE;          // the wave's samples of a tile: t0 .. t0 + LP_PER_WAVE - 1
  double* Rsl = Rws + (size_t)blockIdx.x * n * LP_TILE * DD;
  int* eRsl = eRws + (size_t)blockIdx.x * n * LP_TILE;
  double* part = parts + (size_t)blockIdx.x * n * 2 * M * DD;
  const double Zh = hdr[1], eE0 = hdr[2];
  const bool Zok = ms_norm_ok(Zh);
  const double logZh = log(Zh);
  double wacc = 0.0;
  bool first = true;
#pragma unroll 1
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x, first = false) {
    const long long b0 = tile * LP_TILE;
    const int nact = (int)(B - b0 < LP_TILE ? B - b0 : LP_TILE);
    __syncthreads();
    const int t1 = nact < t0 + LP_PER_WAVE ? nact : t0 + LP_PER_WAVE;
    if (tid < LP_TILE) {
      const bool act = tid < nact;
      Zs[tid] = act ? (unsigned long long)idx[b0 + tid] : 0ull;
      Ws[tid] = (act && want_grad) ? wgt[b0 + tid] : 0.0;
    }
    __syncthreads();
    if (want_grad) {
      for (int t = 0; t < LP_TILE; ++t) wacc += Ws[t];
      // right to left: R^_1 .. R^_{n-1} and their exponents into the slice
      for (int t = t0; t < t1; ++t) lp_lds_store(Rho + t * 256, lane, lp_e0(lane));
      if (tid < LP_TILE) Ex[tid] = 0;
#pragma unroll 1
      for (int k = n; k >= 1; --k) {
        __syncthreads();
        lp_load_site<M>(cores, k, D, As);
        __syncthreads();
#pragma unroll 1
        for (int t = t0; t < t1; ++t) {
          const lp_d4 R = lp_lds_tile(Rho + t * 256, lane);
          const int er = Ex[t];
          if (k < n) {
            double* dst = Rsl + ((size_t)k * LP_TILE + t) * DD;
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (4 * j + fk < D && fr < D) dst[(4 * j + fk) * D + fr] = R[j];
            if (lane == 0) eRsl[k * LP_TILE + t] = er;
          }
          const int s = ms_bit(Zs[t], n, k);
          lp_d4 Rn = lp_zero();
#pragma unroll
          for (int mu = 0; mu < M; ++mu) {
            const double* Aj = As + (s * M + mu) * LP_MAT;
            lp_d4 aT;
#pragma unroll
            for (int j = 0; j < 4; ++j) aT[j] = Aj[fr * LP_PITCH + 4 * j + fk];
            const lp_d4 V = lp_mma(R, aT, lp_zero());      // R A^T
            Rn = lp_mma(aT, V, Rn);                        // += A (R A^T)
          }
          const int e = lp_rescale(Rn);
          lp_lds_store(Rho + t * 256, lane, Rn);
          if (lane == 0) Ex[t] = er + e;
        }
      }
      __syncthreads();
      if (tid < LP_TILE) {
        const double h = Rho[tid * 256];      // R^_0[0, 0]
        const bool good = tid < nact && ms_amplitude_ok(h, Zok);
        Gc[tid] = good ? (Ws[tid] + Ws[tid]) / h : 0.0;
        Er0[tid] = Ex[tid];
        if (tid < nact && !good) *status = 2;
      }
    }
    // left to right
    __syncthreads();
    for (int t = t0; t < t1; ++t) lp_lds_store(Rho + t * 256, lane, lp_e0(lane));
    if (tid < LP_TILE) Ex[tid] = 0;
#pragma unroll 1
    for (int k = 1; k <= n; ++k) {
      __syncthreads();
      lp_load_site<M>(cores, k, D, As);
      __syncthreads();
      lp_d4 G0[M], G1[M];
#pragma unroll
      for (int mu = 0; mu < M; ++mu) {
        G0[mu] = lp_zero();
        G1[mu] = lp_zero();
      }
#pragma unroll 1
      for (int t = t0; t < t1; ++t) {
        const lp_d4 rho = lp_lds_tile(Rho + t * 256, lane);
        const int el = Ex[t];
        const int s = __builtin_amdgcn_readfirstlane(ms_bit(Zs[t], n, k));
        lp_d4 Rk = lp_e0(lane), rs = lp_zero();
        if (want_grad) {
          int erk = 0;
          if (k < n) {
            const double* src = Rsl + ((size_t)k * LP_TILE + t) * DD;
#pragma unroll
            for (int j = 0; j < 4; ++j) Rk[j] = (4 * j + fk < D && fr < D) ? src[(4 * j + fk) * D + fr] : 0.0;
            erk = eRsl[k * LP_TILE + t];
          }
          const double cf = ms_site_factor(Gc[t], el, erk, Er0[t]);
#pragma unroll
          for (int j = 0; j < 4; ++j) rs[j] = cf * rho[j];
        }
        lp_d4 rn = lp_zero();
#pragma unroll
        for (int mu = 0; mu < M; ++mu) {
          const double* Aj = As + (s * M + mu) * LP_MAT;
          lp_d4 a;
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = Aj[(4 * j + fk) * LP_PITCH + fr];
          const lp_d4 Y = lp_mma(rho, a, lp_zero());      // rho A
          rn = lp_mma(a, Y, rn);                          // += A^T (rho A)
          if (want_grad) {
            lp_d4 aT;
#pragma unroll
            for (int j = 0; j < 4; ++j) aT[j] = Aj[fr * LP_PITCH + 4 * j + fk];
            const lp_d4 W = lp_mma(aT, Rk, lp_zero());    // A R_k
            if (s == 0) G0[mu] = lp_mma(rs, W, G0[mu]);   // += c rho (A R_k)
            else G1[mu] = lp_mma(rs, W, G1[mu]);
          }
        }
        const int e = lp_rescale(rn);
        lp_lds_store(Rho + t * 256, lane, rn);
        if (lane == 0) Ex[t] = el + e;
      }
      if (want_grad) {
        // D[row = fk + 4 j][col = fr]: entry (a = fk + 4 j, c = fr) of the block; the waves add their tiles in wave order
        double* pk = part + (size_t)(k - 1) * 2 * M * DD;
#pragma unroll 1
        for (int wv = 0; wv < LP_WAVES; ++wv) {
          if (wave == wv) {
            const bool store = first && wv == 0;
#pragma unroll
            for (int mu = 0; mu < M; ++mu)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int a = fk + 4 * j;
                if (a < D && fr < D) {
                  double* p0 = pk + (size_t)mu * DD + a * D + fr;
                  double* p1 = pk + (size_t)(M + mu) * DD + a * D + fr;
                  *p0 = store ? G0[mu][j] : *p0 + G0[mu][j];
                  *p1 = store ? G1[mu][j] : *p1 + G1[mu][j];
                }
              }
          }
          __syncthreads();
        }
      }
    }
    __syncthreads();
    if (tid < nact) {
      const double h = Rho[tid * 256];        // rho^_n[0, 0]
      logq[b0 + tid] = (log(h) - logZh) + ((double)Ex[tid] - eE0) * MS_LN2;
      if (!ms_amplitude_ok(h, Zok)) *status = 2;
    }
  }
  if (want_grad && tid == 0) wpart[blockIdx.x] = wacc;
}

// grid n: grad[k - 1] = the workgroups' partials in order - (sum_b w_b) 2 L_{k-1} A_j E_k / Z
__global__ __launch_bounds__(MS_ENV_THREADS) void lps_score_finish_kernel(const double* __restrict__ cores, int n, int m, int D, int G,
                                                                       const double* __restrict__ parts,
                                                                       const double* __restrict__ wpart, const double* __restrict__ E,
                                                                       const double* __restrict__ L, const int* __restrict__ eE,
                                                                       const int* __restrict__ eL, const double* __restrict__ hdr,
                                                                       double* __restrict__ grad) {
  __shared__ double As[2 * LP_MMAX * LP_DMAX * LP_DMAX];
  __shared__ double T[2 * LP_MMAX * LP_DMAX * LP_DMAX];
  __shared__ double Em[LP_DMAX * LP_DMAX], Lm[LP_DMAX * LP_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  const int k = blockIdx.x + 1, t = threadIdx.x, DD = D * D, S = 2 * m;
  double wv = 0.0;
  for (int i = t; i < G; i += MS_ENV_THREADS) wv += wpart[i];
  wv = wave_sum(wv);
  if ((t & 63) == 0) red[t >> 6] = wv;
  for (int i = t; i < S * DD; i += MS_ENV_THREADS) As[i] = cores[(long long)(k - 1) * S * DD + i];
  if (t < DD) {
    Em[t] = E[(long long)k * DD + t];
    Lm[t] = L[(long long)(k - 1) * DD + t];
  }
  __syncthreads();
  for (int i = t; i < S * DD; i += MS_ENV_THREADS) {      // T_j = A_j E^_k
    const int j = i / DD, a = (i % DD) / D, d = i % D;
    double acc = 0.0;
    for (int c = 0; c < D; ++c) acc = fma(As[j * DD + a * D + c], Em[c * D + d], acc);
    T[i] = acc;
  }
  __syncthreads();
  const double W = ((red[0] + red[1]) + red[2]) + red[3];
  const int ex = eL[k - 1] + eE[k] - eE[0];
  const double Zh = hdr[1];
  const size_t stride = (size_t)n * S * DD;
  for (int i = t; i < S * DD; i += MS_ENV_THREADS) {      // M_j = L^_{k-1} T_j
    const int j = i / DD, a = (i % DD) / D, d = i % D;
    double mm = 0.0;
    for (int c = 0; c < D; ++c) mm = fma(Lm[a * D + c], T[j * DD + c * D + d], mm);
    const double env = ldexp(mm / Zh, ex);
    double sum = 0.0;
    const double* p = parts + (size_t)(k - 1) * S * DD + i;
    for (int g = 0; g < G; ++g) sum += p[g * stride];
    grad[(size_t)(k - 1) * S * DD + i] = sum - W * (env + env);
  }
}

}  // namespace

size_t lps_workspace_bytes(int n, int m, int D, long long B) { return lp_layout(n, m, D, B).total + 256; }

hipError_t launch_lps_environments(int n, int m, int D, long long B, const double* cores, double* logZ_out, void* ws, hipStream_t st) {
  const LpLayout S = lp_layout(n, m, D, B);
  char* base = ws_align(ws);
  lps_env_kernel<<<2, MS_ENV_THREADS, 0, st>>>(cores, n, m, D, (double*)(base + S.E), (double*)(base + S.L), (int*)(base + S.eE),
                                           (int*)(base + S.eL), (double*)(base + S.hdr), logZ_out);
  return hipGetLastError();
}

hipError_t launch_lps_sample(int n, int m, int D, long long B, const double* cores, unsigned long long seed, const long long* epoch_dev,
                             long long* idx, long long* aux, int* status, void* ws, hipStream_t st) {
  const LpLayout S = lp_layout(n, m, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((B + MS_LANES - 1) / MS_LANES);
  switch (S.DP) {
#define LPS_SAMPLE_CASE(DPV)                                                                                                        \
  case DPV:                                                                                                                         \
    lps_sample_kernel<DPV><<<grid, MS_LANES, 0, st>>>(cores, n, m, D, B, (const double*)(base + S.E), (uint32_t)seed,               \
                                                      (uint32_t)(seed >> 32), epoch_dev, idx, aux, status);                         \
    break;
    LPS_SAMPLE_CASE(2)
    LPS_SAMPLE_CASE(4)
    LPS_SAMPLE_CASE(8)
    default:
      LPS_SAMPLE_CASE(16)
#undef LPS_SAMPLE_CASE
  }
  return hipGetLastError();
}

hipError_t launch_lps_score_vjp(int n, int m, int D, long long B, const double* cores, const long long* idx, const double* w,
                                double* logq, double* grad_cores, int* status, void* ws, hipStream_t st) {
  const LpLayout S = lp_layout(n, m, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const long long ntiles = (B + LP_TILE - 1) / LP_TILE;
  const int want = grad_cores != nullptr;
  switch (m) {
#define LPS_SCORE_CASE(MV)                                                                                                          \
  case MV:                                                                                                                          \
    lps_score_kernel<MV><<<(unsigned)S.G, LP_THREADS, 0, st>>>(cores, n, D, B, ntiles, idx, w, (const double*)(base + S.hdr), logq,   \
                                                             status, (double*)(base + S.R), (int*)(base + S.eR),                    \
                                                             (double*)(base + S.parts), (double*)(base + S.wpart), want);           \
    break;
    LPS_SCORE_CASE(1)
    LPS_SCORE_CASE(2)
    LPS_SCORE_CASE(3)
    default:
      LPS_SCORE_CASE(4)
#undef LPS_SCORE_CASE
  }
  e = hipGetLastError();
  if (e != hipSuccess || !want) return e;
  lps_score_finish_kernel<<<(unsigned)n, MS_ENV_THREADS, 0, st>>>(cores, n, m, D, S.G, (const double*)(base + S.parts),
                                                              (const double*)(base + S.wpart), (const double*)(base + S.E),
                                                              (const double*)(base + S.L), (const int*)(base + S.eE),
                                                              (const int*)(base + S.eL), (const double*)(base + S.hdr), grad_cores);
  return hipGetLastError();
}

}  // namespace bornvi
