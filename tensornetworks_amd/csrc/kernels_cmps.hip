// Sampled matrix-product-state Born machine with complex cores (include/bornvi_cmps.h).
//
// Conventions.  cores is float64 [n, 2, D, D, 2] with (re, im) last: torch.view_as_real of a complex128 [n, 2, D, D].
//   A_k[s] = X + iY.   psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0 in C: a plain product, no conjugate.
//   q(z) = |psi(z)|^2 / Z,  Z = sum_z |psi(z)|^2.   Bit order, index word and boundary vectors as in section 6g:
//   z_k is bit n - k of the index word.   1 <= n <= 63, 1 <= D <= 16, 1 <= B <= 2^24.
// Environments, Hermitian and positive semi-definite:
//   E_n = e0 e0^T,  E_{k-1} = sum_s A_k[s] E_k A_k[s]^H;   L_0 = e0 e0^T,  L_k = sum_s A_k[s]^T L_{k-1} conj(A_k[s]);   Z = Re E_0[0, 0].
//   After every step the matrix is multiplied by 2^-e, e = ilogb of its largest |re| or |im| (exact), and the running sum
//   of the e's is stored beside it.  log Z = log E^_0[0, 0] + eE[0] ln 2.
//
// Complex products.  Re and im are separate planes in LDS and separate arrays in registers.  Every entry is one fma chain
// per part, over the summation index in order, the two real products of a term one after the other:
//   re:  acc = fma(xr, yr, acc); acc = fma(-xi, yi, acc)        im:  acc = fma(xr, yi, acc); acc = fma(xi, yr, acc)
// (with conj(y): re + xi yi, im: xi yr - xr yi).  With every imaginary part +0.0 the second product of re adds an exact zero,
// so re is the real kernels' chain (mps_sample_dev.hpp) bit for bit, and im stays +0.0.  Rescaling exponents are taken over
// re and im together.
//
// cmps_env_kernel: one launch of two workgroups (0: right, 1: left), n dependent steps each, one thread per entry (D D <= 256).
//   T_s = A_s X (left: A_s^T X), chain over c;  X'[a][b] = sum_s sum_d T_s[a][d] conj(A_s[b][d]) (left: conj(A_s[d][b])), chain
//   s outer / d inner.  The thread of (a, b) computes the entry (min, max) and takes its conjugate below the diagonal; the
//   diagonal's imaginary part is set to 0.0: the stored matrices are Hermitian bit for bit.
// cmps_sample_kernel<DP>: one sample per lane, one wave per workgroup; l (DP complex) in registers, A_k[0], A_k[1], E^_k
//   zero-padded in LDS and read as broadcasts.  u_s = l A_k[s] (chain over a, the two s in one loop), t_s[d] = sum_c u_s[c] E^_k[c][d],
//   m_s = sum_d (Re t_s[d] Re u_s[d] + Im t_s[d] Im u_s[d]): the real part of u_s E u_s^H only.  z_k = [U_k (m_0 + m_1) >= m_0],
//   U_k the uniform of bornvi_mps_sample (kernels_mps_sample.hip: same key, counter and words).  l = u_{z_k} 2^-e.
//   logq = ms_logq(|l^_n[0]|, el) with |.| = hypot.  m_0 + m_1 zero or not finite: status 1, remaining bits 0, logq NaN.
// cmps_score_kernel<DP>: the real score kernel's grid: at most CM_MAX_WG workgroups of one wave, each walking the 64-sample
//   tiles wg, wg + G, ...  Right to left r <- A_k[z_k] r (chain over c), r^_1 .. r^_{n-1} and their exponents into the
//   workgroup's slice.  psi_b = r^_0[0] 2^er_0.  Left to right: X_b = g_b 2^(el + er_k - er_0) l^_{k-1} with g_b = 2 w_b / r^_0[0]
//   (complex; 0 for a sample whose amplitude is 0 or not finite: status 2), R_b = r^_k; per s the two 16 x 16 tiles
//     dX += Xr^T Rr - Xi^T Ri,   dY += -(Xr^T Ri + Xi^T Rr)
//   are four v_mfma_f64_16x16x4_f64 a step of 4 samples, 16 steps a tile.  The workgroup adds the tiles into its own partial
//   [n, 2, D, D, 2] (first tile: stores).
// cmps_score_finish_kernel, one workgroup per site: the partials in workgroup order, sum_b w_b as in the real finish kernel,
//   and G_k[s] = L_{k-1} conj(A_k[s]) E_k^T / Z as T_s = conj(A_s) E^_k^T (chain over c'), M_s = L^_{k-1} T_s (chain over a'),
//   times 2^(eL[k-1] + eE[k] - eE[0]) / E^_0[0, 0]:   grad_X = parts - W 2 Re G,  grad_Y = parts + W 2 Im G.
//
// Workspace (cm_layout; every region 256-byte aligned): header (log Z, E^_0[0, 0], eE[0]); E^ [n + 1][re, im][D][D]; L^ the
//   same; eE, eL int [n + 1]; slices [G][n][64][re D | im D]; slice exponents int [G][n][64]; partials [G][n, 2, D, D, 2];
//   weight totals [256].  G = min(tiles, 256): bounded in B.
//
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.  The status word is cleared by
// the one-lane kernel of kernels_mps_sample.hip in front of the launch and set by plain stores.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "mps_sample_dev.hpp"
#include "philox_dev.hpp"

namespace bornvi {

namespace {
constexpr int CM_MAX_WG = 256;
constexpr int CM_DMAX = 16;

typedef double cm_d4 __attribute__((ext_vector_type(4)));

struct CmLayout {
  int DP, G;
  size_t hdr, E, L, eE, eL, r, er, parts, wpart, total;   // byte offsets from the aligned base
};

CmLayout cm_layout(int n, int D, long long B) {
  CmLayout S;
  S.DP = bond_dp(D);
  const long long tiles = (B + MS_LANES - 1) / MS_LANES;
  S.G = (int)(tiles < CM_MAX_WG ? tiles : CM_MAX_WG);
  size_t o = 0;
  S.hdr = o;   o += 256;
  S.E = o;     o += ws_round((size_t)(n + 1) * 2 * D * D * sizeof(double));
  S.L = o;     o += ws_round((size_t)(n + 1) * 2 * D * D * sizeof(double));
  S.eE = o;    o += ws_round((size_t)(n + 1) * sizeof(int));
  S.eL = o;    o += ws_round((size_t)(n + 1) * sizeof(int));
  S.r = o;     o += ws_round((size_t)S.G * n * MS_LANES * 2 * D * sizeof(double));
  S.er = o;    o += ws_round((size_t)S.G * n * MS_LANES * sizeof(int));
  S.parts = o; o += ws_round((size_t)S.G * n * 4 * D * D * sizeof(double));
  S.wpart = o; o += ws_round((size_t)CM_MAX_WG * sizeof(double));
  S.total = o;
  return S;
}

// ---- environments ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_ENV_THREADS) void cmps_env_kernel(const double* __restrict__ cores, int n, int D, double* __restrict__ E,
                                                               double* __restrict__ L, int* __restrict__ eE, int* __restrict__ eL,
                                                               double* __restrict__ hdr, double* __restrict__ logZ_out) {
  static_assert(CM_DMAX * CM_DMAX <= MS_ENV_THREADS, "one thread per entry");
  __shared__ double Ar[2 * CM_DMAX * CM_DMAX], Ai[2 * CM_DMAX * CM_DMAX];
  __shared__ double Xr[CM_DMAX * CM_DMAX], Xi[CM_DMAX * CM_DMAX];
  __shared__ double Tr[2 * CM_DMAX * CM_DMAX], Ti[2 * CM_DMAX * CM_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  const bool right = blockIdx.x == 0;
  double* out = right ? E : L;
  int* eo = right ? eE : eL;
  const int DD = D * D, t = threadIdx.x;
  if (t < DD) {
    Xr[t] = t == 0 ? 1.0 : 0.0;
    Xi[t] = 0.0;
    double* o = out + (long long)(right ? n : 0) * 2 * DD;
    o[t] = Xr[t];
    o[DD + t] = 0.0;
  }
  if (t == 0) eo[right ? n : 0] = 0;
  int ex = 0;
  for (int step = 0; step < n; ++step) {
    const int k = right ? n - step : step + 1;       // the site whose matrices this step uses
    const int dst = right ? k - 1 : k;
    __syncthreads();
    for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {
      const double* p = cores + ((long long)(k - 1) * 2 * DD + i) * 2;
      Ar[i] = p[0];
      Ai[i] = p[1];
    }
    __syncthreads();
    for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {      // T_s = A_s X (A_s^T X)
      const int s = i / DD, a = (i % DD) / D, d = i % D;
      double tr = 0.0, ti = 0.0;
      for (int c = 0; c < D; ++c) {
        const int ia = right ? s * DD + a * D + c : s * DD + c * D + a;
        const double ar = Ar[ia], ai = Ai[ia], xr = Xr[c * D + d], xi = Xi[c * D + d];
        tr = fma(ar, xr, tr);
        tr = fma(-ai, xi, tr);
        ti = fma(ar, xi, ti);
        ti = fma(ai, xr, ti);
      }
      Tr[i] = tr;
      Ti[i] = ti;
    }
    __syncthreads();
    double vr = 0.0, vi = 0.0, mx = 0.0;
    if (t < DD) {
      const int a0 = t / D, b0 = t % D;
      const int a = a0 < b0 ? a0 : b0, b = a0 < b0 ? b0 : a0;
      for (int s = 0; s < 2; ++s)
        for (int d = 0; d < D; ++d) {
          const int ia = right ? s * DD + b * D + d : s * DD + d * D + b;
          const double ar = Ar[ia], ai = Ai[ia], tr = Tr[s * DD + a * D + d], ti = Ti[s * DD + a * D + d];
          vr = fma(tr, ar, vr);
          vr = fma(ti, ai, vr);
          vi = fma(ti, ar, vi);
          vi = fma(-tr, ai, vi);
        }
      if (a0 > b0) vi = 0.0 - vi;
      else if (a0 == b0) vi = 0.0;
      mx = fmax(fabs(vr), fabs(vi));
    }
    mx = wave_max(mx);
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    const int e = ms_exponent(mx);
    if (t < DD) {
      const double xr = ldexp(vr, -e), xi = ldexp(vi, -e);
      Xr[t] = xr;
      Xi[t] = xi;
      double* o = out + (long long)dst * 2 * DD;
      o[t] = xr;
      o[DD + t] = xi;
    }
    ex += e;
    if (t == 0) eo[dst] = ex;
  }
  __syncthreads();
  if (right && t == 0) {
    const double Zh = Xr[0];
    const double lz = log(Zh) + (double)ex * MS_LN2;
    hdr[0] = lz;
    hdr[1] = Zh;
    hdr[2] = (double)ex;
    if (logZ_out) logZ_out[0] = lz;
  }
}

// ---- lane vectors ------------------------------------------------------------------------------------------------
// A_k[s] zero-padded to DP x DP in LDS, re and im planes [s][a][b]; optionally the planes of a D x D matrix M [re, im][D][D]
template <int DP>
__device__ __forceinline__ void cm_load_site(const double* cores, int k, int D, double* Ar, double* Ai, const double* M, double* Mr,
                                             double* Mi) {
  const double* A = cores + (long long)(k - 1) * 4 * D * D;
  for (int i = threadIdx.x; i < 2 * DP * DP; i += MS_LANES) {
    const int s = i / (DP * DP), a = (i / DP) % DP, b = i % DP;
    const bool in = a < D && b < D;
    const int j = in ? ((s * D + a) * D + b) * 2 : 0;
    Ar[i] = in ? A[j] : 0.0;
    Ai[i] = in ? A[j + 1] : 0.0;
  }
  if (M)
    for (int i = threadIdx.x; i < DP * DP; i += MS_LANES) {
      const int a = i / DP, b = i % DP;
      const bool in = a < D && b < D;
      const int j = in ? a * D + b : 0;
      Mr[i] = in ? M[j] : 0.0;
      Mi[i] = in ? M[D * D + j] : 0.0;
    }
}

// v <- v 2^-e, e = ilogb of the largest |re| or |im|, returned
template <int DP>
__device__ __forceinline__ int cm_rescale(double (&vr)[DP], double (&vi)[DP]) {
  double mx = 0.0;
#pragma unroll
  for (int a = 0; a < DP; ++a) mx = fmax(mx, fmax(fabs(vr[a]), fabs(vi[a])));
  const int e = ms_exponent(mx);
#pragma unroll
  for (int a = 0; a < DP; ++a) {
    vr[a] = ldexp(vr[a], -e);
    vi[a] = ldexp(vi[a], -e);
  }
  return e;
}

// l <- l A, rescaled; A: the planes of one DP x DP matrix in LDS
template <int DP>
__device__ __forceinline__ int cm_left_step(double (&lr)[DP], double (&li)[DP], const double* Ar, const double* Ai) {
  double nr[DP], ni[DP];
#pragma unroll
  for (int c = 0; c < DP; ++c) {
    double xr = 0.0, xi = 0.0;
#pragma unroll
    for (int a = 0; a < DP; ++a) {
      const double ar = Ar[a * DP + c], ai = Ai[a * DP + c];
      xr = fma(lr[a], ar, xr);
      xr = fma(-li[a], ai, xr);
      xi = fma(lr[a], ai, xi);
      xi = fma(li[a], ar, xi);
    }
    nr[c] = xr;
    ni[c] = xi;
  }
#pragma unroll
  for (int a = 0; a < DP; ++a) {
    lr[a] = nr[a];
    li[a] = ni[a];
  }
  return cm_rescale<DP>(lr, li);
}

// r <- A r, rescaled
template <int DP>
__device__ __forceinline__ int cm_right_step(const double* Ar, const double* Ai, double (&rr)[DP], double (&ri)[DP]) {
  double nr[DP], ni[DP];
#pragma unroll
  for (int a = 0; a < DP; ++a) {
    double xr = 0.0, xi = 0.0;
#pragma unroll
    for (int c = 0; c < DP; ++c) {
      const double ar = Ar[a * DP + c], ai = Ai[a * DP + c];
      xr = fma(ar, rr[c], xr);
      xr = fma(-ai, ri[c], xr);
      xi = fma(ar, ri[c], xi);
      xi = fma(ai, rr[c], xi);
    }
    nr[a] = xr;
    ni[a] = xi;
  }
#pragma unroll
  for (int a = 0; a < DP; ++a) {
    rr[a] = nr[a];
    ri[a] = ni[a];
  }
  return cm_rescale<DP>(rr, ri);
}

// ---- sampler ---------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(MS_LANES) void cmps_sample_kernel(const double* __restrict__ cores, int n, int D, long long B,
                                                               const double* __restrict__ E, const double* __restrict__ hdr,
                                                               uint32_t seed_lo, uint32_t seed_hi,
                                                               const long long* __restrict__ epoch_dev, long long* __restrict__ idx,
                                                               double* __restrict__ logq, int* status) {
  __shared__ double Ar[2 * DP * DP], Ai[2 * DP * DP];
  __shared__ double Er[DP * DP], Ei[DP * DP];
  const long long b = (long long)blockIdx.x * MS_LANES + threadIdx.x;
  const bool active = b < B;
  const uint32_t ep = (uint32_t)(unsigned long long)(*epoch_dev);
  double lr[DP], li[DP];
  ms_fill<DP>(lr, 1.0);
  ms_fill<DP>(li, 0.0);
  int el = 0;
  unsigned long long z = 0;
  bool dead = false;
  uint4 w = make_uint4(0, 0, 0, 0);
#pragma unroll 1
  for (int k = 1; k <= n; ++k) {
    __syncthreads();
    cm_load_site<DP>(cores, k, D, Ar, Ai, E + (long long)k * 2 * D * D, Er, Ei);
    __syncthreads();
    if (k & 1) w = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)((k + 1) / 2 - 1), MS_PHILOX_DOMAIN, ep), seed_lo, seed_hi);
    const double U = (k & 1) ? unit53(w.x, w.y) : unit53(w.z, w.w);
    double u0r[DP], u0i[DP], u1r[DP], u1i[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) {
      double a0r = 0.0, a0i = 0.0, a1r = 0.0, a1i = 0.0;
#pragma unroll
      for (int a = 0; a < DP; ++a) {
        const double x0r = Ar[a * DP + c], x0i = Ai[a * DP + c], x1r = Ar[DP * DP + a * DP + c], x1i = Ai[DP * DP + a * DP + c];
        a0r = fma(lr[a], x0r, a0r);
        a1r = fma(lr[a], x1r, a1r);
        a0r = fma(-li[a], x0i, a0r);
        a1r = fma(-li[a], x1i, a1r);
        a0i = fma(lr[a], x0i, a0i);
        a1i = fma(lr[a], x1i, a1i);
        a0i = fma(li[a], x0r, a0i);
        a1i = fma(li[a], x1r, a1i);
      }
      u0r[c] = a0r;
      u0i[c] = a0i;
      u1r[c] = a1r;
      u1i[c] = a1i;
    }
    double m0 = 0.0, m1 = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      double t0r = 0.0, t0i = 0.0, t1r = 0.0, t1i = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) {
        const double er = Er[c * DP + d], ei = Ei[c * DP + d];
        t0r = fma(u0r[c], er, t0r);
        t1r = fma(u1r[c], er, t1r);
        t0r = fma(-u0i[c], ei, t0r);
        t1r = fma(-u1i[c], ei, t1r);
        t0i = fma(u0r[c], ei, t0i);
        t1i = fma(u1r[c], ei, t1i);
        t0i = fma(u0i[c], er, t0i);
        t1i = fma(u1i[c], er, t1i);
      }
      m0 = fma(t0r, u0r[d], m0);
      m1 = fma(t1r, u1r[d], m1);
      m0 = fma(t0i, u0i[d], m0);
      m1 = fma(t1i, u1i[d], m1);
    }
    const double tot = m0 + m1;
    if (!dead && !(tot > 0.0 && isfinite(tot))) {
      dead = true;
      if (active) *status = 1;
    }
    const bool bit = !dead && (U * tot >= m0);
    z = (z << 1) | (bit ? 1ull : 0ull);
#pragma unroll
    for (int a = 0; a < DP; ++a) {
      lr[a] = bit ? u1r[a] : u0r[a];
      li[a] = bit ? u1i[a] : u0i[a];
    }
    el += cm_rescale<DP>(lr, li);
  }
  if (active) {
    idx[b] = (long long)z;
    logq[b] = dead ? __builtin_nan("") : ms_logq(hypot(lr[0], li[0]), el, hdr[1], hdr[2]);
  }
}

// ---- score gradient --------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(MS_LANES) void cmps_score_kernel(const double* __restrict__ cores, int n, int D, long long B,
                                                              long long ntiles, const long long* __restrict__ idx,
                                                              const double* __restrict__ wgt, const double* __restrict__ hdr,
                                                              double* __restrict__ logq, int* status, double* rws, int* erws,
                                                              double* parts, double* __restrict__ wpart) {
  static_assert(DP <= 16, "one 16 x 16 tile per part");
  constexpr int XP = 17;                     // row pitch of X in LDS (odd: the lanes' rows start in different banks)
  __shared__ double Ar[2 * DP * DP], Ai[2 * DP * DP];
  __shared__ double Xr[MS_LANES * XP], Xi[MS_LANES * XP];
  __shared__ int Zs[MS_LANES];
  const int lane = threadIdx.x, fr = lane & 15, fk = lane >> 4;
  const int RS = 2 * D;                      // a sample's slot of the slice: re D | im D
  double* rsl = rws + (size_t)blockIdx.x * n * MS_LANES * RS;
  int* esl = erws + (size_t)blockIdx.x * n * MS_LANES;
  double* part = parts + (size_t)blockIdx.x * n * 4 * D * D;
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
    double rr[DP], ri[DP];
    ms_fill<DP>(rr, 1.0);
    ms_fill<DP>(ri, 0.0);
    int er0 = 0;
#pragma unroll 1
    for (int k = n; k >= 1; --k) {
      if (k < n) {
        double* dst = rsl + ((size_t)k * MS_LANES + lane) * RS;
#pragma unroll
        for (int a = 0; a < DP; ++a)
          if (a < D) {
            dst[a] = rr[a];
            dst[D + a] = ri[a];
          }
        esl[k * MS_LANES + lane] = er0;
      }
      __syncthreads();
      cm_load_site<DP>(cores, k, D, Ar, Ai, nullptr, nullptr, nullptr);
      __syncthreads();
      const int s = ms_bit(z, n, k);
      er0 += cm_right_step<DP>(Ar + s * DP * DP, Ai + s * DP * DP, rr, ri);
    }
    const double h = hypot(rr[0], ri[0]);
    const bool good = ms_amplitude_ok(h, Zok);
    if (active) {
      logq[b] = ms_logq(h, er0, Zh, eE0);
      if (!good) *status = 2;
    }
    // g = 2 w / r^_0[0] = (2 w / h) conj(r^_0[0] / h)
    const double gm = good ? (wv + wv) / h : 0.0;
    const double gr = good ? gm * (rr[0] / h) : 0.0;
    const double gi = good ? 0.0 - gm * (ri[0] / h) : 0.0;
    // left to right
    double lr[DP], li[DP];
    ms_fill<DP>(lr, 1.0);
    ms_fill<DP>(li, 0.0);
    int el = 0;
#pragma unroll 1
    for (int k = 1; k <= n; ++k) {
      __syncthreads();
      cm_load_site<DP>(cores, k, D, Ar, Ai, nullptr, nullptr, nullptr);
      const int s = ms_bit(z, n, k);
      const int erk = k < n ? esl[k * MS_LANES + lane] : 0;
      const int sh = el + erk - er0;
      const double cr = ldexp(gr, sh), ci = ldexp(gi, sh);
#pragma unroll
      for (int a = 0; a < DP; ++a) {
        Xr[lane * XP + a] = cr * lr[a] - ci * li[a];
        Xi[lane * XP + a] = cr * li[a] + ci * lr[a];
      }
      Zs[lane] = s;
      __syncthreads();
      cm_d4 accX[2], accY[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        accX[q] = (cm_d4){0.0, 0.0, 0.0, 0.0};
        accY[q] = (cm_d4){0.0, 0.0, 0.0, 0.0};
      }
#pragma unroll 4
      for (int kk = 0; kk < MS_LANES / 4; ++kk) {
        const int bb = 4 * kk + fk;
        const int sb = Zs[bb];
        const bool in = fr < D;
        const double xr = in ? Xr[bb * XP + fr] : 0.0;
        const double xi = in ? Xi[bb * XP + fr] : 0.0;
        double vr, vi;
        if (k < n) {
          const double* src = rsl + ((size_t)k * MS_LANES + bb) * RS;
          vr = in ? src[fr] : 0.0;
          vi = in ? src[D + fr] : 0.0;
        } else {
          vr = fr == 0 ? 1.0 : 0.0;
          vi = 0.0;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const double ar = sb == q ? xr : 0.0, ai = sb == q ? xi : 0.0;
          accX[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, vr, accX[q], 0, 0, 0);
          accX[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, vi, accX[q], 0, 0, 0);
          accY[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ar, vi, accY[q], 0, 0, 0);
          accY[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, vr, accY[q], 0, 0, 0);
        }
      }
      // D[row = fk + 4 i][col = fr]: entry (a = fk + 4 i, c = fr)
      double* pk = part + (size_t)(k - 1) * 4 * D * D;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ar = fk + 4 * i, bc = fr;
          if (ar < D && bc < D) {
            double* p = pk + ((q * D + ar) * D + bc) * 2;
            p[0] = first ? accX[q][i] : p[0] + accX[q][i];
            p[1] = first ? accY[q][i] : p[1] + accY[q][i];
          }
        }
      el += cm_left_step<DP>(lr, li, Ar + s * DP * DP, Ai + s * DP * DP);
    }
  }
  if (lane == 0) wpart[blockIdx.x] = wacc;
}

// grid n: grad[k - 1] = the workgroups' partials in order - (sum_b w_b) (2 Re G_k, -2 Im G_k)
__global__ __launch_bounds__(MS_ENV_THREADS) void cmps_score_finish_kernel(const double* __restrict__ cores, int n, int D, int G,
                                                                        const double* __restrict__ parts,
                                                                        const double* __restrict__ wpart, const double* __restrict__ E,
                                                                        const double* __restrict__ L, const int* __restrict__ eE,
                                                                        const int* __restrict__ eL, const double* __restrict__ hdr,
                                                                        double* __restrict__ grad) {
  __shared__ double Ar[2 * CM_DMAX * CM_DMAX], Ai[2 * CM_DMAX * CM_DMAX];
  __shared__ double Er[CM_DMAX * CM_DMAX], Ei[CM_DMAX * CM_DMAX];
  __shared__ double Lr[CM_DMAX * CM_DMAX], Li[CM_DMAX * CM_DMAX];
  __shared__ double Tr[2 * CM_DMAX * CM_DMAX], Ti[2 * CM_DMAX * CM_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  const int k = blockIdx.x + 1, t = threadIdx.x, DD = D * D;
  double wv = 0.0;
  for (int i = t; i < G; i += MS_ENV_THREADS) wv += wpart[i];
  wv = wave_sum(wv);
  if ((t & 63) == 0) red[t >> 6] = wv;
  for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {
    const double* p = cores + ((long long)(k - 1) * 2 * DD + i) * 2;
    Ar[i] = p[0];
    Ai[i] = p[1];
  }
  if (t < DD) {
    Er[t] = E[(long long)k * 2 * DD + t];
    Ei[t] = E[(long long)k * 2 * DD + DD + t];
    Lr[t] = L[(long long)(k - 1) * 2 * DD + t];
    Li[t] = L[(long long)(k - 1) * 2 * DD + DD + t];
  }
  __syncthreads();
  for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {      // T_s[a][c] = sum_c' conj(A_s[a][c']) E^[c][c']
    const int s = i / DD, a = (i % DD) / D, c = i % D;
    double tr = 0.0, ti = 0.0;
    for (int cc = 0; cc < D; ++cc) {
      const double ar = Ar[s * DD + a * D + cc], ai = Ai[s * DD + a * D + cc], er = Er[c * D + cc], ei = Ei[c * D + cc];
      tr = fma(ar, er, tr);
      tr = fma(ai, ei, tr);
      ti = fma(ar, ei, ti);
      ti = fma(-ai, er, ti);
    }
    Tr[i] = tr;
    Ti[i] = ti;
  }
  __syncthreads();
  const double W = ((red[0] + red[1]) + red[2]) + red[3];
  const int ex = eL[k - 1] + eE[k] - eE[0];
  const double Zh = hdr[1];
  const size_t stride = (size_t)n * 4 * DD;
  for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {      // M_s[a][c] = sum_a' L^[a][a'] T_s[a'][c]
    const int s = i / DD, a = (i % DD) / D, c = i % D;
    double mr = 0.0, mi = 0.0;
    for (int aa = 0; aa < D; ++aa) {
      const double lr = Lr[a * D + aa], li = Li[a * D + aa], tr = Tr[s * DD + aa * D + c], ti = Ti[s * DD + aa * D + c];
      mr = fma(lr, tr, mr);
      mr = fma(-li, ti, mr);
      mi = fma(lr, ti, mi);
      mi = fma(li, tr, mi);
    }
    const double envr = ldexp(mr / Zh, ex), envi = ldexp(mi / Zh, ex);
    double sr = 0.0, si = 0.0;
    const double* p = parts + ((size_t)(k - 1) * 2 * DD + i) * 2;
    for (int g = 0; g < G; ++g) {
      sr += p[g * stride];
      si += p[g * stride + 1];
    }
    double* o = grad + ((size_t)(k - 1) * 2 * DD + i) * 2;
    o[0] = sr - W * (envr + envr);
    o[1] = si + W * (envi + envi);
  }
}

}  // namespace

size_t cmps_workspace_bytes(int n, int D, long long B) { return cm_layout(n, D, B).total + 256; }

hipError_t launch_cmps_environments(int n, int D, long long B, const double* cores, double* logZ_out, void* ws, hipStream_t st) {
  const CmLayout S = cm_layout(n, D, B);
  char* base = ws_align(ws);
  cmps_env_kernel<<<2, MS_ENV_THREADS, 0, st>>>(cores, n, D, (double*)(base + S.E), (double*)(base + S.L), (int*)(base + S.eE),
                                            (int*)(base + S.eL), (double*)(base + S.hdr), logZ_out);
  return hipGetLastError();
}

// CALL with `DP` a constant expression equal to DPV (= bond_dp(D) <= 16)
#define CMPS_DISPATCH(DPV, CALL)                      \
  switch (DPV) {                                      \
    case 2: { constexpr int DP = 2; CALL; } break;    \
    case 4: { constexpr int DP = 4; CALL; } break;    \
    case 8: { constexpr int DP = 8; CALL; } break;    \
    default: { constexpr int DP = 16; CALL; } break;  \
  }

hipError_t launch_cmps_sample(int n, int D, long long B, const double* cores, unsigned long long seed, const long long* epoch_dev,
                              long long* idx, double* logq, int* status, void* ws, hipStream_t st) {
  const CmLayout S = cm_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((B + MS_LANES - 1) / MS_LANES);
  CMPS_DISPATCH(S.DP, (cmps_sample_kernel<DP><<<grid, MS_LANES, 0, st>>>(cores, n, D, B, (const double*)(base + S.E),
                                                                       (const double*)(base + S.hdr), (uint32_t)seed,
                                                                       (uint32_t)(seed >> 32), epoch_dev, idx, logq, status)));
  return hipGetLastError();
}

hipError_t launch_cmps_score_vjp(int n, int D, long long B, const double* cores, const long long* idx, const double* w, double* logq,
                                 double* grad_cores, int* status, void* ws, hipStream_t st) {
  const CmLayout S = cm_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const long long ntiles = (B + MS_LANES - 1) / MS_LANES;
  CMPS_DISPATCH(S.DP, (cmps_score_kernel<DP><<<(unsigned)S.G, MS_LANES, 0, st>>>(
                        cores, n, D, B, ntiles, idx, w, (const double*)(base + S.hdr), logq, status, (double*)(base + S.r),
                        (int*)(base + S.er), (double*)(base + S.parts), (double*)(base + S.wpart))));
  cmps_score_finish_kernel<<<(unsigned)n, MS_ENV_THREADS, 0, st>>>(cores, n, D, S.G, (const double*)(base + S.parts),
                                                               (const double*)(base + S.wpart), (const double*)(base + S.E),
                                                               (const double*)(base + S.L), (const int*)(base + S.eE),
                                                               (const int*)(base + S.eL), (const double*)(base + S.hdr), grad_cores);
  return hipGetLastError();
}

}  // namespace bornvi
