// Sample-space Gram of the sampled MPS Born machine's score rows: T = O O^T / B for the B x P matrix O
// of centred score rows o_b (kernels_mps_sample.hip, bornvi_mps_score_rows), without ever forming a row.  o_b = t_b - mu with
// t_b a sum over the sites of rank-one terms at [k, z_bk], so
//   B T_bb' = sum_k [z_bk = z_b'k] (x_bk . x_b'k)(r_bk . r_b'k) - m_b - m_b' + M,
//   x_bk = (2 / psi_b) l_{b,k-1},   m_b = sum_k x_bk^T mu_k[z_bk] r_bk,   M = sum_{k,s} ||mu_k[s]||_F^2.
//
// bornvi_mps_score_sample_gram = the status word's clear (launch_ms_clear_status) + mps_score_mu_kernel (kernels_mps_sample.hip,
// into the mu region of the environments' workspace) + three kernels; l^, r^, their exponents and the site factor are
// mps_sample_dev.hpp's:
//   mps_gram_vectors_kernel<DP>: one sample per lane, one wave per workgroup, workgroup g owns the samples 64 g .. 64 g + 63.
//     ms_right_sweep stores r^_k (k = n: e0) and its exponent er_k for every site; the left-to-right sweep (ms_left_step)
//     keeps l^ in registers and stores x^_bk = cf l^_{k-1}, cf = ms_site_factor with g = 2 / r^_0[0], and adds the site's m
//     term: one fma chain over (a, c) of (x^[a] r^[c]) mu[s][a][c], the sites added in order.  Layout of both vector sets:
//     [site][fragment of 16 samples][component, D4 = D rounded up to 4, zero padded][sample in the fragment]: step j of a
//     16-sample fragment is 64 consecutive doubles, lane (fr, fk) reading component 4 j + fk of sample fr, which is what
//     v_mfma_f64_16x16x4_f64 takes as A and as B without a transpose.
//     A sample that fails ms_amplitude_ok gets zero vectors, m_b = 0, alive = 0 and sets the status word to 2; so do the
//     padding samples B .. 64 ceil(B / 64) - 1 (without the status).
//   mps_gram_mu_norm_kernel: M, one workgroup; lane t squares the entries t, t + 256, ... in one fma chain, then wave_sum
//     over the 64 lanes and the four waves in order.
//   mps_sample_gram_kernel: one wave per 32 x 32 tile on or above the diagonal (2 x 2 fragments).  Per site the wave forms the
//     two dot-product tiles x . x' and r . r' of every fragment pair on the matrix cores (D4 / 4 steps each, components in
//     order), multiplies them entry by entry and adds the product with one fma into the entry's sum when bit n - k of
//     idx[b] ^ idx[b'] is clear; sites in order.  Then T_bb' = (((acc - m_b) - m_b') + M) / B for b <= b', stored at [b][b']
//     and at [b'][b]; 0.0 where either sample is not alive.  The row sample is always the A operand and b <= b', so an entry's
//     bits depend on (n, D, cores, the two samples) and on B through that one division only: not on the tile or the grid.
//
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "mps_sample_dev.hpp"

namespace bornvi {

namespace {
constexpr int SG_LANES = MS_LANES;          // one sample per lane, one wave per workgroup
constexpr int SG_FRAG = 16;                // samples of one matrix-core fragment
constexpr int SG_NORM_THREADS = 256;

typedef double sg_d4 __attribute__((ext_vector_type(4)));

struct SgLayout {
  int DP, D4, nfrag, ntile;                // ntile: 32-sample tiles that hold a sample < B
  long long Bp;                            // B rounded up to 64
  size_t x, r, er, m, alive, M, total;     // byte offsets from the aligned base
};

SgLayout sg_layout(int n, int D, long long B) {
  SgLayout S;
  S.DP = bond_dp(D);
  S.D4 = (D + 3) & ~3;
  S.Bp = (B + SG_LANES - 1) / SG_LANES * SG_LANES;
  S.nfrag = (int)(S.Bp / SG_FRAG);
  S.ntile = (int)((B + 31) / 32);
  size_t o = 0;
  S.x = o;     o += ws_round((size_t)n * S.Bp * S.D4 * sizeof(double));
  S.r = o;     o += ws_round((size_t)n * S.Bp * S.D4 * sizeof(double));
  S.er = o;    o += ws_round((size_t)n * S.Bp * sizeof(int));
  S.m = o;     o += ws_round((size_t)S.Bp * sizeof(double));
  S.alive = o; o += ws_round((size_t)S.Bp * sizeof(int));
  S.M = o;     o += 256;
  S.total = o;
  return S;
}

// component a of a stored vector: v[a] below DP, the zero padding from DP up to D4 (only DP = 2 has D4 = 4 > DP)
template <int DP>
__device__ __forceinline__ double sg_component(const double (&v)[DP], int a) { return a < DP ? v[a] : 0.0; }

// ---- vectors ---------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(SG_LANES) void mps_gram_vectors_kernel(const double* __restrict__ cores, int n, int D, int D4, long long B,
                                                                    long long Bp, const long long* __restrict__ idx,
                                                                    const double* __restrict__ hdr, const double* __restrict__ mu,
                                                                    double* xv, double* rv, int* erw, double* __restrict__ mv,
                                                                    int* __restrict__ alive, int* status) {
  constexpr int DV = DP < 4 ? 4 : DP;        // D4 <= DV
  __shared__ double As[2 * DP * DP];
  __shared__ double Mu[2 * DP * DP];         // mu[k] as stored: [s][a][c] with pitch D
  const int lane = threadIdx.x, R = 2 * D * D;
  const long long b = (long long)blockIdx.x * SG_LANES + lane;      // b < Bp
  const bool active = b < B;
  const unsigned long long z = active ? (unsigned long long)idx[b] : 0ull;
  const size_t site = (size_t)Bp * D4;                               // doubles of one site's vectors
  const size_t at = (size_t)(b / SG_FRAG) * D4 * SG_FRAG + (size_t)(b % SG_FRAG);
  const bool Zok = ms_norm_ok(hdr[1]);
  // right to left: r^_k and er_k of every site k = n .. 1 in the fragment layout
  double r[DP];
  const int er0 = ms_right_sweep<DP>(cores, n, D, z, As, r, [&](int k, const double (&rk)[DP], int er) {
    double* dst = rv + (size_t)(k - 1) * site + at;
#pragma unroll
    for (int a = 0; a < DV; ++a)
      if (a < D4) dst[a * SG_FRAG] = sg_component<DP>(rk, a);
    erw[(size_t)(k - 1) * Bp + b] = er;
  });
  const double r0 = r[0];
  const bool good = active && ms_amplitude_ok(r0, Zok);
  if (active && !good) *status = 2;
  const double g = good ? 2.0 / r0 : 0.0;
  // left to right
  double l[DP];
  ms_fill<DP>(l, 1.0);
  int el = 0;
  double m = 0.0;
#pragma unroll 1
  for (int k = 1; k <= n; ++k) {
    __syncthreads();
    ms_load_site<DP>(cores, k, D, As, nullptr, nullptr);
    for (int i = lane; i < R; i += SG_LANES) Mu[i] = mu[(size_t)(k - 1) * R + i];
    __syncthreads();
    const int s = ms_bit(z, n, k);
    const double cf = ms_site_factor(g, el, erw[(size_t)(k - 1) * Bp + b], er0);
    double* xd = xv + (size_t)(k - 1) * site + at;
    double* rd = rv + (size_t)(k - 1) * site + at;
    double rr[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) rr[c] = (good && c < D) ? rd[c * SG_FRAG] : 0.0;
    if (!good) {
#pragma unroll
      for (int a = 0; a < DV; ++a)
        if (a < D4) rd[a * SG_FRAG] = 0.0;
    }
    const double* Ms = Mu + s * D * D;
    double ms = 0.0;
#pragma unroll
    for (int a = 0; a < DV; ++a) {
      const double xa = good ? cf * sg_component<DP>(l, a) : 0.0;
      if (a < D4) xd[a * SG_FRAG] = xa;
      if (a < D) {
#pragma unroll
        for (int c = 0; c < DP; ++c)
          if (c < D) ms = fma(xa * rr[c], Ms[a * D + c], ms);
      }
    }
    m += ms;
    el += ms_left_step<DP>(l, As + s * DP * DP);
  }
  mv[b] = good ? m : 0.0;
  alive[b] = good ? 1 : 0;
}

// ---- M = sum mu^2 ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_NORM_THREADS) void mps_gram_mu_norm_kernel(const double* __restrict__ mu, int count,
                                                                           double* __restrict__ M) {
  __shared__ double red[SG_NORM_THREADS / 64];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < count; i += SG_NORM_THREADS) acc = fma(mu[i], mu[i], acc);
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) M[0] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- Gram ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_LANES) void mps_sample_gram_kernel(int n, int D4, long long B, int nfrag, int ntile,
                                                                   const long long* __restrict__ idx, const double* __restrict__ xv,
                                                                   const double* __restrict__ rv, const double* __restrict__ mv,
                                                                   const int* __restrict__ alive, const double* __restrict__ Mp,
                                                                   double* __restrict__ T) {
  const int lane = threadIdx.x, fr = lane & 15, fk = lane >> 4;
  // tile (ti, tj), ti <= tj, of the upper triangle in row order
  int ti = 0, rest = (int)blockIdx.x;
  while (rest >= ntile - ti) {
    rest -= ntile - ti;
    ++ti;
  }
  const int tj = ti + rest;
  // D[row = fk + 4 i][col = fr]: the row samples of fragment p are 32 ti + 16 p + fk + 4 i, the column sample of fragment q
  // is 32 tj + 16 q + fr
  unsigned long long zx[2][2][4];
  {
    unsigned long long zc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const long long bc = 32ll * tj + 16 * q + fr;
      zc[q] = bc < B ? (unsigned long long)idx[bc] : 0ull;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long br = 32ll * ti + 16 * p + fk + 4 * i;
        const unsigned long long zr = br < B ? (unsigned long long)idx[br] : 0ull;
#pragma unroll
        for (int q = 0; q < 2; ++q) zx[p][q][i] = zr ^ zc[q];
      }
  }
  sg_d4 tot[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) tot[p][q] = (sg_d4){0.0, 0.0, 0.0, 0.0};
  const int steps = D4 / 4;
  const size_t fstride = (size_t)D4 * SG_FRAG, sstride = (size_t)nfrag * fstride;
  const size_t rowoff[2] = {(size_t)(2 * ti) * fstride, (size_t)(2 * ti + 1) * fstride};     // 2 t + 1 < nfrag: nfrag is a
  const size_t coloff[2] = {(size_t)(2 * tj) * fstride, (size_t)(2 * tj + 1) * fstride};     // multiple of 4, 32 t < B <= 16 nfrag
#pragma unroll 1
  for (int k = 1; k <= n; ++k) {
    const double* xs = xv + (size_t)(k - 1) * sstride;
    const double* rs = rv + (size_t)(k - 1) * sstride;
    sg_d4 ax[2][2], ar[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q) ax[p][q] = ar[p][q] = (sg_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int j = 0; j < steps; ++j) {
      const size_t off = (size_t)(4 * j + fk) * SG_FRAG + fr;
      double xa[2], xb[2], ra[2], rb[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        xa[p] = xs[rowoff[p] + off];
        ra[p] = rs[rowoff[p] + off];
        xb[p] = xs[coloff[p] + off];
        rb[p] = rs[coloff[p] + off];
      }
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          ax[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[p], xb[q], ax[p][q], 0, 0, 0);
          ar[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[p], rb[q], ar[p][q], 0, 0, 0);
        }
    }
    const int bit = n - k;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!((zx[p][q][i] >> bit) & 1ull)) tot[p][q][i] = fma(ax[p][q][i], ar[p][q][i], tot[p][q][i]);
  }
  const double M = Mp[0], den = (double)B;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const long long bc = 32ll * tj + 16 * q + fr;
    if (bc >= B) continue;
    const double mc = mv[bc];
    const bool okc = alive[bc] != 0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long br = 32ll * ti + 16 * p + fk + 4 * i;
        if (br > bc) continue;                                   // br <= bc < B
        const double v = (okc && alive[br] != 0) ? (((tot[p][q][i] - mv[br]) - mc) + M) / den : 0.0;
        T[br * B + bc] = v;
        T[bc * B + br] = v;
      }
  }
}

}  // namespace

size_t mps_sample_gram_workspace_bytes(int n, int D, long long B) { return sg_layout(n, D, B).total + 256; }

hipError_t launch_mps_score_sample_gram(int n, int D, long long B, const double* cores, const long long* idx, double* T, int* status,
                                        void* env_ws, void* ws, hipStream_t st) {
  const SgLayout S = sg_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const double* hdr = nullptr;
  const double* mu = nullptr;
  e = launch_mps_score_mu(n, D, B, cores, env_ws, &hdr, &mu, st);
  if (e != hipSuccess) return e;
  double* xv = (double*)(base + S.x);
  double* rv = (double*)(base + S.r);
  BOND_DISPATCH(S.DP, (mps_gram_vectors_kernel<DP><<<(unsigned)(S.Bp / SG_LANES), SG_LANES, 0, st>>>(
                        cores, n, D, S.D4, B, S.Bp, idx, hdr, mu, xv, rv, (int*)(base + S.er), (double*)(base + S.m),
                        (int*)(base + S.alive), status)));
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mps_gram_mu_norm_kernel<<<1, SG_NORM_THREADS, 0, st>>>(mu, n * 2 * D * D, (double*)(base + S.M));
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mps_sample_gram_kernel<<<(unsigned)(S.ntile * (S.ntile + 1) / 2), SG_LANES, 0, st>>>(
      n, S.D4, B, S.nfrag, S.ntile, idx, xv, rv, (const double*)(base + S.m), (const int*)(base + S.alive),
      (const double*)(base + S.M), T);
  return hipGetLastError();
}

}  // namespace bornvi
