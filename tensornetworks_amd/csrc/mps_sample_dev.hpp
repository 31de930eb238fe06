// The sampled-MPS kernels' one definition of their site sweeps (kernels_mps_sample.hip, kernels_mps_sample_gram.hip), so that
// l^, r^, their exponents and mu are the same bits in every kernel because they are the same code.
//
// Vectors: one sample per lane, DP doubles (DP = ms_dp(D) = 2, 4, 8, 16, 32 >= D, zero padded) in registers; a site's matrices
//   A_k[0], A_k[1] zero-padded to DP x DP in LDS (ms_load_site) and read as broadcasts.  z_k is bit n - k of the index word.
// Products: an entry of x A (ms_row_dot) or of A r (ms_dot_col) is one fma chain in index order that continues from the
//   accumulator it is given; the left and right steps are built on them.  Two kernels write this chain out themselves,
//   because each runs two chains in one loop with their terms alternating, around one shared load: the sampler (u_0 and
//   u_1 share l[a]) and the jvp (l A and dl A share the entry of A).  Routed through ms_row_dot they give the same bits
//   but are slower (profiles/sampled_sweep_core_variants.jsonl).
// Steps: l <- l A_k[z_k] (ms_left_step), r <- A_k[z_k] r (ms_right_step); the new vector is taken times 2^-e (ms_take), e =
//   ilogb of its largest magnitude (exact; ms_rescale), e returned:  true l_k = l^_k 2^el_k, true r_k = r^_k 2^er_k, el, er
//   the sums of the e's.
// Right-to-left sweep (ms_right_sweep): r^_n = e0, er_n = 0; for k = n .. 1 the caller's store gets (k, r^_k, er_k), the
//   workgroup loads site k, and the lane steps.  Leaves r^_0 and returns er_0:  psi = r^_0[0] 2^er_0.
// Amplitude (ms_norm_ok, ms_amplitude_ok, ms_site_factor): a sample counts when r^_0[0] is finite and not 0 and E^_0[0, 0] is
//   finite and positive; its factor at site k is g 2^(el_{k-1} + er_k - er_0), g = 2 w_b / r^_0[0] or 2 / r^_0[0] (0 when it does not count).
//   log q = 2 log|psi| - log Z with the exponents kept apart (ms_logq).
// Environment term (ms_env_stage, ms_env_entry; a workgroup of MS_ENV_THREADS per site): mu[k - 1][s][a][d] =
//   2 (L_{k-1} A_k[s] E_k)[a][d] / Z as T_s = A_s E^_k, M_s = L^_{k-1} T_s, fma chains in index order through LDS, then
//   2^(eL[k-1] + eE[k] - eE[0]) / E^_0[0, 0].
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace bornvi {

constexpr int MS_LANES = 64;               // sampler, score and Gram-vector kernels: one wave per workgroup
constexpr int MS_ENV_THREADS = 256;        // environment kernels: one workgroup per site (or per direction)
constexpr int MS_DMAX = 32;
constexpr double MS_LN2 = 0.693147180559945309417232121458;

inline int ms_dp(int D) { return D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }

#define MS_DISPATCH(DPV, CALL)                        \
  switch (DPV) {                                      \
    case 2: { constexpr int DP = 2; CALL; } break;    \
    case 4: { constexpr int DP = 4; CALL; } break;    \
    case 8: { constexpr int DP = 8; CALL; } break;    \
    case 16: { constexpr int DP = 16; CALL; } break;  \
    default: { constexpr int DP = 32; CALL; } break;  \
  }

__device__ __forceinline__ double ms_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// exponent of the exact power-of-two rescaling: ilogb of a positive finite largest magnitude, else 0 (nothing to rescale)
__device__ __forceinline__ int ms_exponent(double mx) { return (mx > 0.0 && isfinite(mx)) ? ilogb(mx) : 0; }

template <int DP>
__device__ __forceinline__ int ms_rescale(double (&v)[DP]) {
  double mx = 0.0;
#pragma unroll
  for (int a = 0; a < DP; ++a) mx = fmax(mx, fabs(v[a]));
  const int e = ms_exponent(mx);
#pragma unroll
  for (int a = 0; a < DP; ++a) v[a] = ldexp(v[a], -e);
  return e;
}

// A_k[s] zero-padded to DP x DP in LDS, As[s][a][b]; optionally a D x D matrix M the same way
template <int DP>
__device__ __forceinline__ void ms_load_site(const double* cores, int k, int D, double* As, const double* M, double* Ms) {
  const double* A = cores + (long long)(k - 1) * 2 * D * D;
  for (int i = threadIdx.x; i < 2 * DP * DP; i += MS_LANES) {
    const int s = i / (DP * DP), a = (i / DP) % DP, b = i % DP;
    As[i] = (a < D && b < D) ? A[(s * D + a) * D + b] : 0.0;
  }
  if (M)
    for (int i = threadIdx.x; i < DP * DP; i += MS_LANES) {
      const int a = i / DP, b = i % DP;
      Ms[i] = (a < D && b < D) ? M[a * D + b] : 0.0;
    }
}

__device__ __forceinline__ int ms_bit(unsigned long long z, int n, int k) { return (int)((z >> (n - k)) & 1ull); }

// v = (first, 0, ..., 0): e0 where a sweep starts, 0 for a tangent
template <int DP>
__device__ __forceinline__ void ms_fill(double (&v)[DP], double first) {
#pragma unroll
  for (int a = 0; a < DP; ++a) v[a] = a == 0 ? first : 0.0;
}

// acc + sum_a x[a] A[a][c]: entry c of x A
template <int DP>
__device__ __forceinline__ double ms_row_dot(const double (&x)[DP], const double* A, int c, double acc) {
#pragma unroll
  for (int a = 0; a < DP; ++a) acc = fma(x[a], A[a * DP + c], acc);
  return acc;
}

// acc + sum_c A[a][c] r[c]: entry a of A r
template <int DP>
__device__ __forceinline__ double ms_dot_col(const double* A, int a, const double (&r)[DP], double acc) {
#pragma unroll
  for (int c = 0; c < DP; ++c) acc = fma(A[a * DP + c], r[c], acc);
  return acc;
}

// v <- vn 2^-e, e returned
template <int DP>
__device__ __forceinline__ int ms_take(double (&v)[DP], const double (&vn)[DP]) {
#pragma unroll
  for (int a = 0; a < DP; ++a) v[a] = vn[a];
  return ms_rescale<DP>(v);
}

template <int DP>
__device__ __forceinline__ int ms_left_step(double (&l)[DP], const double* A) {
  double ln[DP];
#pragma unroll
  for (int c = 0; c < DP; ++c) ln[c] = ms_row_dot<DP>(l, A, c, 0.0);
  return ms_take<DP>(l, ln);
}

template <int DP>
__device__ __forceinline__ int ms_right_step(const double* A, double (&r)[DP]) {
  double rn[DP];
#pragma unroll
  for (int a = 0; a < DP; ++a) rn[a] = ms_dot_col<DP>(A, a, r, 0.0);
  return ms_take<DP>(r, rn);
}

// store(k, r^_k, er_k) for k = n .. 1, each before site k is loaded into As (2 DP DP doubles of LDS) and stepped over
template <int DP, class Store>
__device__ __forceinline__ int ms_right_sweep(const double* cores, int n, int D, unsigned long long z, double* As, double (&r)[DP],
                                              Store&& store) {
  ms_fill<DP>(r, 1.0);
  int er = 0;
#pragma unroll 1
  for (int k = n; k >= 1; --k) {
    store(k, r, er);
    __syncthreads();
    ms_load_site<DP>(cores, k, D, As, nullptr, nullptr);
    __syncthreads();
    er += ms_right_step<DP>(As + ms_bit(z, n, k) * DP * DP, r);
  }
  return er;
}

__device__ __forceinline__ bool ms_norm_ok(double Zh) { return Zh > 0.0 && isfinite(Zh); }      // once per kernel
__device__ __forceinline__ bool ms_amplitude_ok(double a0, bool Zok) { return a0 != 0.0 && isfinite(a0) && Zok; }
__device__ __forceinline__ double ms_site_factor(double g, int el, int erk, int er0) { return ldexp(g, el + erk - er0); }
// a0 2^e the amplitude, Zh 2^eE0 = Z
__device__ __forceinline__ double ms_logq(double a0, int e, double Zh, double eE0) {
  return (2.0 * log(fabs(a0)) - log(Zh)) + (2.0 * (double)e - eE0) * MS_LN2;
}

// site k's A (as stored, pitch D), E^_k, L^_{k-1} into LDS and T[s][c][d] = sum_e A[s][c][e] E^_k[e][d]; ends on a barrier
__device__ __forceinline__ void ms_env_stage(const double* cores, int k, int D, const double* E, const double* L, double* As, double* Em,
                                             double* Lm, double* T) {
  const int t = threadIdx.x, DD = D * D;
  for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) As[i] = cores[(long long)(k - 1) * 2 * DD + i];
  for (int i = t; i < DD; i += MS_ENV_THREADS) {
    Em[i] = E[(long long)k * DD + i];
    Lm[i] = L[(long long)(k - 1) * DD + i];
  }
  __syncthreads();
  for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {
    const int s = i / DD, c = (i % DD) / D, d = i % D;
    double acc = 0.0;
    for (int e = 0; e < D; ++e) acc = fma(As[s * DD + c * D + e], Em[e * D + d], acc);
    T[i] = acc;
  }
  __syncthreads();
}

// entry i = (s D + a) D + d of mu[k - 1], after ms_env_stage; ex = eL[k - 1] + eE[k] - eE[0], Zh = E^_0[0, 0]
__device__ __forceinline__ double ms_env_entry(const double* Lm, const double* T, int D, int i, double Zh, int ex) {
  const int DD = D * D, s = i / DD, a = (i % DD) / D, d = i % D;
  double m = 0.0;
  for (int c = 0; c < D; ++c) m = fma(Lm[a * D + c], T[s * DD + c * D + d], m);
  const double env = ldexp(m / Zh, ex);
  return env + env;
}

}  // namespace bornvi
