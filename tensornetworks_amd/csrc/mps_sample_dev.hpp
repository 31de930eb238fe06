// The sampled-MPS kernels' one definition of their site sweeps (kernels_mps_sample.hip, _sample_gram.hip, _query.hip), so that
// l^, r^, the environments, their exponents and mu are the same bits in every kernel because they are the same code.
//
// Wave sums and maxima, the padded bond dimension and its dispatch macro come from reduce_dev.hpp.
//
// Vectors: one sample per lane, DP doubles (DP = bond_dp(D) = 2, 4, 8, 16, 32 >= D, zero padded) in registers; a site's matrices
//   A_k[0], A_k[1] zero-padded to DP x DP in LDS (ms_load_site) and read as broadcasts.  z_k is bit n - k of the index word.
// Products: an entry of x A (ms_row_dot) or of A r (ms_dot_col) is one fma chain in index order that continues from the
//   accumulator it is given; the left and right steps are built on them.  Two kernels write this chain out themselves,
//   because each runs two chains in one loop with their terms alternating, around one shared load: the sampler's sweep (u_0 and
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
// Workgroup level (MS_ENV_THREADS threads, D x D matrices of pitch D in LDS): ms_allowed, the s allowed at site k under an evidence
//   as bits (3: free);  ms_load_site_wg;  ms_mul_AX: T[s] = A[s] X for the allowed s, and ms_env_chain: entry (s D + a) D + d of L T[s],
//   one fma chain in index order each.  ms_mul_AX takes s = [i >= D D], the others divide i by D D: the same indices, each form the
//   one at which its callers meet their timings (profiles/mps_env_core_isa.txt).
// Environment term (ms_env_stage, ms_env_entry; one workgroup per site): mu[k - 1][s][a][d] = 2 (L_{k-1} A_k[s] E_k)[a][d] / Z
//   as T_s = A_s E^_k (ms_mul_AX), M_s = L^_{k-1} T_s (ms_env_chain), then 2^(eL[k-1] + eE[k] - eE[0]) / E^_0[0, 0].
// Environment step (ms_env_step): X <- sum_s A[s] X A[s]^T (right) or sum_s A[s]^T X A[s] (left) over the ALLOWED s, as T_s = A_s X
//   (A_s^T X), X' = sum_s T_s A_s^T (T_s A_s), each entry one fma chain in index order (c, then s outer / d inner), then times 2^-e.
//   T_s is ms_mul_AX on the right where `right` is a literal, and one loop with a select where it is a run-time value (ANY_DIR,
//   mps_env_kernel): split, that kernel misses its timing, and unsplit the literal callers miss theirs (mps_env_core_isa.txt).
// Environment sweep (ms_env_sweep): X = e0 e0^T (slot n, exponent 0); for k = n .. 1 the workgroup loads site k and steps (right) with
//   allowed_of(k) into slot k - 1 of `out` (the stack, or null); store(slot, exponent sum) runs in every thread.  The clamped sweeps of
//   kernels_mps_query.hip; mps_env_kernel, either direction by a run-time choice, keeps its own loop.
// Sampler sweep (ms_sample_sweep): the site loop of bornvi_mps_sample, stated in kernels_mps_sample.hip, and with CLAMP the
//   same loop under an evidence (mask, value): a clamped site takes the evidence's bit and ignores U_k.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "philox_dev.hpp"
#include "reduce_dev.hpp"

namespace bornvi {

constexpr int MS_LANES = 64;               // sampler, score and Gram-vector kernels: one wave per workgroup
constexpr int MS_ENV_THREADS = 256;        // environment kernels: one workgroup per site (or per direction)
constexpr int MS_DMAX = 32;
constexpr double MS_LN2 = 0.693147180559945309417232121458;

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
__device__ __forceinline__ int ms_allowed(unsigned long long mask, unsigned long long value, int n, int k) {
  return ms_bit(mask, n, k) ? 1 << ms_bit(value, n, k) : 3;
}
__device__ __forceinline__ void ms_load_site_wg(const double* cores, int k, int D, double* As) {
  for (int DD = D * D, i = threadIdx.x; i < 2 * DD; i += MS_ENV_THREADS) As[i] = cores[(long long)(k - 1) * 2 * DD + i];
}
__device__ __forceinline__ void ms_mul_AX(int D, int allowed, const double* As, const double* X, double* T) {      // T: the caller's next barrier
  for (int DD = D * D, i = threadIdx.x; i < 2 * DD; i += MS_ENV_THREADS) {
    const int s = i >= DD, r = i - s * DD, a = r / D, d = r % D;      // s is 0 or 1: a literal allowed = 3 leaves no test behind
    if (!((allowed >> s) & 1)) continue;
    double acc = 0.0;
    for (int c = 0; c < D; ++c) acc = fma(As[s * DD + a * D + c], X[c * D + d], acc);
    T[i] = acc;
  }
}
__device__ __forceinline__ double ms_env_chain(const double* Lm, const double* T, int D, int i) {
  const int DD = D * D, s = i / DD, a = (i % DD) / D, d = i % D;
  double m = 0.0;
  for (int c = 0; c < D; ++c) m = fma(Lm[a * D + c], T[s * DD + c * D + d], m);
  return m;
}
// site k's A, E^_k, L^_{k-1} into LDS and T[s] = A[s] E^_k; ends on a barrier
__device__ __forceinline__ void ms_env_stage(const double* cores, int k, int D, const double* E, const double* L, double* As, double* Em,
                                             double* Lm, double* T) {
  const int DD = D * D, t = threadIdx.x;
  ms_load_site_wg(cores, k, D, As);
  for (int i = t; i < DD; i += MS_ENV_THREADS) {
    Em[i] = E[(long long)k * DD + i];
    Lm[i] = L[(long long)(k - 1) * DD + i];
  }
  __syncthreads();
  ms_mul_AX(D, 3, As, Em, T);
  __syncthreads();
}

// entry i = (s D + a) D + d of mu[k - 1], after ms_env_stage; ex = eL[k - 1] + eE[k] - eE[0], Zh = E^_0[0, 0]
__device__ __forceinline__ double ms_env_entry(const double* Lm, const double* T, int D, int i, double Zh, int ex) {
  const double env = ldexp(ms_env_chain(Lm, T, D, i) / Zh, ex);
  return env + env;
}

// As, X in LDS, published by a barrier; T (2 D D), red (one a wave): scratch.  The new X, times 2^-e, goes to out too where not null; e returned.
template <bool ANY_DIR = false>
__device__ __forceinline__ int ms_env_step(bool right, int D, int allowed, const double* As, double* X, double* T, double* red,
                                           double* out) {
  const int DD = D * D, t = threadIdx.x;
  if (!ANY_DIR && right) ms_mul_AX(D, allowed, As, X, T);
  else
    for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {      // T_s = A_s^T X (A_s X)
      const int s = i / DD, a = (i % DD) / D, d = i % D;
      if (!((allowed >> s) & 1)) continue;
      double acc = 0.0;
      for (int c = 0; c < D; ++c) acc = fma(right ? As[s * DD + a * D + c] : As[s * DD + c * D + a], X[c * D + d], acc);
      T[i] = acc;
    }
  __syncthreads();
  double v[4];
  double mx = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = t + MS_ENV_THREADS * j;
    v[j] = 0.0;
    if (i < DD) {
      const int a = i / D, b = i % D;
      double acc = 0.0;
      for (int s = 0; s < 2; ++s) {
        if (!((allowed >> s) & 1)) continue;
        for (int d = 0; d < D; ++d) acc = fma(T[s * DD + a * D + d], right ? As[s * DD + b * D + d] : As[s * DD + d * D + b], acc);
      }
      v[j] = acc;
      mx = fmax(mx, fabs(acc));
    }
  }
  mx = wave_max(mx);
  if ((t & 63) == 0) red[t >> 6] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const int e = ms_exponent(mx);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = t + MS_ENV_THREADS * j;
    if (i < DD) {
      const double x = ldexp(v[j], -e);
      X[i] = x;
      if (out) out[i] = x;
    }
  }
  return e;
}

template <class Allowed, class Store>
__device__ __forceinline__ int ms_env_sweep(const double* cores, int n, int D, Allowed&& allowed_of, double* As, double* X, double* T,
                                            double* red, double* out, Store&& store) {
  const int DD = D * D, t = threadIdx.x;
  for (int i = t; i < DD; i += MS_ENV_THREADS) {
    X[i] = i == 0 ? 1.0 : 0.0;
    if (out) out[(long long)n * DD + i] = X[i];
  }
  store(n, 0);
  int ex = 0;
  for (int k = n; k >= 1; --k) {
    __syncthreads();
    ms_load_site_wg(cores, k, D, As);
    __syncthreads();
    ex += ms_env_step(true, D, allowed_of(k), As, X, T, red, out ? out + (long long)(k - 1) * DD : nullptr);
    store(k - 1, ex);
  }
  return ex;
}

constexpr uint32_t MS_PHILOX_DOMAIN = 0xffffffffu;

// The sampler's site loop for the lane's sample b (one wave per workgroup; As 2 DP DP and Es DP DP doubles of LDS) against the
// environments E [n + 1, D, D]: leaves the index word z, l^_n and its exponent el, and whether the sample died.  CLAMP: a site
// whose bit of `mask` is set takes that bit of `value`, ignores U_k and kills the sample when the m_s of that branch is not
// positive and finite; a dead sample's free bits are 0 and its clamped bits the evidence's.  The Philox counter does not
// depend on the mask: a free site sees the same U_k whatever else is clamped.
template <int DP, bool CLAMP>
__device__ __forceinline__ void ms_sample_sweep(const double* __restrict__ cores, int n, int D, long long b, bool active,
                                                const double* __restrict__ E, uint32_t seed_lo, uint32_t seed_hi, uint32_t ep,
                                                unsigned long long mask, unsigned long long value, double* As, double* Es,
                                                unsigned long long& z_out, double (&l)[DP], int& el_out, bool& dead_out, int* status) {
  ms_fill<DP>(l, 1.0);
  int el = 0;
  unsigned long long z = 0;
  bool dead = false;
  uint4 w = make_uint4(0, 0, 0, 0);
#pragma unroll 1
  for (int k = 1; k <= n; ++k) {
    __syncthreads();
    ms_load_site<DP>(cores, k, D, As, E + (long long)k * D * D, Es);
    __syncthreads();
    if (k & 1) w = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)((k + 1) / 2 - 1), MS_PHILOX_DOMAIN, ep), seed_lo, seed_hi);
    const double U = (k & 1) ? unit53(w.x, w.y) : unit53(w.z, w.w);
    double u0[DP], u1[DP];           // ms_row_dot's chains, both s in one loop: see the head of this file
#pragma unroll
    for (int c = 0; c < DP; ++c) {
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int a = 0; a < DP; ++a) {
        a0 = fma(l[a], As[a * DP + c], a0);
        a1 = fma(l[a], As[DP * DP + a * DP + c], a1);
      }
      u0[c] = a0;
      u1[c] = a1;
    }
    double m0 = 0.0, m1 = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      double t0 = 0.0, t1 = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) {
        const double e = Es[c * DP + d];
        t0 = fma(u0[c], e, t0);
        t1 = fma(u1[c], e, t1);
      }
      m0 = fma(t0, u0[d], m0);
      m1 = fma(t1, u1[d], m1);
    }
    const bool clamped = CLAMP && ((mask >> (n - k)) & 1ull);
    const bool ev = (value >> (n - k)) & 1ull;
    const double tot = clamped ? (ev ? m1 : m0) : m0 + m1;
    if (!dead && !(tot > 0.0 && isfinite(tot))) {
      dead = true;
      if (active) *status = 1;
    }
    const bool bit = clamped ? ev : (!dead && (U * tot >= m0));
    z = (z << 1) | (bit ? 1ull : 0ull);
#pragma unroll
    for (int a = 0; a < DP; ++a) l[a] = bit ? u1[a] : u0[a];
    el += ms_rescale<DP>(l);
  }
  z_out = z;
  el_out = el;
  dead_out = dead;
}

}  // namespace bornvi
