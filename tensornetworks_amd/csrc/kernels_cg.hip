// Conjugate gradients for (F + damping I) x = g with the product F p left to the caller: the
// matrix-free natural gradient of the sampled MPS, F p = O^T (O p) / B from bornvi_mps_score_jvp and bornvi_mps_score_vjp.
//
//   bornvi_cg_init     x = 0, r = p = g;  state = (rr = g^T g, rr0 = rr, iterations 0, done, relres, fallback, 0, 0)
//   bornvi_cg_step     q = Fp + damping p,  alpha = rr / p^T q,  x += alpha p,  r -= alpha q,  rr' = r^T r,  p = r + (rr' / rr) p
//   bornvi_cg_finish   x = g where the fallback flag is set or x is not finite;  info, the iteration count, sqrt(rr / rr0)
//
// Each entry point is one workgroup of CG_THREADS threads; thread t owns the elements t, t + CG_THREADS, ... of every
// vector (P <= 2 * 63 * 32^2 = 129 024 for an MPS: at most 126 elements per thread), so no element is read by a thread that
// did not write it and a step needs no fence.  Every dot product is one fixed-order reduction (reduce_dev.hpp, DESIGN.md
// section 4.6): the thread's elements in order, then block_sum over the 16 waves.  q is not stored: fma(damping, p, Fp) is
// evaluated again, to the same bits, where r is updated.
//
// The launch sequence of a solve never depends on the data.  Once the done flag is set (converged: rr' <= rel_tol^2 rr0;
// g = 0; g not finite; p^T q not positive and finite) a step writes nothing, so x, the iteration count and relres stay what
// they were and any number of further steps is harmless.  A breakdown at iteration 0 and a non-finite g set the fallback
// flag: there is no iterate to return.
//
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace bornvi {

namespace {
constexpr int CG_THREADS = 1024;
constexpr int CG_WAVES = CG_THREADS / 64;
enum { CG_RR = 0, CG_RR0 = 1, CG_ITERS = 2, CG_DONE = 3, CG_RELRES = 4, CG_FALLBACK = 5 };

__global__ __launch_bounds__(CG_THREADS) void cg_init_kernel(long long P, const double* __restrict__ g, double* __restrict__ x,
                                                             double* __restrict__ r, double* __restrict__ p,
                                                             double* __restrict__ state, int* __restrict__ info) {
  __shared__ double red[CG_WAVES];
  const int t = threadIdx.x;
  double acc = 0.0;
  int bad = 0;
  for (long long i = t; i < P; i += CG_THREADS) {
    const double gi = g[i];
    x[i] = 0.0;
    r[i] = gi;
    p[i] = gi;
    acc = fma(gi, gi, acc);
    bad |= !isfinite(gi);
  }
  const double rr = block_sum<CG_WAVES>(acc, red);
  const int anybad = __syncthreads_or(bad);
  if (t == 0) {
    state[CG_RR] = rr;
    state[CG_RR0] = rr;
    state[CG_ITERS] = 0.0;
    state[CG_DONE] = (anybad || !(rr > 0.0) || !isfinite(rr)) ? 1.0 : 0.0;
    state[CG_RELRES] = rr == 0.0 ? 0.0 : sqrt(rr / rr);                      // 1; 0 for g = 0; NaN where rr is not finite
    state[CG_FALLBACK] = (anybad || !isfinite(rr)) ? 1.0 : 0.0;
    state[6] = 0.0;
    state[7] = 0.0;
    *info = (anybad || !isfinite(rr)) ? 1 : 0;
  }
}

__global__ __launch_bounds__(CG_THREADS) void cg_step_kernel(long long P, double damping, double tol2, const double* __restrict__ Fp,
                                                             double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                                             double* __restrict__ state) {
  __shared__ double red[CG_WAVES];
  const int t = threadIdx.x;
  if (state[CG_DONE] != 0.0) return;                 // (uniform) frozen: nothing is written
  const double rr = state[CG_RR], rr0 = state[CG_RR0], iters = state[CG_ITERS];
  double acc = 0.0;
  for (long long i = t; i < P; i += CG_THREADS) {
    const double pi = p[i];
    acc = fma(pi, fma(damping, pi, Fp[i]), acc);
  }
  const double pq = block_sum<CG_WAVES>(acc, red);
  if (!(pq > 0.0) || !isfinite(pq)) {                // (uniform) no step: x stays the last iterate
    __syncthreads();                                 // every thread has read the state
    if (t == 0) {
      state[CG_DONE] = 1.0;
      if (iters == 0.0) state[CG_FALLBACK] = 1.0;
    }
    return;
  }
  const double alpha = rr / pq;
  acc = 0.0;
  for (long long i = t; i < P; i += CG_THREADS) {
    const double pi = p[i];
    const double qi = fma(damping, pi, Fp[i]);
    x[i] = fma(alpha, pi, x[i]);
    const double ri = fma(-alpha, qi, r[i]);
    r[i] = ri;
    acc = fma(ri, ri, acc);
  }
  const double rr1 = block_sum<CG_WAVES>(acc, red);
  const double beta = rr1 / rr;
  for (long long i = t; i < P; i += CG_THREADS) p[i] = fma(beta, p[i], r[i]);
  if (t == 0) {
    state[CG_RR] = rr1;
    state[CG_ITERS] = iters + 1.0;
    state[CG_RELRES] = sqrt(rr1 / rr0);
    if (rr1 <= tol2 * rr0) state[CG_DONE] = 1.0;
  }
}

__global__ __launch_bounds__(CG_THREADS) void cg_finish_kernel(long long P, const double* __restrict__ g, double* __restrict__ x,
                                                               const double* __restrict__ state, int* __restrict__ info,
                                                               int* __restrict__ iters, double* __restrict__ relres) {
  const int t = threadIdx.x;
  int bad = state[CG_FALLBACK] != 0.0;
  for (long long i = t; i < P; i += CG_THREADS) bad |= !isfinite(x[i]);
  const int fallback = __syncthreads_or(bad);
  if (fallback)
    for (long long i = t; i < P; i += CG_THREADS) x[i] = g[i];
  if (t == 0) {
    *info = fallback ? 1 : 0;
    *iters = (int)state[CG_ITERS];
    *relres = state[CG_RELRES];
  }
}
}  // namespace

hipError_t launch_cg_init(long long P, const double* g, double* x, double* r, double* p, double* state, int* info, hipStream_t st) {
  static_assert(BORNVI_CG_STATE_DOUBLES >= 8, "state words");
  cg_init_kernel<<<1, CG_THREADS, 0, st>>>(P, g, x, r, p, state, info);
  return hipGetLastError();
}

hipError_t launch_cg_step(long long P, double damping, double rel_tol, const double* Fp, double* x, double* r, double* p,
                          double* state, hipStream_t st) {
  cg_step_kernel<<<1, CG_THREADS, 0, st>>>(P, damping, rel_tol * rel_tol, Fp, x, r, p, state);
  return hipGetLastError();
}

hipError_t launch_cg_finish(long long P, const double* g, double* x, const double* state, int* info, int* iters, double* relres,
                            hipStream_t st) {
  cg_finish_kernel<<<1, CG_THREADS, 0, st>>>(P, g, x, state, info, iters, relres);
  return hipGetLastError();
}

}  // namespace bornvi
