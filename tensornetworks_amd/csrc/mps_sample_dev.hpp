// Device helpers shared by the sampled-MPS kernels (kernels_mps_sample.hip, kernels_mps_sample_gram.hip): one definition of the
// power-of-two rescaling and of a site's load into LDS, so that l^, r^ and their exponents are the same bits in every kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace bornvi {

constexpr int MS_LANES = 64;               // sampler, score and Gram-vector kernels: one wave per workgroup

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

}  // namespace bornvi
