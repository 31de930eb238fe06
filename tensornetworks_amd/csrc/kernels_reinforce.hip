// Classical Born machine, adversarial (KL) trainer: the REINFORCE step of the probability-table family
// (bornvi_reinforce_step).  Replaces reference adversarial_vi.py:200-222 for one observation.
//
// From B sampled outcome indices idx_b, the classifier's logits and the table log p(x_obs | z):
//   raw_b    = logit_b - log_p[idx_b]                       mean = (1/B) sum_b raw_b
//   baseline = mean (first call) or decay baseline + (1 - decay) mean
//   w_b      = raw_b - baseline + entropy_coef               (the reward plus the folded entropy bonus)
//   S_i      = sum of w_b over the samples with idx_b = i
//   dLdq[i]  = [q_i >= q_floor] S_i / (B q_i)                loss = (1/B) sum_i log max(q_i, q_floor) S_i
// (loss equals the reference's per-sample mean of log q_b w_b, regrouped by outcome.)
//
// The per-outcome sums S_i are integer sums: every w_b is rounded once to a multiple of u = 2^-e and added as a 64-bit
// integer, so the result does not depend on the order in which the adds arrive -- bitwise reproducible, and equal under
// any permutation of the samples that leaves the baseline's bits unchanged.  e is chosen from a bound of |w_b|,
//   W = max_b |raw_b| + |baseline| + |entropy_coef|,  e = 60 - ceil(log2 B) - ilogb(W),
// so that |w_b| / u < 2^(61 - ceil(log2 B)) and no sum of B terms leaves 62 bits.  Rounding error of S_i: at most
// c_i u / 2 for c_i samples on outcome i, u <= W 2^-(60 - ceil(log2 B)): 2^-44 W at B = 65,536, 2^-36 W at B = 2^24.
// The accumulator is the output buffer itself (a double and an int64 are both 8 bytes; integer 0 is +0.0), so outcomes
// no sample hit cost no store.  Adds go through a small per-workgroup LDS table first (a peaked q puts most samples of
// a workgroup on a few outcomes: they become one global add each); what does not find a slot is added directly.
//
// The mean is a two-level float64 sum in the fixed order of reduce_dev.hpp over sample positions (per-workgroup partials in
// the workspace, reduced by every workgroup of the next kernel in the same order): bitwise repeatable; permuting the samples changes
// its last bits.  A non-finite raw_b (log_p may hold +-inf) makes mean and baseline non-finite as in the reference;
// no add is made then, dLdq is all zeros, loss = NaN and found_inf = 1.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace bornvi {

namespace {
constexpr int RF_THREADS = 256;
constexpr int RF_WAVES = RF_THREADS / 64;
constexpr long long RF_SAMPLES_PER_WG = 1024;   // target samples per workgroup
constexpr long long RF_OUTCOMES_PER_WG = 4096;  // target outcomes per workgroup (zeroing and the finishing pass)
constexpr long long RF_MAX_WG = 1024;           // partials per level at most
constexpr int RF_SLOT_BITS = 10, RF_SLOTS = 1 << RF_SLOT_BITS;   // LDS pre-aggregation table of a workgroup

ChunkGeom rf_geom(long long count, long long per_wg) { return chunk_geom(count, per_wg, RF_MAX_WG, 1); }

// scalars handed from kernel to kernel through the workspace
struct RfScalars {
  double baseline_new;
  double scale;       // 2^e
  double inv_scale;   // 2^-e
  int bad;            // 1: a weight is not finite (no adds were made)
};

// raw reward of sample b; 0 for an index outside the table (never dereferenced: "no sample")
__device__ __forceinline__ double raw_reward(const long long* __restrict__ idx, const float* __restrict__ logit,
                                             const float* __restrict__ log_p, long long N, long long b, long long& i) {
  i = idx[b];
  if (i < 0 || i >= N) {
    i = -1;
    return 0.0;
  }
  return (double)logit[b] - (double)log_p[i];
}

// pass 1: zero the accumulator (= dLdq); per sample chunk the sum and the largest magnitude of the raw rewards.
// grid = max(G samples chunks, Gz outcome chunks) workgroups.
__global__ __launch_bounds__(RF_THREADS) void reinforce_stats_kernel(const long long* __restrict__ idx,
                                                                     const float* __restrict__ logit,
                                                                     const float* __restrict__ log_p, long long N, long long B,
                                                                     long long chunk, int G, long long zchunk,
                                                                     long long* __restrict__ acc, double* __restrict__ part) {
  __shared__ double lds[RF_WAVES];
  const long long g = blockIdx.x;
  const long long z0 = g * zchunk, z1 = min(N, z0 + zchunk);
  for (long long i = z0 + threadIdx.x; i < z1; i += RF_THREADS) acc[i] = 0;
  if (g >= G) return;
  const long long c0 = g * chunk, c1 = min(B, c0 + chunk);
  double s = 0.0, m = 0.0;
  for (long long b = c0 + threadIdx.x; b < c1; b += RF_THREADS) {
    long long i;
    const double r = raw_reward(idx, logit, log_p, N, b, i);
    s += r;
    m = max_nan(m, fabs(r));
  }
  s = block_sum<RF_WAVES>(s, lds);
  m = block_max_nan<RF_WAVES>(m, lds);
  if (threadIdx.x == 0) {
    part[2 * g] = s;
    part[2 * g + 1] = m;
  }
}

// pass 2: mean, baseline and the fixed-point scale from the partials (every workgroup, same order); then the adds.
__global__ __launch_bounds__(RF_THREADS) void reinforce_scatter_kernel(const long long* __restrict__ idx,
                                                                       const float* __restrict__ logit,
                                                                       const float* __restrict__ log_p, long long N,
                                                                       long long B, long long chunk, int G, int log2B_ceil,
                                                                       const double* __restrict__ part,
                                                                       const double* __restrict__ baseline, int first,
                                                                       double decay, double coef,
                                                                       unsigned long long* __restrict__ acc,
                                                                       RfScalars* __restrict__ sc) {
  __shared__ double lds[RF_WAVES];
  __shared__ int keys[RF_SLOTS];
  __shared__ unsigned long long vals[RF_SLOTS];
  const int t = threadIdx.x;
  for (int k = t; k < RF_SLOTS; k += RF_THREADS) {
    keys[k] = -1;
    vals[k] = 0ull;
  }
  double s = 0.0, m = 0.0;
  for (int k = t; k < G; k += RF_THREADS) {
    s += part[2 * k];
    m = max_nan(m, part[2 * k + 1]);
  }
  s = block_sum<RF_WAVES>(s, lds);
  m = block_max_nan<RF_WAVES>(m, lds);      // (its barriers also publish the cleared table)
  const double mean = s / (double)B;
  const double base = first ? mean : decay * baseline[0] + (1.0 - decay) * mean;
  const double W = m + fabs(base) + fabs(coef);
  const bool bad = !(W < INFINITY);           // NaN or Inf: some weight is not finite
  int e = 0;
  if (!bad && W > 0.0) {
    e = 60 - log2B_ceil - ilogb(W);
    e = e > 1000 ? 1000 : (e < -1000 ? -1000 : e);
  }
  const double scale = ldexp(1.0, e);
  if (blockIdx.x == 0 && t == 0) {
    sc->baseline_new = base;
    sc->scale = scale;
    sc->inv_scale = ldexp(1.0, -e);
    sc->bad = bad ? 1 : 0;
  }
  if (bad) return;
  const long long g = blockIdx.x;
  const long long c0 = g * chunk, c1 = min(B, c0 + chunk);
  for (long long b = c0 + t; b < c1; b += RF_THREADS) {
    long long i;
    const double r = raw_reward(idx, logit, log_p, N, b, i);
    if (i < 0) continue;
    const unsigned long long f = (unsigned long long)__double2ll_rn((r - base + coef) * scale);
    const int slot = (int)(((unsigned)i * 2654435761u) >> (32 - RF_SLOT_BITS));
    const int prev = atomicCAS(&keys[slot], -1, (int)i);
    if (prev == -1 || prev == (int)i) atomicAdd(&vals[slot], f);
    else atomicAdd(&acc[i], f);
  }
  __syncthreads();
  for (int k = t; k < RF_SLOTS; k += RF_THREADS) {
    const int key = keys[k];
    const unsigned long long v = vals[k];
    if (key >= 0 && v != 0ull) atomicAdd(&acc[key], v);
  }
}

// pass 3: the integer sums become dLdq in place; per outcome chunk the partial of sum_i log max(q_i, floor) S_i.
__global__ __launch_bounds__(RF_THREADS) void reinforce_finish_kernel(const float* __restrict__ q32, long long N, long long B,
                                                                      long long zchunk, float q_floor,
                                                                      const RfScalars* __restrict__ sc,
                                                                      long long* __restrict__ acc, double* __restrict__ lpart) {
  __shared__ double lds[RF_WAVES];
  const long long g = blockIdx.x;
  const long long z0 = g * zchunk, z1 = min(N, z0 + zchunk);
  const double inv_scale = sc->inv_scale;
  const double Bd = (double)B;
  double l = 0.0;
  for (long long i = z0 + threadIdx.x; i < z1; i += RF_THREADS) {
    const long long S = acc[i];
    if (S == 0) continue;
    const double s = (double)S * inv_scale;
    const float q = q32[i];
    const float c = (q < q_floor) ? q_floor : q;      // (a NaN stays NaN, as in torch.clamp)
    l += log((double)c) * s;
    // the clamp passes no gradient below the floor
    acc[i] = __double_as_longlong((q >= q_floor || q != q) ? s / (Bd * (double)q) : 0.0);
  }
  l = block_sum<RF_WAVES>(l, lds);
  if (threadIdx.x == 0) lpart[g] = l;
}

// pass 4: loss, the guard flag and the baseline.  One workgroup.
__global__ __launch_bounds__(RF_THREADS) void reinforce_loss_kernel(const double* __restrict__ lpart, int Gz, long long B,
                                                                    const RfScalars* __restrict__ sc,
                                                                    double* __restrict__ baseline, float* __restrict__ loss,
                                                                    float* __restrict__ found_inf) {
  __shared__ double lds[RF_WAVES];
  const double l = sum_partials<RF_THREADS>(lpart, Gz, lds);
  if (threadIdx.x == 0) {
    const float lf = sc->bad ? NAN : (float)(l / (double)B);
    loss[0] = lf;
    found_inf[0] = (lf - lf == 0.0f) ? 0.0f : 1.0f;
    baseline[0] = sc->baseline_new;
  }
}

}  // namespace

size_t reinforce_workspace_bytes(int n, long long B) {
  const ChunkGeom gs = rf_geom(B, RF_SAMPLES_PER_WG), gz = rf_geom(1ll << n, RF_OUTCOMES_PER_WG);
  return 256 + (size_t)(2 * gs.G + gz.G) * sizeof(double) + 512;
}

hipError_t launch_reinforce_step(int n, long long B, const long long* idx, const float* logit, const float* log_p,
                                 const float* q32, double* baseline, int first, double decay, double coef, double q_floor,
                                 double* dLdq, float* loss, float* found_inf, void* ws, hipStream_t st) {
  const long long N = 1ll << n;
  const ChunkGeom gs = rf_geom(B, RF_SAMPLES_PER_WG), gz = rf_geom(N, RF_OUTCOMES_PER_WG);
  char* w = ws_align(ws);
  RfScalars* sc = (RfScalars*)w;
  double* part = (double*)(w + 256);
  double* lpart = part + 2 * gs.G;
  int log2B = 0;
  while ((1ll << log2B) < B) ++log2B;
  // pass 1 zeroes slice g of the accumulator in workgroup g: as many workgroups as the larger of the two chunkings
  const int G1 = gs.G > gz.G ? gs.G : gz.G;
  const long long zchunk1 = (N + G1 - 1) / G1;
  reinforce_stats_kernel<<<dim3((unsigned)G1), RF_THREADS, 0, st>>>(idx, logit, log_p, N, B, gs.chunk, gs.G, zchunk1,
                                                                   (long long*)dLdq, part);
  reinforce_scatter_kernel<<<dim3((unsigned)gs.G), RF_THREADS, 0, st>>>(idx, logit, log_p, N, B, gs.chunk, gs.G, log2B, part,
                                                                       baseline, first, decay, coef,
                                                                       (unsigned long long*)dLdq, sc);
  reinforce_finish_kernel<<<dim3((unsigned)gz.G), RF_THREADS, 0, st>>>(q32, N, B, gz.chunk, (float)q_floor, sc,
                                                                      (long long*)dLdq, lpart);
  reinforce_loss_kernel<<<dim3(1), RF_THREADS, 0, st>>>(lpart, gz.G, B, sc, baseline, loss, found_inf);
  return hipGetLastError();
}

}  // namespace bornvi
