// Exact posterior queries of the sampled matrix-product-state Born machine: what the fitted q says
// about parts of z, read off its environments in O(n D^3) per query.  Conventions of kernels_mps_sample.hip: cores
// [n, 2, D, D] float64, 1 <= n <= 63, 1 <= D <= 32, site k's bit is bit n - k of an int64 word (ms_bit).  An evidence is a pair
// of words (mask, value): a set mask bit clamps that site to the value's bit; value bits outside the mask and bits at or
// above n are never looked at.
//
// Clamped environments:  E^(j)_n = e0 e0^T,  E^(j)_{k-1} = sum_{s allowed at k} A_k[s] E^(j)_k A_k[s]^T; a clamped site allows one
//   s, a free site both (ms_allowed).  The sweep is ms_env_sweep, its step mps_env_kernel's ms_env_step: an empty mask gives that kernel's bits.
//
// bornvi_mps_log_marginals: mps_query_env_kernel, one workgroup per query and one more (the last) for the empty mask; each
//   leaves (E^^(j)_0[0, 0], e_j) in the workspace's pair table and nothing of size Q n D^2 is stored.  mps_query_logm_kernel:
//   logm_j = (log E^^(j)_0[0, 0] - log E^_0[0, 0]) + (e_j - e) ln 2:  an empty evidence gives exactly 0.0, a full one log q of
//   that state.  A pair that is not finite (or negative) gives NaN, a zero one -inf; either sets the status word to 1.
//
// bornvi_mps_sample_clamped: mps_query_env_kernel with a grid of two (the evidence, whose stack E^^(j)_k and exponents go to
//   the workspace, and the empty mask), then mps_sample_clamped_kernel: ms_sample_sweep, the loop of mps_sample_kernel, with
//   the evidence.  logq = ms_logq(l^_n[0], el, E^^(j)_0[0, 0], e_j) = log q(z | evidence); with all n sites clamped it is 0.0 by
//   definition (a point mass), not by cancellation.  Lane 0 of workgroup 0 writes logm.
//
// bornvi_mps_marginals runs both unclamped sweeps itself (mps_env_kernel into the query workspace), then
//   mps_marginals_kernel, one workgroup per site i:
//     m1[i] = <L_{i-1}, A_i[1] E_i A_i[1]^T> / Z                                          (mq_inner)
//     M = A_i[1]^T L_{i-1} A_i[1]                                                        (ms_env_step, left, s = 1 alone)
//     j = i + 1 .. n:  m2[i][j] = <M, A_j[1] E_j A_j[1]^T> / Z,  M <- sum_s A_j[s]^T M A_j[s]   (ms_env_step, left, both s)
//   M is rescaled by an exact power of two at every step; the exponents eL[i - 1], M's own, eE[j] and eE[0] are folded in with
//   one ldexp.  mq_inner: T = A[1] E and G = T A[1]^T as D-term fma chains through LDS, then per row a the chain
//   sum_b X[a][b] G[a][b] and the rows added in order.  m2[j][i] is stored from the value of m2[i][j] and m2[i][i] from m1[i].
//
// bornvi_mps_log_marginals_vjp: the gradient of weighted log-marginals, stated above its kernels below.
//
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "mps_sample_dev.hpp"

namespace bornvi {

namespace {

struct MqLayout {
  size_t hdr, E, L, eE, eL, pairs, total;     // byte offsets from the aligned base
};

MqLayout mq_layout(int n, int D, int Q) {
  MqLayout S;
  size_t o = 0;
  S.hdr = o;   o += 256;                                                     // log Z, E^_0[0, 0], eE[0] of the unclamped sweep
  S.E = o;     o += ws_round((size_t)(n + 1) * D * D * sizeof(double));      // the stack of one evidence, or the unclamped one
  S.L = o;     o += ws_round((size_t)(n + 1) * D * D * sizeof(double));
  S.eE = o;    o += ws_round((size_t)(n + 1) * sizeof(int));
  S.eL = o;    o += ws_round((size_t)(n + 1) * sizeof(int));
  S.pairs = o; o += ws_round((size_t)(Q + 1) * 2 * sizeof(double));          // (E^^(j)_0[0, 0], e_j), slot Q: the empty mask
  S.total = o;
  return S;
}

// grid Q + 1: workgroup j < Q sweeps the evidence (mask[j], value[j]), workgroup Q the empty mask.  pairs[2 j], [2 j + 1] =
// E^^(j)_0[0, 0], e_j.  stackE / stackeE (or null): where workgroup 0 leaves E^^(0)_k and its exponents, k = n .. 0.
__global__ __launch_bounds__(MS_ENV_THREADS) void mps_query_env_kernel(const double* __restrict__ cores, int n, int D, int Q,
                                                                    const long long* __restrict__ mask,
                                                                    const long long* __restrict__ value, double* __restrict__ pairs,
                                                                    double* __restrict__ stackE, int* __restrict__ stackeE) {
  __shared__ double As[2 * MS_DMAX * MS_DMAX];
  __shared__ double X[MS_DMAX * MS_DMAX];
  __shared__ double T[2 * MS_DMAX * MS_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  const int j = blockIdx.x, t = threadIdx.x;
  const unsigned long long mk = j < Q ? (unsigned long long)mask[j] : 0ull;
  const unsigned long long vl = j < Q ? (unsigned long long)value[j] : 0ull;
  double* out = (j == 0 && stackE) ? stackE : nullptr;
  const int ex = ms_env_sweep(cores, n, D, [&](int k) { return ms_allowed(mk, vl, n, k); }, As, X, T, red, out,
                              [&](int slot, int e) { if (out && t == 0) stackeE[slot] = e; });
  __syncthreads();
  if (t == 0) {
    pairs[2 * j] = X[0];
    pairs[2 * j + 1] = (double)ex;
  }
}

// (a_j, e_j) against (a, e) of the empty mask: log of the ratio, the exponents kept apart
__device__ __forceinline__ double mq_logm(double aj, double ej, double a, double e, bool* bad) {
  const bool fin = isfinite(aj) && isfinite(a) && aj >= 0.0 && a >= 0.0;
  *bad = !fin || !(aj > 0.0) || !(a > 0.0);
  if (!fin) return __builtin_nan("");
  return (log(aj) - log(a)) + (ej - e) * MS_LN2;
}

__global__ __launch_bounds__(256) void mps_query_logm_kernel(int Q, const double* __restrict__ pairs, double* __restrict__ logm,
                                                            int* status) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Q) return;
  bool bad;
  logm[j] = mq_logm(pairs[2 * j], pairs[2 * j + 1], pairs[2 * Q], pairs[2 * Q + 1], &bad);
  if (bad) *status = 1;
}

template <int DP>
__global__ __launch_bounds__(MS_LANES) void mps_sample_clamped_kernel(const double* __restrict__ cores, int n, int D, long long B,
                                                                      const double* __restrict__ E, const double* __restrict__ pairs,
                                                                      const long long* __restrict__ mask,
                                                                      const long long* __restrict__ value, uint32_t seed_lo,
                                                                      uint32_t seed_hi, const long long* __restrict__ epoch_dev,
                                                                      long long* __restrict__ idx, double* __restrict__ logq,
                                                                      double* __restrict__ logm, int* status) {
  __shared__ double As[2 * DP * DP];
  __shared__ double Es[DP * DP];
  const long long b = (long long)blockIdx.x * MS_LANES + threadIdx.x;
  const bool active = b < B;
  const uint32_t ep = (uint32_t)(unsigned long long)(*epoch_dev);
  const unsigned long long mk = (unsigned long long)mask[0], vl = (unsigned long long)value[0];
  double l[DP];
  int el;
  unsigned long long z;
  bool dead;
  ms_sample_sweep<DP, true>(cores, n, D, b, active, E, seed_lo, seed_hi, ep, mk, vl, As, Es, z, l, el, dead, status);
  if (active) {
    idx[b] = (long long)z;
    // all n sites clamped: q(. | evidence) is a point mass, log 1 = 0.0 exactly (the two roundings of psi^2 would not cancel)
    const bool full = (mk & ((1ull << n) - 1ull)) == (1ull << n) - 1ull;
    logq[b] = dead ? __builtin_nan("") : full ? 0.0 : ms_logq(l[0], el, pairs[0], pairs[1]);
  }
  if (b == 0) {
    bool bad;
    logm[0] = mq_logm(pairs[0], pairs[1], pairs[2], pairs[3], &bad);
    if (bad) *status = 1;
  }
}

// <X, A[1] Em A[1]^T> for D x D matrices in LDS (A1 = the site's A[1] as stored, pitch D): T and G are D D doubles of scratch,
// R holds D row sums.  Begins and ends on a barrier; every lane returns the same value.
__device__ __forceinline__ double mq_inner(int D, const double* X, const double* A1, const double* Em, double* T, double* G, double* R) {
  const int DD = D * D, t = threadIdx.x;
  __syncthreads();
  for (int i = t; i < DD; i += MS_ENV_THREADS) {        // ms_mul_AX's chain for s = 1 alone: profiles/mps_env_core_isa.txt
    const int a = i / D, d = i % D;
    double acc = 0.0;
    for (int e = 0; e < D; ++e) acc = fma(A1[a * D + e], Em[e * D + d], acc);
    T[i] = acc;
  }
  __syncthreads();
  for (int i = t; i < DD; i += MS_ENV_THREADS) {
    const int a = i / D, b = i % D;
    double acc = 0.0;
    for (int d = 0; d < D; ++d) acc = fma(T[a * D + d], A1[b * D + d], acc);
    G[i] = acc;
  }
  __syncthreads();
  if (t < D) {
    double acc = 0.0;
    for (int b = 0; b < D; ++b) acc = fma(X[t * D + b], G[t * D + b], acc);
    R[t] = acc;
  }
  __syncthreads();
  double sum = 0.0;
  for (int a = 0; a < D; ++a) sum += R[a];
  __syncthreads();
  return sum;
}

// grid n: site i = blockIdx.x + 1
__global__ __launch_bounds__(MS_ENV_THREADS) void mps_marginals_kernel(const double* __restrict__ cores, int n, int D,
                                                                    const double* __restrict__ E, const double* __restrict__ L,
                                                                    const int* __restrict__ eE, const int* __restrict__ eL,
                                                                    const double* __restrict__ hdr, double* __restrict__ m1,
                                                                    double* __restrict__ m2) {
  __shared__ double As[2 * MS_DMAX * MS_DMAX];
  __shared__ double X[MS_DMAX * MS_DMAX];
  __shared__ double Em[MS_DMAX * MS_DMAX];
  __shared__ double T[2 * MS_DMAX * MS_DMAX];
  __shared__ double R[MS_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  const int i = blockIdx.x + 1, DD = D * D, t = threadIdx.x;
  const double Zh = hdr[1];
  const int eZ = eE[0];
  ms_load_site_wg(cores, i, D, As);
  for (int x = t; x < DD; x += MS_ENV_THREADS) {
    X[x] = L[(long long)(i - 1) * DD + x];
    Em[x] = E[(long long)i * DD + x];
  }
  const double s1 = mq_inner(D, X, As + DD, Em, T, T + DD, R);
  const double v1 = ldexp(s1 / Zh, eL[i - 1] + eE[i] - eZ);
  if (t == 0) {
    m1[i - 1] = v1;
    if (m2) m2[(long long)(i - 1) * n + (i - 1)] = v1;
  }
  if (!m2) return;
  int eM = eL[i - 1] + ms_env_step(false, D, 2, As, X, T, red, nullptr);
  for (int j = i + 1; j <= n; ++j) {
    __syncthreads();
    ms_load_site_wg(cores, j, D, As);
    for (int x = t; x < DD; x += MS_ENV_THREADS) Em[x] = E[(long long)j * DD + x];
    const double s2 = mq_inner(D, X, As + DD, Em, T, T + DD, R);
    const double v2 = ldexp(s2 / Zh, eM + eE[j] - eZ);
    if (t == 0) {
      m2[(long long)(i - 1) * n + (j - 1)] = v2;
      m2[(long long)(j - 1) * n + (i - 1)] = v2;
    }
    if (j < n) eM += ms_env_step(false, D, 3, As, X, T, red, nullptr);
  }
}

// ---- gradient of weighted log-marginals -----------------------------------------------------
// grad = sum_j c_j grad log q(evidence_j),  log q(e_j) = log m_j - log Z,  m_j = E^(j)_0[0, 0],
//   d m_j / d A_k[s] = 2 L^(j)_{k-1} A_k[s] E^(j)_k  for s allowed at site k, 0 for a disallowed s,
// L^(j) the clamped LEFT environments (L_0 = e0 e0^T, L_k = sum_{s allowed} A_k[s]^T L_{k-1} A_k[s]); minus (sum_j c_j) times
// the same expression of the empty mask (Z is the empty evidence's mass).
//
// mps_logm_vjp_kernel, grid G + 1 of MS_ENV_THREADS: workgroup g < G = min(Q, MQ_VJP_MAX_WG) takes the queries g, g + G, ... in
// that order, workgroup G the empty mask with weight 1.  Per query:
//   right sweep: ms_env_sweep, mps_query_env_kernel's call, the stack E^^(j)_k into the workgroup's own slot of the workspace, its
//     exponents into LDS, (E^^(j)_0[0, 0], e_j) into the pair table: logm is mps_query_logm_kernel's, bornvi_mps_log_marginals' bits;
//   left sweep, k = 1 .. n, L^ in LDS:  T_s = A_s E^^_k (ms_mul_AX), M_s = L^_{k-1} T_s (ms_env_chain) for the allowed s; the entry
//     is M_s (c_j / E^^(j)_0[0, 0]) 2^(eL + eE[k] - e_j), doubled, and is added to the workgroup's own partial [n, 2, D, D]: entry i of a
//     site always by thread i mod MS_ENV_THREADS, so no atomics and no barrier guard it; then ms_env_step (left), the same allowed set.
//   A query whose mass is not positive and finite, or whose weight is 0.0, takes no left sweep and adds nothing, and an impossible
//   one's weight stays out of the workgroup's weight sum.  mps_logm_vjp_finish_kernel: per entry the partials of workgroups
//   0 .. G - 1 in order, minus W times the empty mask's entry, W the workgroups' weight sums by sum_partials.
constexpr int MQ_VJP_MAX_WG = 256;      // one per compute unit of the MI355X

__host__ __device__ inline int mq_vjp_groups(int Q) { return Q < MQ_VJP_MAX_WG ? Q : MQ_VJP_MAX_WG; }

struct MqVjpLayout {
  size_t parts, stacks, wpart, pairs, total;
  int G;
};

MqVjpLayout mq_vjp_layout(int n, int D, int Q) {
  MqVjpLayout S;
  S.G = mq_vjp_groups(Q);
  size_t o = 0;
  S.parts = o;  o += ws_round((size_t)(S.G + 1) * n * 2 * D * D * sizeof(double));     // slot G: the empty mask's term
  S.stacks = o; o += ws_round((size_t)(S.G + 1) * (n + 1) * D * D * sizeof(double));
  S.wpart = o;  o += ws_round((size_t)(S.G + 1) * sizeof(double));
  S.pairs = o;  o += ws_round((size_t)(Q + 1) * 2 * sizeof(double));
  S.total = o;
  return S;
}

__global__ __launch_bounds__(MS_ENV_THREADS) void mps_logm_vjp_kernel(const double* __restrict__ cores, int n, int D, int Q, int G,
                                                                   const long long* __restrict__ mask,
                                                                   const long long* __restrict__ value,
                                                                   const double* __restrict__ c, double* __restrict__ pairs,
                                                                   double* parts, double* stacks, double* __restrict__ wpart) {
  __shared__ double As[2 * MS_DMAX * MS_DMAX];
  __shared__ double X[MS_DMAX * MS_DMAX];
  __shared__ double Em[MS_DMAX * MS_DMAX];
  __shared__ double T[2 * MS_DMAX * MS_DMAX];
  __shared__ double red[MS_ENV_THREADS / 64];
  __shared__ int eEs[64];
  const int g = blockIdx.x, DD = D * D, t = threadIdx.x;
  double* part = parts + (size_t)g * n * 2 * DD;
  double* stack = stacks + (size_t)g * (n + 1) * DD;
  for (int k = 0; k < n; ++k)
    for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) part[(size_t)k * 2 * DD + i] = 0.0;
  double wsum = 0.0;
  const int first = g < G ? g : Q, step = g < G ? G : 1;      // workgroup G: the one "query" Q, the empty mask
  for (int j = first; j <= Q && (j < Q || g == G); j += step) {
    const unsigned long long mk = j < Q ? (unsigned long long)mask[j] : 0ull;
    const unsigned long long vl = j < Q ? (unsigned long long)value[j] : 0ull;
    const double cj = j < Q ? c[j] : 1.0;
    const auto allowed_of = [&](int k) { return ms_allowed(mk, vl, n, k); };
    __syncthreads();                                           // the query before this one is done with X, As and eEs
    const int ex = ms_env_sweep(cores, n, D, allowed_of, As, X, T, red, stack, [&](int slot, int e) { if (t == 0) eEs[slot] = e; });
    __syncthreads();                                           // publishes X, the stack and eEs
    const double aj = X[0];
    if (t == 0) {
      pairs[2 * j] = aj;
      pairs[2 * j + 1] = (double)ex;
    }
    const bool possible = aj > 0.0 && isfinite(aj);
    if (possible) wsum += cj;
    if (!possible || cj == 0.0) continue;                      // the same decision in every thread
    const double f = cj / aj;
    __syncthreads();                                           // every thread has read X[0]
    for (int i = t; i < DD; i += MS_ENV_THREADS) X[i] = i == 0 ? 1.0 : 0.0;
    int eL = 0;
    for (int k = 1; k <= n; ++k) {
      const int allowed = allowed_of(k);
      __syncthreads();                                         // the step before is done with As and T
      ms_load_site_wg(cores, k, D, As);
      for (int i = t; i < DD; i += MS_ENV_THREADS) Em[i] = stack[(size_t)k * DD + i];
      __syncthreads();
      ms_mul_AX(D, allowed, As, Em, T);
      __syncthreads();
      const int sh = eL + eEs[k] - ex;
      for (int i = t; i < 2 * DD; i += MS_ENV_THREADS) {
        if (!((allowed >> (i / DD)) & 1)) continue;
        const double term = ldexp(ms_env_chain(X, T, D, i) * f, sh);          // its own scaling: not ms_env_entry's rounding
        part[(size_t)(k - 1) * 2 * DD + i] += term + term;
      }
      __syncthreads();                                         // T is the step's scratch
      if (k < n) eL += ms_env_step(false, D, allowed, As, X, T, red, nullptr);
    }
  }
  if (t == 0) wpart[g] = wsum;
}

__global__ __launch_bounds__(MS_ENV_THREADS) void mps_logm_vjp_finish_kernel(long long count, int G, const double* __restrict__ parts,
                                                                          const double* __restrict__ wpart,
                                                                          double* __restrict__ grad) {
  __shared__ double red[MS_ENV_THREADS / 64];
  const double W = sum_partials<MS_ENV_THREADS>(wpart, G, red);
  const long long i = (long long)blockIdx.x * MS_ENV_THREADS + threadIdx.x;
  if (i >= count) return;
  double sum = 0.0;
  for (int g = 0; g < G; ++g) sum += parts[(size_t)g * count + i];
  grad[i] = sum - W * parts[(size_t)G * count + i];
}

}  // namespace

size_t mps_log_marginals_vjp_workspace_bytes(int n, int D, int Q) { return mq_vjp_layout(n, D, Q).total + 256; }

int mps_log_marginals_vjp_groups(int Q) { return mq_vjp_groups(Q); }

hipError_t launch_mps_log_marginals_vjp(int n, int D, int Q, const double* cores, const long long* mask, const long long* value,
                                        const double* c, double* grad, double* logm, int* status, void* ws, hipStream_t st) {
  const MqVjpLayout S = mq_vjp_layout(n, D, Q);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  double* pairs = (double*)(base + S.pairs);
  double* parts = (double*)(base + S.parts);
  double* wpart = (double*)(base + S.wpart);
  mps_logm_vjp_kernel<<<(unsigned)(S.G + 1), MS_ENV_THREADS, 0, st>>>(cores, n, D, Q, S.G, mask, value, c, pairs, parts,
                                                                    (double*)(base + S.stacks), wpart);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long count = (long long)n * 2 * D * D;
  mps_logm_vjp_finish_kernel<<<(unsigned)((count + MS_ENV_THREADS - 1) / MS_ENV_THREADS), MS_ENV_THREADS, 0, st>>>(count, S.G, parts,
                                                                                                                 wpart, grad);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mps_query_logm_kernel<<<(unsigned)((Q + 255) / 256), 256, 0, st>>>(Q, pairs, logm, status);
  return hipGetLastError();
}

size_t mps_query_workspace_bytes(int n, int D, int Q) { return mq_layout(n, D, Q).total + 256; }

hipError_t launch_mps_log_marginals(int n, int D, int Q, const double* cores, const long long* mask, const long long* value,
                                    double* logm, int* status, void* ws, hipStream_t st) {
  const MqLayout S = mq_layout(n, D, Q);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  double* pairs = (double*)(base + S.pairs);
  mps_query_env_kernel<<<(unsigned)(Q + 1), MS_ENV_THREADS, 0, st>>>(cores, n, D, Q, mask, value, pairs, nullptr, nullptr);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mps_query_logm_kernel<<<(unsigned)((Q + 255) / 256), 256, 0, st>>>(Q, pairs, logm, status);
  return hipGetLastError();
}

hipError_t launch_mps_sample_clamped(int n, int D, long long B, const double* cores, const long long* mask, const long long* value,
                                     unsigned long long seed, const long long* epoch_dev, long long* idx, double* logq, double* logm,
                                     int* status, void* ws, hipStream_t st) {
  const MqLayout S = mq_layout(n, D, 1);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  double* pairs = (double*)(base + S.pairs);
  mps_query_env_kernel<<<2, MS_ENV_THREADS, 0, st>>>(cores, n, D, 1, mask, value, pairs, (double*)(base + S.E), (int*)(base + S.eE));
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int DPV = bond_dp(D);
  const unsigned grid = (unsigned)((B + MS_LANES - 1) / MS_LANES);
  BOND_DISPATCH(DPV, (mps_sample_clamped_kernel<DP><<<grid, MS_LANES, 0, st>>>(cores, n, D, B, (const double*)(base + S.E), pairs, mask,
                                                                             value, (uint32_t)seed, (uint32_t)(seed >> 32), epoch_dev,
                                                                             idx, logq, logm, status)));
  return hipGetLastError();
}

hipError_t launch_mps_marginals(int n, int D, const double* cores, double* m1, double* m2, void* ws, hipStream_t st) {
  const MqLayout S = mq_layout(n, D, 1);
  char* base = ws_align(ws);
  double* E = (double*)(base + S.E);
  double* L = (double*)(base + S.L);
  int* eE = (int*)(base + S.eE);
  int* eL = (int*)(base + S.eL);
  double* hdr = (double*)(base + S.hdr);
  hipError_t e = launch_mps_environments_into(n, D, cores, E, L, eE, eL, hdr, st);
  if (e != hipSuccess) return e;
  mps_marginals_kernel<<<(unsigned)n, MS_ENV_THREADS, 0, st>>>(cores, n, D, E, L, eE, eL, hdr, m1, m2);
  return hipGetLastError();
}

}  // namespace bornvi
