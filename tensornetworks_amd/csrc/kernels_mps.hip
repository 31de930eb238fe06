// Matrix-product-state Born machine (bornvi_mps_probs / bornvi_mps_vjp): theta -> q over all 2^n outcomes and
// (theta, dL/dq) -> dL/dtheta for  q(z) = psi(z)^2 / Z,  psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0,  cores [n, 2, D, D] float64.
//
// Forward, prefix doubling:  V_0 = e0^T,  V_k[2p + s, :] = V_{k-1}[p, :] A_k[s]  (p < 2^(k-1)),  psi(z) = V_n[z, 0].
// Backward, given g = dL/dq:  G_n[z, 0] = 2 psi_z (g_z - c) / Z with c = sum q g;  for k = n .. 1
//   dA_k[s] = sum_p V_{k-1}[p, :]^T G_k[2p + s, :],      G_{k-1}[p, :] = sum_s G_k[2p + s, :] A_k[s]^T.
//
// Workspace (mps_layout): a header (Z), the partials of Z and c, psi [2^n], the levels V_0 .. V_{n-1} (V_k is [2^k, DS]
// doubles, DS = D rounded up to even so that every row is a whole number of 16-byte accesses; the pad column is 0), two
// buffers for G_{n-1}, G_{n-2}, ... in turn, and per level the workgroups' partials of dA_k.  bornvi_mps_probs fills the
// header, psi and the levels; bornvi_mps_vjp reads them: V_n is never stored (only its column 0 = psi is needed).
//
// Work split.  A level k has P = 2^(k-1) parent rows.
//   Levels k <= MPS_FUSED (P <= 512) run in ONE launch of one workgroup, which walks them with a barrier in between (the
//   rows go through the workspace: a workgroup sees its own global writes after the barrier); for n <= MPS_FUSED + 1 that
//   launch also does the last level.  Larger levels are one launch each, min(1024, P / 256) workgroups with a contiguous
//   block of parents each.
//   Row products (V A, G A^T): one lane per parent row, the row in registers (16-byte loads and stores), A_k[s] zero-padded
//   to DP x DP (DP = 2, 4, 8, 16, 32 >= D) in LDS and read as broadcasts; plain v_fma_f64, the sum over the bond index in
//   index order.
//   dA_k = V^T G is a GEMM whose long dimension is p: v_mfma_f64_16x16x4_f64 with both operands read straight from global
//   memory in the instruction's own layout (lane l supplies V[p0 + (l >> 4)][l & 15] and G[2(p0 + (l >> 4)) + s][l & 15]: 16
//   consecutive doubles of 4 rows), each wave over a contiguous quarter of the workgroup's parents; the four waves' tiles
//   are added in wave order through LDS and written as the workgroup's partial.  The workgroup walks its whole block of
//   G_k twice, first for G_{k-1} and then here: the second read comes from a cache only while the block is small (256
//   parents per workgroup up to level 19, 2^(k-11) above), so the traffic counts it as a read of its own.
//   Last level: psi(2p + s) = V_{n-1}[p, :] . A_n[s][:, 0] and the workgroup's partial of Z; a second launch adds the Z
//   partials (every workgroup adds all of them in the same fixed order) and writes q = psi^2 / Z.
// Every long sum is fixed-order partials plus a finishing step (reduce_dev.hpp): no atomics, two calls
// are bitwise equal.  No allocation, no synchronisation (capturable).  Fragment layout of the f64 MFMA as in syrk_f64.hpp.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace bornvi {

namespace {
constexpr int MPS_THREADS = 256;
constexpr int MPS_WAVES = MPS_THREADS / 64;
constexpr int MPS_FUSED = 10;             // levels 1 .. MPS_FUSED (at most 512 parents) share one launch
constexpr long long MPS_MAX_WG = 1024;    // workgroups of a streamed level at most
constexpr long long MPS_Q_PER_WG = 4096;  // entries per workgroup of the elementwise passes over 2^n (at most 1024 workgroups)
constexpr int MPS_MAX_PART = 1024;        // partials of Z and of c at most

typedef double mps_d4 __attribute__((ext_vector_type(4)));
typedef double mps_d2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline bool mps_level_fused(int k, int n) { return k <= MPS_FUSED || (k == n && n <= MPS_FUSED + 1); }
// workgroups (= partials of dA_k, and of Z for k = n) of level k
__host__ __device__ inline long long mps_nwg(int k, int n) {
  if (mps_level_fused(k, n)) return 1;
  const long long w = (1ll << (k - 1)) / MPS_THREADS;
  return w < MPS_MAX_WG ? w : MPS_MAX_WG;
}
__host__ __device__ inline long long mps_part_off(int k, int n, int D) {   // doubles before level k's partials
  long long s = 0;
  for (int j = 1; j < k; ++j) s += mps_nwg(j, n);
  return s * 2 * D * D;
}
__host__ __device__ inline long long mps_voff(int k, int DS) { return (long long)DS * ((1ll << k) - 1); }   // doubles before V_k

ChunkGeom mps_qgeom(long long N) { return chunk_geom(N, MPS_Q_PER_WG, MPS_MAX_PART, 1); }

// G_n[z, 0]
__device__ __forceinline__ double mps_gamma(double psi, double g, double c, double Z) {
  const double t = psi * (g - c);
  return (t + t) / Z;
}

// A_k[s] zero-padded to DP x DP in LDS: As[s][a][b], or its transpose As[s][b][a] (TR)
template <int DP, bool TR>
__device__ __forceinline__ void mps_load_core(const double* cores, int k, int D, double* As) {
  const double* A = cores + (long long)(k - 1) * 2 * D * D;
  for (int i = threadIdx.x; i < 2 * DP * DP; i += MPS_THREADS) {
    const int s = i / (DP * DP), a = (i / DP) % DP, b = i % DP;
    As[TR ? (s * DP + b) * DP + a : i] = (a < D && b < D) ? A[(s * D + a) * D + b] : 0.0;
  }
}

template <int DP>
__device__ __forceinline__ void mps_load_row(const double* row, int DS, double (&v)[DP]) {
#pragma unroll
  for (int j = 0; j < DP / 2; ++j) {
    mps_d2 x = (mps_d2){0.0, 0.0};
    if (2 * j < DS) x = reinterpret_cast<const mps_d2*>(row)[j];
    v[2 * j] = x.x;
    v[2 * j + 1] = x.y;
  }
}

// V_k[2p + s, :] = V_{k-1}[p, :] A_k[s] for the parents [p0, p1).  At: the TRANSPOSED padded cores, At[s][b][a]: the parent row
// stays in registers, the output columns are walked two at a time (the pad rows and columns of At are 0).
template <int DP>
__device__ __forceinline__ void mps_fwd_level(const double* At, const double* Vp, double* Vc, long long p0, long long p1, int DS) {
  for (long long p = p0 + threadIdx.x; p < p1; p += MPS_THREADS) {
    double v[DP];
    mps_load_row<DP>(Vp + p * DS, DS, v);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      double* out = Vc + (2 * p + s) * DS;
#pragma unroll 1
      for (int b = 0; b < DS; b += 2) {
        const double* m0 = At + (s * DP + b) * DP;
        double o0 = 0.0, o1 = 0.0;
#pragma unroll
        for (int j = 0; j < DP / 2; ++j) {
          const mps_d2 x0 = *reinterpret_cast<const mps_d2*>(m0 + 2 * j);
          const mps_d2 x1 = *reinterpret_cast<const mps_d2*>(m0 + DP + 2 * j);
          o0 = fma(v[2 * j], x0.x, o0);
          o1 = fma(v[2 * j], x1.x, o1);
          o0 = fma(v[2 * j + 1], x0.y, o0);
          o1 = fma(v[2 * j + 1], x1.y, o1);
        }
        *reinterpret_cast<mps_d2*>(out + b) = (mps_d2){o0, o1};
      }
    }
  }
}

// psi(2p + s) = V_{n-1}[p, :] . col[s][:] for the parents [p0, p1); returns the thread's sum of psi^2
template <int DP>
__device__ __forceinline__ double mps_psi_level(const double* col /*LDS [2][DP]*/, const double* Vp, double* psi, long long p0,
                                                long long p1, int D, int DS) {
  double z = 0.0;
  for (long long p = p0 + threadIdx.x; p < p1; p += MPS_THREADS) {
    double v[DP];
    mps_load_row<DP>(Vp + p * DS, DS, v);
    double o0 = 0.0, o1 = 0.0;
#pragma unroll
    for (int a = 0; a < DP; ++a) {
      if (a < D) {
        o0 = fma(v[a], col[a], o0);
        o1 = fma(v[a], col[DP + a], o1);
      }
    }
    reinterpret_cast<mps_d2*>(psi)[p] = (mps_d2){o0, o1};
    z = fma(o0, o0, z);
    z = fma(o1, o1, z);
  }
  return z;
}

template <int DP>
__device__ __forceinline__ void mps_load_col(const double* cores, int n, int D, double* col) {
  const double* A = cores + (long long)(n - 1) * 2 * D * D;
  for (int i = threadIdx.x; i < 2 * DP; i += MPS_THREADS) {
    const int s = i / DP, a = i % DP;
    col[i] = a < D ? A[(s * D + a) * D] : 0.0;
  }
}

// G_{k-1}[p, :] = sum_s G_k[2p + s, :] A_k[s]^T for the parents [p0, p1).  TOP (k = n): G_n has column 0 only, made from
// psi and g on the fly.
template <int DP, bool TOP>
__device__ __forceinline__ void mps_bwd_rows(const double* As, const double* Gc, double* Gp, const double* psi, const double* g,
                                             double c, double Z, long long p0, long long p1, int D, int DS) {
  for (long long p = p0 + threadIdx.x; p < p1; p += MPS_THREADS) {
    double* out = Gp + p * DS;
    if (TOP) {
      const mps_d2 ps = reinterpret_cast<const mps_d2*>(psi)[p];
      const double ga0 = mps_gamma(ps.x, g[2 * p], c, Z), ga1 = mps_gamma(ps.y, g[2 * p + 1], c, Z);
#pragma unroll
      for (int j = 0; j < DP / 2; ++j) {
        if (2 * j < DS) {
          mps_d2 o;
          o.x = fma(ga1, As[(DP + 2 * j) * DP], ga0 * As[(2 * j) * DP]);
          o.y = fma(ga1, As[(DP + 2 * j + 1) * DP], ga0 * As[(2 * j + 1) * DP]);
          reinterpret_cast<mps_d2*>(out)[j] = o;
        }
      }
    } else {
      double g0[DP], g1[DP];
      mps_load_row<DP>(Gc + 2 * p * DS, DS, g0);
      mps_load_row<DP>(Gc + (2 * p + 1) * DS, DS, g1);
#pragma unroll 1
      for (int a = 0; a < DS; a += 2) {
        double o[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double* m0 = As + (a + h) * DP;
          const double* m1 = m0 + DP * DP;
          double s0 = 0.0, s1 = 0.0;
#pragma unroll
          for (int b = 0; b < DP / 2; ++b) {
            const mps_d2 x0 = *reinterpret_cast<const mps_d2*>(m0 + 2 * b);
            const mps_d2 x1 = *reinterpret_cast<const mps_d2*>(m1 + 2 * b);
            s0 = fma(g0[2 * b], x0.x, s0);
            s1 = fma(g1[2 * b], x1.x, s1);
            s0 = fma(g0[2 * b + 1], x0.y, s0);
            s1 = fma(g1[2 * b + 1], x1.y, s1);
          }
          o[h] = s0 + s1;
        }
        *reinterpret_cast<mps_d2*>(out + a) = (mps_d2){o[0], o[1]};
      }
    }
  }
}

// The workgroup's partial of dA_k[s][a][b] = sum over its parents [p0, p1) of V_{k-1}[p, a] G_k[2p + s, b] -> part [2][D][D].
// red: LDS [MPS_WAVES][16 NT][16 NT].  Called by every thread of the workgroup (barriers inside).
template <int NT, bool TOP>
__device__ __forceinline__ void mps_bwd_cores(const double* Vp, const double* Gc, const double* psi, const double* g, double c,
                                              double Z, long long p0, long long p1, int D, int DS, double* red, double* part) {
  constexpr int NB = TOP ? 1 : NT;
  constexpr int DM = 16 * NT;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const long long per = (((p1 - p0 + MPS_WAVES - 1) / MPS_WAVES) + 3) & ~3ll;
  const long long w0 = p0 + wave * per;
  const long long w1 = (w0 + per < p1) ? w0 + per : p1;
  mps_d4 acc[2][NT][NB];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
      for (int tb = 0; tb < NB; ++tb) acc[s][ta][tb] = (mps_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (long long pg = w0; pg < w1; pg += 4) {
    const long long p = pg + fk;
    const bool ok = p < w1;
    double a[NT], b[2][NB];
#pragma unroll
    for (int ta = 0; ta < NT; ++ta) {
      const int col = ta * 16 + fr;
      a[ta] = (ok && col < D) ? Vp[p * DS + col] : 0.0;
    }
    if (TOP) {
#pragma unroll
      for (int s = 0; s < 2; ++s) b[s][0] = (ok && fr == 0) ? mps_gamma(psi[2 * p + s], g[2 * p + s], c, Z) : 0.0;
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int tb = 0; tb < NB; ++tb) {
          const int col = tb * 16 + fr;
          b[s][tb] = (ok && col < D) ? Gc[(2 * p + s) * DS + col] : 0.0;
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NB; ++tb)
          acc[s][ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], b[s][tb], acc[s][ta][tb], 0, 0, 0);
  }
  // D[row = fk + 4 r][col = fr] of tile (ta, tb): entry (a = 16 ta + fk + 4 r, b = 16 tb + fr); the waves' tiles in wave order
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    __syncthreads();
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
      for (int tb = 0; tb < NT; ++tb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          red[(wave * DM + ta * 16 + fk + 4 * r) * DM + tb * 16 + fr] = tb < NB ? acc[s][ta][tb < NB ? tb : 0][r] : 0.0;
    __syncthreads();
    for (int e = t; e < DM * DM; e += MPS_THREADS) {
      const int ar = e / DM, bc = e % DM;
      if (ar < D && bc < D)
        part[(s * D + ar) * D + bc] = ((red[e] + red[DM * DM + e]) + red[2 * DM * DM + e]) + red[3 * DM * DM + e];
    }
  }
}

template <int DP>
struct MpsLds {
  static constexpr int NT = DP > 16 ? 2 : 1;
  static constexpr int RED = MPS_WAVES * 256 * NT * NT;
};

// ---- forward ---------------------------------------------------------------------------------------------------
// One workgroup: V_0, the levels 1 .. kmax and, if last, psi and the single partial of Z.
template <int DP>
__global__ __launch_bounds__(MPS_THREADS) void mps_fwd_fused_kernel(const double* cores, int n, int D, int DS, int kmax, int last,
                                                                    double* V, double* psi, double* zpart) {
  __shared__ __attribute__((aligned(16))) double As[2 * DP * DP];
  __shared__ double lds[MPS_WAVES];
  for (int i = threadIdx.x; i < DS; i += MPS_THREADS) V[i] = i == 0 ? 1.0 : 0.0;
  for (int k = 1; k <= kmax; ++k) {
    __syncthreads();
    mps_load_core<DP, true>(cores, k, D, As);
    __syncthreads();
    mps_fwd_level<DP>(As, V + mps_voff(k - 1, DS), V + mps_voff(k, DS), 0, 1ll << (k - 1), DS);
  }
  if (last) {
    __syncthreads();
    mps_load_col<DP>(cores, n, D, As);
    __syncthreads();
    double z = mps_psi_level<DP>(As, V + mps_voff(n - 1, DS), psi, 0, 1ll << (n - 1), D, DS);
    z = block_sum<MPS_WAVES>(z, lds);
    if (threadIdx.x == 0) zpart[0] = z;
  }
}

template <int DP>
__global__ __launch_bounds__(MPS_THREADS) void mps_fwd_level_kernel(const double* __restrict__ cores, int k, int D, int DS,
                                                                    long long chunk, const double* __restrict__ Vp,
                                                                    double* __restrict__ Vc) {
  __shared__ __attribute__((aligned(16))) double As[2 * DP * DP];
  mps_load_core<DP, true>(cores, k, D, As);
  __syncthreads();
  const long long p0 = blockIdx.x * chunk;
  mps_fwd_level<DP>(As, Vp, Vc, p0, p0 + chunk, DS);
}

template <int DP>
__global__ __launch_bounds__(MPS_THREADS) void mps_psi_kernel(const double* __restrict__ cores, int n, int D, int DS, long long chunk,
                                                              const double* __restrict__ Vp, double* __restrict__ psi,
                                                              double* __restrict__ zpart) {
  __shared__ double col[2 * DP];
  __shared__ double lds[MPS_WAVES];
  mps_load_col<DP>(cores, n, D, col);
  __syncthreads();
  const long long p0 = blockIdx.x * chunk;
  double z = mps_psi_level<DP>(col, Vp, psi, p0, p0 + chunk, D, DS);
  z = block_sum<MPS_WAVES>(z, lds);
  if (threadIdx.x == 0) zpart[blockIdx.x] = z;
}

// q = psi^2 / Z (every entry NaN unless Z is positive and finite); workgroup 0 records Z
__global__ __launch_bounds__(MPS_THREADS) void mps_q_kernel(const double* __restrict__ psi, const double* __restrict__ zpart, int nz,
                                                            long long N, long long chunk, double* __restrict__ q64,
                                                            float* __restrict__ q32, double* __restrict__ psi_out,
                                                            double* __restrict__ Z_out, double* __restrict__ hdr) {
  __shared__ double lds[MPS_WAVES];
  const double Z = sum_partials<MPS_THREADS>(zpart, nz, lds);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    hdr[0] = Z;
    if (Z_out) Z_out[0] = Z;
  }
  const bool good = Z > 0.0 && isfinite(Z);
  const long long c0 = blockIdx.x * chunk, c1 = min(N, c0 + chunk);
  for (long long i = c0 + threadIdx.x; i < c1; i += MPS_THREADS) {
    const double ps = psi[i];
    const double q = good ? (ps * ps) / Z : __builtin_nan("");
    q64[i] = q;
    if (q32) q32[i] = (float)q;
    if (psi_out) psi_out[i] = ps;
  }
}

// ---- backward --------------------------------------------------------------------------------------------------
// partials of c = sum_z q_z g_z, q_z = psi_z^2 / Z as mps_q_kernel forms it
__global__ __launch_bounds__(MPS_THREADS) void mps_gstats_kernel(const double* __restrict__ psi, const double* __restrict__ hdr,
                                                                 const double* __restrict__ g, long long N, long long chunk,
                                                                 double* __restrict__ cpart) {
  __shared__ double lds[MPS_WAVES];
  const double Z = hdr[0];
  const bool good = Z > 0.0 && isfinite(Z);
  const long long c0 = blockIdx.x * chunk, c1 = min(N, c0 + chunk);
  double v = 0.0;
  for (long long i = c0 + threadIdx.x; i < c1; i += MPS_THREADS) {
    const double ps = psi[i];
    const double q = good ? (ps * ps) / Z : __builtin_nan("");
    v = fma(q, g[i], v);
  }
  v = block_sum<MPS_WAVES>(v, lds);
  if (threadIdx.x == 0) cpart[blockIdx.x] = v;
}

// One workgroup: the levels ktop .. 1 (ktop = n: the top level too).  G_k lives in Ga when n - 1 - k is even, else in Gb.
template <int DP>
__global__ __launch_bounds__(MPS_THREADS) void mps_bwd_fused_kernel(const double* cores, int n, int D, int DS, int ktop,
                                                                    const double* V, const double* psi, const double* hdr,
                                                                    const double* g, const double* cpart, int nc, double* Ga,
                                                                    double* Gb, double* parts) {
  constexpr int NT = MpsLds<DP>::NT;
  __shared__ __attribute__((aligned(16))) double As[2 * DP * DP];
  __shared__ double red[MpsLds<DP>::RED];
  __shared__ double lds[MPS_WAVES];
  double c = 0.0, Z = 1.0;
  if (ktop == n) {
    c = sum_partials<MPS_THREADS>(cpart, nc, lds);
    Z = hdr[0];
  }
  for (int k = ktop; k >= 1; --k) {
    __syncthreads();
    mps_load_core<DP, false>(cores, k, D, As);
    __syncthreads();
    const double* Gc = ((n - 1 - k) & 1) ? Gb : Ga;     // (k = n: not read)
    double* Gp = ((n - k) & 1) ? Gb : Ga;
    const double* Vp = V + mps_voff(k - 1, DS);
    const long long P = 1ll << (k - 1);
    double* part = parts + mps_part_off(k, n, D);
    if (k == n) {
      if (k > 1) mps_bwd_rows<DP, true>(As, nullptr, Gp, psi, g, c, Z, 0, P, D, DS);
      mps_bwd_cores<NT, true>(Vp, nullptr, psi, g, c, Z, 0, P, D, DS, red, part);
    } else {
      if (k > 1) mps_bwd_rows<DP, false>(As, Gc, Gp, nullptr, nullptr, 0.0, 1.0, 0, P, D, DS);
      mps_bwd_cores<NT, false>(Vp, Gc, nullptr, nullptr, 0.0, 1.0, 0, P, D, DS, red, part);
    }
  }
}

template <int DP, bool TOP>
__global__ __launch_bounds__(MPS_THREADS) void mps_bwd_level_kernel(const double* __restrict__ cores, int k, int D, int DS,
                                                                    long long chunk, const double* __restrict__ Vp,
                                                                    const double* __restrict__ Gc, double* __restrict__ Gp,
                                                                    const double* __restrict__ psi, const double* __restrict__ hdr,
                                                                    const double* __restrict__ g, const double* __restrict__ cpart,
                                                                    int nc, double* __restrict__ part) {
  constexpr int NT = MpsLds<DP>::NT;
  __shared__ __attribute__((aligned(16))) double As[2 * DP * DP];
  __shared__ double red[MpsLds<DP>::RED];
  __shared__ double lds[MPS_WAVES];
  double c = 0.0, Z = 1.0;
  if (TOP) {
    c = sum_partials<MPS_THREADS>(cpart, nc, lds);
    Z = hdr[0];
  }
  mps_load_core<DP, false>(cores, k, D, As);
  __syncthreads();
  const long long p0 = blockIdx.x * chunk;
  mps_bwd_rows<DP, TOP>(As, Gc, Gp, psi, g, c, Z, p0, p0 + chunk, D, DS);
  mps_bwd_cores<NT, TOP>(Vp, Gc, psi, g, c, Z, p0, p0 + chunk, D, DS, red, part + (long long)blockIdx.x * 2 * D * D);
}

// grid (n, ceil(2 D^2 / 64)): grad_cores[k - 1] = level k's partials added in a fixed order: four contiguous quarters of the
// workgroups, one per wave of this block, each in index order, then the quarters in order.
__global__ __launch_bounds__(MPS_THREADS) void mps_finish_kernel(const double* __restrict__ parts, int n, int D,
                                                                 double* __restrict__ grad) {
  __shared__ double sl[MPS_THREADS];
  const int k = blockIdx.x + 1;
  const int E = 2 * D * D;
  const int e = blockIdx.y * 64 + (threadIdx.x & 63), slice = threadIdx.x >> 6;
  const long long nwg = mps_nwg(k, n);
  const double* __restrict__ pk = parts + mps_part_off(k, n, D);
  const long long per = (nwg + MPS_WAVES - 1) / MPS_WAVES;
  const long long j0 = slice * per, j1 = min(nwg, j0 + per);
  double v = 0.0;
  if (e < E)
    for (long long j = j0; j < j1; ++j) v += pk[j * E + e];
  sl[threadIdx.x] = v;
  __syncthreads();
  if (slice == 0 && e < E) {
    const int t = threadIdx.x;
    grad[(long long)(k - 1) * E + e] = ((sl[t] + sl[64 + t]) + sl[128 + t]) + sl[192 + t];
  }
}

struct MpsLayout {
  int DP, DS;
  size_t hdr, zpart, cpart, psi, V, Ga, Gb, parts, total;   // byte offsets from the aligned base
};

MpsLayout mps_layout(int n, int D) {
  MpsLayout L;
  L.DP = bond_dp(D);
  L.DS = (D + 1) & ~1;
  const size_t N = (size_t)1 << n;
  size_t o = 0;
  L.hdr = o;   o += 256;
  L.zpart = o; o += ws_round(MPS_MAX_PART * sizeof(double));
  L.cpart = o; o += ws_round(MPS_MAX_PART * sizeof(double));
  L.psi = o;   o += ws_round(N * sizeof(double));
  L.V = o;     o += ws_round((size_t)L.DS * (N - 1) * sizeof(double) + 16);           // V_0 .. V_{n-1}
  L.Ga = o;    o += ws_round((size_t)L.DS * (N / 2) * sizeof(double) + 16);           // G_{n-1}, G_{n-3}, ...
  L.Gb = o;    o += ws_round((size_t)L.DS * (N / 4) * sizeof(double) + 16);           // G_{n-2}, G_{n-4}, ...
  L.parts = o; o += ws_round((size_t)mps_part_off(n + 1, n, D) * sizeof(double));
  L.total = o;
  return L;
}
}  // namespace

size_t mps_workspace_bytes(int n, int D) { return mps_layout(n, D).total + 256; }

hipError_t launch_mps_probs(int n, int D, const double* cores, double* q64, float* q32, double* psi_out, double* Z_out, void* ws,
                            hipStream_t st) {
  const MpsLayout L = mps_layout(n, D);
  char* base = ws_align(ws);
  double* hdr = (double*)(base + L.hdr);
  double* zpart = (double*)(base + L.zpart);
  double* psi = (double*)(base + L.psi);
  double* V = (double*)(base + L.V);
  const int DS = L.DS;
  const int kmax = (n - 1 < MPS_FUSED) ? n - 1 : MPS_FUSED;
  const int last = mps_level_fused(n, n) ? 1 : 0;
  BOND_DISPATCH(L.DP, (mps_fwd_fused_kernel<DP><<<1, MPS_THREADS, 0, st>>>(cores, n, D, DS, kmax, last, V, psi, zpart)));
  for (int k = kmax + 1; k <= n - 1; ++k) {
    const long long nwg = mps_nwg(k, n), chunk = (1ll << (k - 1)) / nwg;
    BOND_DISPATCH(L.DP, (mps_fwd_level_kernel<DP><<<(unsigned)nwg, MPS_THREADS, 0, st>>>(cores, k, D, DS, chunk, V + mps_voff(k - 1, DS),
                                                                                       V + mps_voff(k, DS))));
  }
  const long long nz = mps_nwg(n, n);
  if (!last) {
    const long long chunk = (1ll << (n - 1)) / nz;
    BOND_DISPATCH(L.DP, (mps_psi_kernel<DP><<<(unsigned)nz, MPS_THREADS, 0, st>>>(cores, n, D, DS, chunk, V + mps_voff(n - 1, DS), psi,
                                                                                zpart)));
  }
  const long long N = 1ll << n;
  const ChunkGeom qg = mps_qgeom(N);
  mps_q_kernel<<<(unsigned)qg.G, MPS_THREADS, 0, st>>>(psi, zpart, (int)nz, N, qg.chunk, q64, q32, psi_out, Z_out, hdr);
  return hipGetLastError();
}

hipError_t launch_mps_vjp(int n, int D, const double* cores, const double* g, double* grad_cores, void* ws, hipStream_t st) {
  const MpsLayout L = mps_layout(n, D);
  char* base = ws_align(ws);
  const double* hdr = (const double*)(base + L.hdr);
  double* cpart = (double*)(base + L.cpart);
  const double* psi = (const double*)(base + L.psi);
  const double* V = (const double*)(base + L.V);
  double* Ga = (double*)(base + L.Ga);
  double* Gb = (double*)(base + L.Gb);
  double* parts = (double*)(base + L.parts);
  const int DS = L.DS;
  const long long N = 1ll << n;
  const ChunkGeom qg = mps_qgeom(N);
  mps_gstats_kernel<<<(unsigned)qg.G, MPS_THREADS, 0, st>>>(psi, hdr, g, N, qg.chunk, cpart);
  int k = n;
  for (; k >= 1 && !mps_level_fused(k, n); --k) {
    const long long nwg = mps_nwg(k, n), chunk = (1ll << (k - 1)) / nwg;
    const double* Gc = ((n - 1 - k) & 1) ? Gb : Ga;
    double* Gp = ((n - k) & 1) ? Gb : Ga;
    double* part = parts + mps_part_off(k, n, D);
    if (k == n) {
      BOND_DISPATCH(L.DP, (mps_bwd_level_kernel<DP, true><<<(unsigned)nwg, MPS_THREADS, 0, st>>>(
                             cores, k, D, DS, chunk, V + mps_voff(k - 1, DS), nullptr, Gp, psi, hdr, g, cpart, qg.G, part)));
    } else {
      BOND_DISPATCH(L.DP, (mps_bwd_level_kernel<DP, false><<<(unsigned)nwg, MPS_THREADS, 0, st>>>(
                             cores, k, D, DS, chunk, V + mps_voff(k - 1, DS), Gc, Gp, nullptr, nullptr, nullptr, nullptr, 0, part)));
    }
  }
  BOND_DISPATCH(L.DP, (mps_bwd_fused_kernel<DP><<<1, MPS_THREADS, 0, st>>>(cores, n, D, DS, k, V, psi, hdr, g, cpart, qg.G, Ga, Gb, parts)));
  mps_finish_kernel<<<dim3((unsigned)n, (unsigned)((2 * D * D + 63) / 64)), MPS_THREADS, 0, st>>>(parts, n, D, grad_cores);
  return hipGetLastError();
}

}  // namespace bornvi
