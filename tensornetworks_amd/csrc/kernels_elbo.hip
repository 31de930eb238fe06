// Exact ELBO (reverse KL) of a Born distribution against a tabulated log-joint (bornvi_elbo_weights): the piece between
// "q is known" and "the gradient engine needs dL/dq" of an ELBO training step, for both Born-machine families.
//
// Per row of q (float64, N = 2^n entries; log_p is shared by all rows), with l_z = log max(q_z, q_floor):
//   w_z      = l_z - log_p_z + [q_z >= q_floor]         = dL/dq_z (the derivative of q log max(q, floor): the clamp passes
//                                                          no gradient below the floor, as in kernels_born_table.hip)
//   neg_elbo = sum_z q_z (l_z - log_p_z)                 (a term with q_z == 0 is exactly 0, whatever log_p_z is)
//   entropy  = -sum_z q_z l_z
// One read of q, one read of log_p, one write of w: 24 bytes per entry, memory-bound.
//
// Reductions as in kernels_born_table.hip, in the fixed order of reduce_dev.hpp: each of the G
// workgroups of a row adds its contiguous chunk (at most 16 entries per thread) and writes its two partials to the
// workspace; a finishing launch adds a row's G partials in the same fixed way.  256-thread workgroups (four waves of 64),
// double2 accesses where the pointers allow them.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace bornvi {

namespace {
constexpr int EL_THREADS = 256;
constexpr int EL_WAVES = EL_THREADS / 64;
constexpr long long EL_PER_WG = 4096;     // target entries per workgroup: 16 per thread
constexpr long long EL_MAX_WG = 1024;     // workgroups per row at most (n > 22: longer chunks)

// a row's workgroups: chunks of a multiple of 4 entries
ChunkGeom el_geom(long long N) { return chunk_geom(N, EL_PER_WG, EL_MAX_WG, 4); }

// One entry: returns w, adds the entry's loss and q log c terms.  The clamp is written so that a NaN q stays NaN.
__device__ __forceinline__ double elbo_entry(double q, double lp, double q_floor, double& loss, double& qlogq) {
  const double c = (q < q_floor) ? q_floor : q;
  const double l = log(c);
  const double d = l - lp;
  if (q != 0.0) {
    loss += q * d;
    qlogq += q * l;
  }
  return d + (q >= q_floor ? 1.0 : 0.0);
}

// grid (G, rows): w and the two partials of a chunk.  part[(row * G + g) * 2 + {0, 1}] = (loss, sum q log c).
__global__ __launch_bounds__(EL_THREADS) void elbo_weights_kernel(const double* __restrict__ q, const double* __restrict__ log_p,
                                                                  long long N, long long chunk, int vec, double q_floor,
                                                                  double* __restrict__ w, double* __restrict__ part) {
  __shared__ double lds[EL_WAVES];
  const long long row = blockIdx.y, g = blockIdx.x;
  const double* __restrict__ qr = q + row * N;
  double* __restrict__ wr = w ? w + row * N : nullptr;
  const long long c0 = g * chunk, c1 = min(N, c0 + chunk);
  double loss = 0.0, qlogq = 0.0;
  if (vec) {      // (N and the chunk are even)
    for (long long i = c0 / 2 + threadIdx.x; i < c1 / 2; i += EL_THREADS) {
      const double2 a = reinterpret_cast<const double2*>(qr)[i];
      const double2 p = reinterpret_cast<const double2*>(log_p)[i];
      double2 o;
      o.x = elbo_entry(a.x, p.x, q_floor, loss, qlogq);
      o.y = elbo_entry(a.y, p.y, q_floor, loss, qlogq);
      if (wr) reinterpret_cast<double2*>(wr)[i] = o;
    }
  } else {        // the same pairs per thread in the same order (N = 2^n, n >= 1, and the chunk are even): the sums' bits do not
                  // depend on where the caller's buffers lie
    for (long long i = c0 / 2 + threadIdx.x; i < c1 / 2; i += EL_THREADS) {
      const double o0 = elbo_entry(qr[2 * i], log_p[2 * i], q_floor, loss, qlogq);
      const double o1 = elbo_entry(qr[2 * i + 1], log_p[2 * i + 1], q_floor, loss, qlogq);
      if (wr) {
        wr[2 * i] = o0;
        wr[2 * i + 1] = o1;
      }
    }
  }
  loss = block_sum<EL_WAVES>(loss, lds);
  qlogq = block_sum<EL_WAVES>(qlogq, lds);
  if (threadIdx.x == 0) {
    double* p = part + 2 * (row * gridDim.x + g);
    p[0] = loss;
    p[1] = qlogq;
  }
}

// grid (rows): neg_elbo[row] = sum of the row's loss partials, entropy[row] = -(sum of its q log c partials).
__global__ __launch_bounds__(EL_THREADS) void elbo_finish_kernel(const double* __restrict__ part, int G,
                                                                 double* __restrict__ neg_elbo, double* __restrict__ entropy) {
  __shared__ double lds[EL_WAVES];
  const double* __restrict__ pr = part + 2 * (long long)blockIdx.x * G;
  double loss = 0.0, qlogq = 0.0;
  for (int k = threadIdx.x; k < G; k += EL_THREADS) {
    loss += pr[2 * k];
    qlogq += pr[2 * k + 1];
  }
  loss = block_sum<EL_WAVES>(loss, lds);
  qlogq = block_sum<EL_WAVES>(qlogq, lds);
  if (threadIdx.x == 0) {
    neg_elbo[blockIdx.x] = loss;
    if (entropy) entropy[blockIdx.x] = -qlogq;
  }
}

}  // namespace

size_t elbo_workspace_bytes(int n, long long rows) {
  const ChunkGeom gm = el_geom(1ll << n);
  return (size_t)rows * gm.G * 2 * sizeof(double) + 512;
}

hipError_t launch_elbo_weights(int n, long long rows, const double* q, const double* log_p, double q_floor, double* w,
                               double* neg_elbo, double* entropy, void* ws, hipStream_t st) {
  const long long N = 1ll << n;
  const ChunkGeom gm = el_geom(N);
  const int vec = (N % 2 == 0) && ((((uintptr_t)q) | ((uintptr_t)log_p) | ((uintptr_t)w)) & 15) == 0;
  double* part = (double*)ws_align(ws);
  elbo_weights_kernel<<<dim3((unsigned)gm.G, (unsigned)rows), EL_THREADS, 0, st>>>(q, log_p, N, gm.chunk, vec, q_floor, w, part);
  elbo_finish_kernel<<<dim3((unsigned)rows), EL_THREADS, 0, st>>>(part, gm.G, neg_elbo, entropy);
  return hipGetLastError();
}

}  // namespace bornvi
