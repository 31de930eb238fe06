// Classical Born machine: the per-epoch kernels of the probability-table family (bornvi_born_table_probs / _vjp).
//
// A row of raw parameters w (float32, N = 2^n entries) becomes the Born distribution
//   mode 0 (use_logits):  q = softmax(w - max w)           mode 1:  q = |w| / sum |w|
// returned as float32 q32 plus its exact float64 upcast q64 (the KSD contraction runs on q32 in float64), and optionally
// the entropy H = -sum q log max(q, 1e-10) over q32.  The VJP maps the gradient of
//   L = sqrt(max(ksd2, 1e-12)) - lambda H          (either term may be absent)
// with respect to q back onto w: dL/dq = y / L (0 where the clamp is active; y = K_p q) + lambda (log c + [q >= 1e-10]),
// c = max(q, 1e-10); then the softmax VJP q (g - sum q g), or for mode 1 sign(w) (g - sum q g) / sum |w| (sign(0) = 0).
//
// Every reduction over a row is two-level and in the fixed order of reduce_dev.hpp: each of the G
// workgroups of a row writes its partial to the workspace, the next kernel reduces the row's G partials (each workgroup
// redundantly, in the same order).  256-thread workgroups (four waves of 64), grid-stride over a contiguous chunk of the
// row with float4 loads where the row allows them.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace bornvi {

namespace {
constexpr int BT_THREADS = 256;
constexpr int BT_WAVES = BT_THREADS / 64;
constexpr long long BT_PER_WG = 4096;     // target entries per workgroup
constexpr long long BT_MAX_WG = 1024;     // workgroups per row at most
constexpr float BT_CLAMP = 1e-10f;        // the reference's clamp(min=1e-10) on a float32 tensor

// a row's workgroups: chunks of a multiple of 4 entries
ChunkGeom bt_geom(long long N) { return chunk_geom(N, BT_PER_WG, BT_MAX_WG, 4); }

// Online (max, sum of exp(w - max)) pair.  Symmetric in its two arguments (so the shuffle butterfly gives every lane the
// same value) and NaN-sticky (a NaN logit reaches every q, as in torch.softmax).
__device__ __forceinline__ void sm_combine(float& M, double& S, float m, double s) {
  if (m != m || M != M || s != s || S != S) {
    M = NAN;
    S = NAN;
    return;
  }
  if (s == 0.0) return;
  if (S == 0.0) {
    M = m;
    S = s;
    return;
  }
  if (m > M) {
    S = S * exp((double)M - (double)m) + s;
    M = m;
  } else {
    S += s * exp((double)m - (double)M);
  }
}

__device__ __forceinline__ void block_softmax_stats(float& M, double& S, float* ldsm, double* ldss) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float m2 = __shfl_xor(M, off);
    const double s2 = __shfl_xor(S, off);
    sm_combine(M, S, m2, s2);
  }
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) {
    ldsm[t >> 6] = M;
    ldss[t >> 6] = S;
  }
  __syncthreads();
  M = -INFINITY;
  S = 0.0;
#pragma unroll
  for (int i = 0; i < BT_WAVES; ++i) sm_combine(M, S, ldsm[i], ldss[i]);
}

// Row statistics from the G partials (each an (M, S) pair; mode 1 uses S only), reduced in a fixed order.
__device__ __forceinline__ void row_stats(const double* __restrict__ part, int G, int mode, float& M, double& S, float* ldsm,
                                          double* ldss) {
  const int t = threadIdx.x;
  if (mode == 0) {
    M = -INFINITY;
    S = 0.0;
    for (int k = t; k < G; k += BT_THREADS) sm_combine(M, S, (float)part[2 * k], part[2 * k + 1]);
    block_softmax_stats(M, S, ldsm, ldss);
  } else {
    double s = 0.0;      // (this loop and the entropy kernel's are sum_partials written out: reduce_dev.hpp says why)
    for (int k = t; k < G; k += BT_THREADS) s += part[2 * k + 1];
    M = 0.0f;
    S = block_sum<BT_WAVES>(s, ldss);
  }
}

__device__ __forceinline__ void elem_stats(float v, int mode, float& M, double& S) {
  if (mode == 0) sm_combine(M, S, v, v == -INFINITY ? 0.0 : 1.0);
  else S += (double)fabsf(v);
}

// pass 1 of bornvi_born_table_probs: per (chunk, row) the softmax pair or the sum of |w|.  grid (G, rows).
__global__ __launch_bounds__(BT_THREADS) void born_table_stats_kernel(const float* __restrict__ w, long long N, long long chunk,
                                                                      int mode, int vec, double* __restrict__ part) {
  __shared__ float ldsm[BT_WAVES];
  __shared__ double ldss[BT_WAVES];
  const long long row = blockIdx.y, g = blockIdx.x;
  const float* __restrict__ wr = w + row * N;
  const long long c0 = g * chunk, c1 = min(N, c0 + chunk);
  float M = -INFINITY;
  double S = 0.0;
  if (vec) {
    for (long long i = c0 / 4 + threadIdx.x; i < c1 / 4; i += BT_THREADS) {
      const float4 v = reinterpret_cast<const float4*>(wr)[i];
      elem_stats(v.x, mode, M, S);
      elem_stats(v.y, mode, M, S);
      elem_stats(v.z, mode, M, S);
      elem_stats(v.w, mode, M, S);
    }
  } else {
    for (long long i = c0 + threadIdx.x; i < c1; i += BT_THREADS) elem_stats(wr[i], mode, M, S);
  }
  if (mode == 0) {
    block_softmax_stats(M, S, ldsm, ldss);
  } else {
    S = block_sum<BT_WAVES>(S, ldss);
  }
  if (threadIdx.x == 0) {
    double* p = part + 2 * (row * gridDim.x + g);
    p[0] = (double)M;
    p[1] = S;
  }
}

__device__ __forceinline__ float table_q(float v, int mode, float M, double S) {
  return mode == 0 ? (float)(exp((double)v - (double)M) / S) : (float)((double)fabsf(v) / S);
}

// q log max(q, 1e-10) of one float32 probability (the clamp is written so that a NaN stays NaN, as in torch.clamp)
__device__ __forceinline__ double plogp(float q) {
  const float c = (q < BT_CLAMP) ? BT_CLAMP : q;
  return (double)q * log((double)c);
}

// pass 2: q32, q64 and the entropy partials.  grid (G, rows).
__global__ __launch_bounds__(BT_THREADS) void born_table_probs_kernel(const float* __restrict__ w, long long N, long long chunk,
                                                                      int mode, int vec, const double* __restrict__ part,
                                                                      float* __restrict__ q32, double* __restrict__ q64,
                                                                      double* __restrict__ hpart) {
  __shared__ float ldsm[BT_WAVES];
  __shared__ double ldss[BT_WAVES];
  const long long row = blockIdx.y, g = blockIdx.x;
  const int G = gridDim.x;
  float M;
  double S;
  row_stats(part + 2 * row * G, G, mode, M, S, ldsm, ldss);
  const float* __restrict__ wr = w + row * N;
  float* __restrict__ qr = q32 + row * N;
  double* __restrict__ dr = q64 + row * N;
  const long long c0 = g * chunk, c1 = min(N, c0 + chunk);
  double h = 0.0;
  if (vec) {
    for (long long i = c0 / 4 + threadIdx.x; i < c1 / 4; i += BT_THREADS) {
      const float4 v = reinterpret_cast<const float4*>(wr)[i];
      const float4 q = make_float4(table_q(v.x, mode, M, S), table_q(v.y, mode, M, S), table_q(v.z, mode, M, S),
                                   table_q(v.w, mode, M, S));
      reinterpret_cast<float4*>(qr)[i] = q;
      reinterpret_cast<double2*>(dr)[2 * i] = make_double2((double)q.x, (double)q.y);
      reinterpret_cast<double2*>(dr)[2 * i + 1] = make_double2((double)q.z, (double)q.w);
      if (hpart) h += plogp(q.x) + plogp(q.y) + plogp(q.z) + plogp(q.w);
    }
  } else {
    for (long long i = c0 + threadIdx.x; i < c1; i += BT_THREADS) {
      const float q = table_q(wr[i], mode, M, S);
      qr[i] = q;
      dr[i] = (double)q;
      if (hpart) h += plogp(q);
    }
  }
  if (hpart) {
    h = block_sum<BT_WAVES>(h, ldss);
    if (threadIdx.x == 0) hpart[row * G + g] = h;
  }
}

// pass 3 (only when H is asked for): H[row] = -(sum of the row's entropy partials).  grid (rows).
__global__ __launch_bounds__(BT_THREADS) void born_table_entropy_kernel(const double* __restrict__ hpart, int G,
                                                                        float* __restrict__ H) {
  __shared__ double ldss[BT_WAVES];
  const long long row = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < G; k += BT_THREADS) s += hpart[row * G + k];
  s = block_sum<BT_WAVES>(s, ldss);
  if (threadIdx.x == 0) H[row] = (float)(-s);
}

// dL/dq of one entry: the KSD term (y / loss, rounded to float32 as the backward of the float64 upcast rounds it) plus
// the entropy term lambda (log c + [q >= 1e-10]) of -lambda H (the clamp passes no gradient below 1e-10).
__device__ __forceinline__ double dl_dq(double q, const double* __restrict__ yr, long long i, double a, double lam) {
  double g = yr ? (double)(float)(yr[i] * a) : 0.0;
  if (lam != 0.0) {
    const float qf = (float)q;
    const float c = (qf < BT_CLAMP) ? BT_CLAMP : qf;
    g += lam * (log((double)c) + (qf >= BT_CLAMP ? 1.0 : 0.0));
  }
  return g;
}

// d loss / d ksd2 times 2: 1 / sqrt(ksd2), 0 where the clamp at 1e-12 is active; 1 when y is dL/dq itself (no ksd2)
__device__ __forceinline__ double ksd_scale(const double* __restrict__ ksd2, long long row) {
  if (!ksd2) return 1.0;
  const double k2 = ksd2[row];
  return (k2 < 1e-12) ? 0.0 : 1.0 / sqrt(k2);
}

// VJP pass 1: per (chunk, row) sum q g and (mode 1) sum |w|.  grid (G, rows).
__global__ __launch_bounds__(BT_THREADS) void born_table_vjp_stats_kernel(const float* __restrict__ w,
                                                                          const double* __restrict__ q64,
                                                                          const double* __restrict__ y,
                                                                          const double* __restrict__ ksd2, double lam,
                                                                          long long N, long long chunk, int mode, int vec,
                                                                          double* __restrict__ part) {
  __shared__ double ldss[BT_WAVES];
  const long long row = blockIdx.y, g = blockIdx.x;
  const double a = ksd_scale(ksd2, row);
  const float* __restrict__ wr = w + row * N;
  const double* __restrict__ qr = q64 + row * N;
  const double* __restrict__ yr = y ? y + row * N : nullptr;
  const long long c0 = g * chunk, c1 = min(N, c0 + chunk);
  double sqg = 0.0, sw = 0.0;
  if (vec) {
    for (long long i = c0 / 4 + threadIdx.x; i < c1 / 4; i += BT_THREADS) {
      const double2 qa = reinterpret_cast<const double2*>(qr)[2 * i], qb = reinterpret_cast<const double2*>(qr)[2 * i + 1];
      sqg += qa.x * dl_dq(qa.x, yr, 4 * i, a, lam) + qa.y * dl_dq(qa.y, yr, 4 * i + 1, a, lam) +
             qb.x * dl_dq(qb.x, yr, 4 * i + 2, a, lam) + qb.y * dl_dq(qb.y, yr, 4 * i + 3, a, lam);
      if (mode == 1) {
        const float4 v = reinterpret_cast<const float4*>(wr)[i];
        sw += (double)fabsf(v.x) + (double)fabsf(v.y) + (double)fabsf(v.z) + (double)fabsf(v.w);
      }
    }
  } else {
    for (long long i = c0 + threadIdx.x; i < c1; i += BT_THREADS) {
      sqg += qr[i] * dl_dq(qr[i], yr, i, a, lam);
      if (mode == 1) sw += (double)fabsf(wr[i]);
    }
  }
  sqg = block_sum<BT_WAVES>(sqg, ldss);
  if (mode == 1) sw = block_sum<BT_WAVES>(sw, ldss);
  if (threadIdx.x == 0) {
    double* p = part + 2 * (row * gridDim.x + g);
    p[0] = sqg;
    p[1] = sw;
  }
}

// one entry of dL/dw: softmax q (g - c); mode 1 sign(w) (g - c) / sum |w| with torch's sign (0 at 0)
__device__ __forceinline__ float vjp_entry(float wv, double q, double gq, double c, int mode, double inv_s) {
  if (mode == 0) return (float)(q * (gq - c));
  const double sg = (double)((wv > 0.0f) - (wv < 0.0f));
  return (float)(sg * (gq - c) * inv_s);
}

// VJP pass 2: grad[row] and loss[row].  grid (G, rows).
__global__ __launch_bounds__(BT_THREADS) void born_table_vjp_kernel(const float* __restrict__ w, const double* __restrict__ q64,
                                                                    const double* __restrict__ y,
                                                                    const double* __restrict__ ksd2, double lam, long long N,
                                                                    long long chunk, int mode, int vec,
                                                                    const double* __restrict__ part, float* __restrict__ grad,
                                                                    double* __restrict__ loss_out) {
  __shared__ double ldss[BT_WAVES];
  const long long row = blockIdx.y, g = blockIdx.x;
  const int G = gridDim.x;
  const double* __restrict__ pr = part + 2 * row * G;
  double c = 0.0, sw = 0.0;
  for (int k = threadIdx.x; k < G; k += BT_THREADS) {
    c += pr[2 * k];
    sw += pr[2 * k + 1];
  }
  c = block_sum<BT_WAVES>(c, ldss);
  if (mode == 1) sw = block_sum<BT_WAVES>(sw, ldss);
  const double inv_s = 1.0 / sw;
  const double a = ksd_scale(ksd2, row);
  const float* __restrict__ wr = w + row * N;
  const double* __restrict__ qr = q64 + row * N;
  const double* __restrict__ yr = y ? y + row * N : nullptr;
  float* __restrict__ gr = grad + row * N;
  const long long c0 = g * chunk, c1 = min(N, c0 + chunk);
  if (vec) {
    for (long long i = c0 / 4 + threadIdx.x; i < c1 / 4; i += BT_THREADS) {
      const double2 qa = reinterpret_cast<const double2*>(qr)[2 * i], qb = reinterpret_cast<const double2*>(qr)[2 * i + 1];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (mode == 1) v = reinterpret_cast<const float4*>(wr)[i];
      float4 o;
      o.x = vjp_entry(v.x, qa.x, dl_dq(qa.x, yr, 4 * i, a, lam), c, mode, inv_s);
      o.y = vjp_entry(v.y, qa.y, dl_dq(qa.y, yr, 4 * i + 1, a, lam), c, mode, inv_s);
      o.z = vjp_entry(v.z, qb.x, dl_dq(qb.x, yr, 4 * i + 2, a, lam), c, mode, inv_s);
      o.w = vjp_entry(v.w, qb.y, dl_dq(qb.y, yr, 4 * i + 3, a, lam), c, mode, inv_s);
      reinterpret_cast<float4*>(gr)[i] = o;
    }
  } else {
    for (long long i = c0 + threadIdx.x; i < c1; i += BT_THREADS)
      gr[i] = vjp_entry(mode == 1 ? wr[i] : 0.0f, qr[i], dl_dq(qr[i], yr, i, a, lam), c, mode, inv_s);
  }
  if (loss_out && ksd2 && g == 0 && threadIdx.x == 0) {
    const double k2 = ksd2[row];
    loss_out[row] = sqrt(k2 < 1e-12 ? 1e-12 : k2);
  }
}

}  // namespace

size_t born_table_workspace_bytes(int n, long long rows) {
  const ChunkGeom gm = bt_geom(1ll << n);
  return (size_t)rows * gm.G * 3 * sizeof(double) + 512;
}

hipError_t launch_born_table_probs(int n, long long rows, int mode, const float* w, float* q32, double* q64, float* H,
                                   void* ws, hipStream_t st) {
  const long long N = 1ll << n;
  const ChunkGeom gm = bt_geom(N);
  const int vec = (N % 4 == 0) && ((((uintptr_t)w) | ((uintptr_t)q32) | ((uintptr_t)q64)) & 15) == 0;
  double* part = (double*)ws_align(ws);
  double* hpart = H ? part + 2 * rows * gm.G : nullptr;
  const dim3 grid((unsigned)gm.G, (unsigned)rows);
  born_table_stats_kernel<<<grid, BT_THREADS, 0, st>>>(w, N, gm.chunk, mode, vec, part);
  born_table_probs_kernel<<<grid, BT_THREADS, 0, st>>>(w, N, gm.chunk, mode, vec, part, q32, q64, hpart);
  if (H) born_table_entropy_kernel<<<dim3((unsigned)rows), BT_THREADS, 0, st>>>(hpart, gm.G, H);
  return hipGetLastError();
}

hipError_t launch_born_table_vjp(int n, long long rows, int mode, const float* w, const double* q64, const double* y,
                                 const double* ksd2, double lam, float* grad, double* loss_out, void* ws, hipStream_t st) {
  const long long N = 1ll << n;
  const ChunkGeom gm = bt_geom(N);
  const int vec = (N % 4 == 0) &&
                  ((((uintptr_t)w) | ((uintptr_t)q64) | ((uintptr_t)y) | ((uintptr_t)grad)) & 15) == 0;
  double* part = (double*)ws_align(ws);
  const dim3 grid((unsigned)gm.G, (unsigned)rows);
  born_table_vjp_stats_kernel<<<grid, BT_THREADS, 0, st>>>(w, q64, y, ksd2, lam, N, gm.chunk, mode, vec, part);
  born_table_vjp_kernel<<<grid, BT_THREADS, 0, st>>>(w, q64, y, ksd2, lam, N, gm.chunk, mode, vec, part, grad, loss_out);
  return hipGetLastError();
}

}  // namespace bornvi
