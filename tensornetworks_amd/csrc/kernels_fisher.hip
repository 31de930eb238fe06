// Natural-gradient pieces (gfx950): the classical Fisher matrix of a Born distribution from the stored parameter-shift
// rows (bornvi_fisher_gram) and the damped Cholesky solve of the natural-gradient step (bornvi_spd_solve).
//
// ---- bornvi_fisher_gram: F_ab = sum_z d_a(z) d_b(z) r_z,  d_a = 1/2 (row_{2a} - row_{2a+1}),  r_z = 1/q_z where
// q_z >= q_floor, else 0 (a state under the floor contributes nothing: both factors of its products are stored as 0).
// The split-K SYRK of syrk_f64.hpp (layout, barriers, order of the sums: there) over P rows of N = 2^n columns, with
//   output tile 64 x 64 (a wave owns 32 x 32 = 2 x 2 MFMA tiles: 32 accumulator VGPRs);
//   what goes into LDS: per slab the reciprocals r_z, once (one IEEE division per entry and slab, not per k-step); on the
//   way into the tiles the thread forms d (one subtraction, the halving is exact) and stores e = d r on the row side (As)
//   and d on the column side (Bs): ONE side is scaled, so a product e_a d_b carries the roundings of d_a, d_b, r, e and
//   the product itself (C_TERM = 5 half-units; tests/test_gpu_fisher_kernel.py); 8 16-byte loads of rows and none of q
//   per thread and k-step;
//   the running total over a workgroup's slabs in 32 more VGPRs;
//   LDS: 32 KiB of r + 36 KiB of tiles = 68 KiB (two workgroups per CU); no scratch (build.py holds the budget).
// Inside a diagonal tile only the entries a <= b are used; fisher_finish_kernel writes F_ab and F_ba from the same sum:
// F == F^T bitwise.
//
// ---- bornvi_spd_solve: (A + damping I) x = b by Cholesky, ONE workgroup (a grid-wide barrier is not used anywhere in
// this library: DESIGN.md section 6).  Blocked right-looking factorisation, panel width 16:
//   the lower triangle of A^T's upper triangle is copied into the workspace W (A itself is never written);
//   per panel: its (P - k0) x 16 block goes to LDS (pitch 17 doubles: a thread per row walks its row, consecutive rows
//   are 34 dwords apart -- 32 distinct 8-byte slots per half-wave), is factored there column by column (pivot test,
//   square root, one division per row, rank-1 update of the panel's remaining columns), written back, and the trailing
//   matrix W22 -= L21 L21^T is updated from LDS in 4 x 4 register blocks whose rows and columns are INTERLEAVED (row
//   i_b + ii S, column j_b + jj S, S = ceil(m / 4)): consecutive lanes touch consecutive columns (coalesced, conflict
//   free) and the blocks with jj > ii lie wholly above the diagonal and are skipped at compile time -- half the flops;
//   then L y = b forward and L^T x = y backward, panel by panel: the 16 x 16 diagonal block is solved by 16 lanes of
//   wave 0 with shuffles, the rest is one thread per row (forward) or per-row products reduced over the workgroup by
//   wave butterflies and the wave totals in order (backward).
// Every sum has a fixed order: bitwise reproducible.  LDS at P = 1024: 136 KiB panel + 8 KiB y + 5 KiB = 149 KiB.
// Failure rule: pivot k (from 0) not positive or not finite -> info = k + 1; b not finite -> info = P + 1; a solution
// that is not finite -> info = P + 2; in each case x = b, bit for bit, and nothing else is written to x.
//
// ---- bornvi_score_fisher_gram: F[j] = (1 / B) X_j X_j^T for nblocks consecutive blocks X_j of R
// rows x ld columns of the score rows bornvi_mps_score_rows wrote (the columns B .. ld - 1 are 0.0).  The same split-K
// SYRK with a plain row source (16-byte loads, stores to LDS, nothing computed on the way), the 64 x 64 tile of the Fisher
// kernel (a site block at D = 4 has 32 rows: a 128-row tile would be 15/16 padding), grid (tile pairs, G, nblocks); the
// geometry is syrk::geom(ld, R, 64) with ld a power of two >= 64, so an entry's sum has the same order whatever R is: a
// site's block equals the diagonal block of the whole matrix bit for bit.  score_gram_finish_kernel adds the G partials in
// index order, divides by B once and writes F_ab and F_ba from that value.
//
// ---- bornvi_spd_solve_batched: the body of bornvi_spd_solve (spd_solve_kernel<true>), one workgroup per system: system j
// works on A[j], b[j], x[j], info[j] and its own P x P slice of the workspace, with the same operation order, info codes and
// "x = b where info != 0" rule: bit for bit what bornvi_spd_solve gives on that system.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "reduce_dev.hpp"
#include "syrk_f64.hpp"

namespace bornvi {

namespace {
// ------------------------------------------------------------------------------------------------ Fisher Gram
constexpr int FG_MT = 2, FG_T = 32 * FG_MT;                           // wave tile 2 x 2 MFMA tiles, workgroup tile 64 x 64
using syrk::d2;

// The row source of syrk::split_k: parameter p's row is d_p = 1/2 (row_{2p} - row_{2p+1}); the row side stores e = d r,
// the column side d; both 0 where r is 0 (under the floor).  Owns the slab's table of reciprocals.
struct FisherRows {
  const double* __restrict__ q;
  double* __restrict__ rs;                                            // [syrk::SLAB_MAX]
  long long N;
  double q_floor;
  int t, lrow, lk;
  const double* ag[FG_MT];
  const double* bg[FG_MT];
  bool aok[FG_MT], bok[FG_MT];                                        // parameters past P read as zero
  d2 ap[FG_MT], am[FG_MT], bp[FG_MT], bm[FG_MT];

  __device__ __forceinline__ FisherRows(const double* __restrict__ shifted, const double* __restrict__ q_, double* __restrict__ rs_,
                                        long long N_, int P, int ti, int tj, double q_floor_)
      : q(q_), rs(rs_), N(N_), q_floor(q_floor_), t(threadIdx.x), lrow(threadIdx.x >> 3), lk((threadIdx.x & 7) * 2) {
#pragma unroll
    for (int u = 0; u < FG_MT; ++u) {
      const int pa = ti * FG_T + lrow + 32 * u, pb = tj * FG_T + lrow + 32 * u;
      aok[u] = pa < P;
      bok[u] = pb < P;
      ag[u] = shifted + (long long)(2 * (aok[u] ? pa : 0)) * N + lk;
      bg[u] = shifted + (long long)(2 * (bok[u] ? pb : 0)) * N + lk;
    }
  }
  __device__ __forceinline__ void load1(bool ok, const double* ptr, long long zoff, d2& p, d2& m) const {
    if (ok) {
      p = *reinterpret_cast<const d2*>(ptr + zoff);
      m = *reinterpret_cast<const d2*>(ptr + N + zoff);
    } else {
      p = m = (d2){0.0, 0.0};
    }
  }
  __device__ __forceinline__ void load(long long z0, long long k0, long long slab) {
    const bool zok = k0 + lk < slab;
    const long long zoff = z0 + k0;
#pragma unroll
    for (int u = 0; u < FG_MT; ++u) load1(zok && aok[u], ag[u], zoff, ap[u], am[u]);
#pragma unroll
    for (int u = 0; u < FG_MT; ++u) load1(zok && bok[u], bg[u], zoff, bp[u], bm[u]);
  }
  // r_z of the slab: one IEEE division per entry and slab, not per k-step
  __device__ __forceinline__ void begin_slab(long long z0, long long slab, long long len16) {
    for (long long i = 2 * t; i < len16; i += 2 * syrk::THREADS) {
      d2 qv = (d2){0.0, 0.0};
      if (i < slab) qv = *reinterpret_cast<const d2*>(q + z0 + i);
      d2 r;
      r.x = qv.x >= q_floor ? 1.0 / qv.x : 0.0;                       // (a NaN q fails the comparison: no contribution)
      r.y = qv.y >= q_floor ? 1.0 / qv.y : 0.0;
      *reinterpret_cast<d2*>(rs + i) = r;
    }
    __syncthreads();
  }
  __device__ __forceinline__ void store(double* __restrict__ As, double* __restrict__ Bs, int buf, long long k0) const {
    const d2 r = *reinterpret_cast<const d2*>(rs + k0 + lk);
#pragma unroll
    for (int u = 0; u < FG_MT; ++u) {
      d2 e, d;
      e.x = r.x != 0.0 ? (0.5 * (ap[u].x - am[u].x)) * r.x : 0.0;
      e.y = r.y != 0.0 ? (0.5 * (ap[u].y - am[u].y)) * r.y : 0.0;
      d.x = r.x != 0.0 ? 0.5 * (bp[u].x - bm[u].x) : 0.0;
      d.y = r.y != 0.0 ? 0.5 * (bp[u].y - bm[u].y) : 0.0;
      *reinterpret_cast<d2*>(As + ((buf * FG_T + lrow + 32 * u) * syrk::PITCH + lk)) = e;
      *reinterpret_cast<d2*>(Bs + ((buf * FG_T + lrow + 32 * u) * syrk::PITCH + lk)) = d;
    }
  }
};

// grid (tiles, G).  part[(g * tiles + tile) * 4096 + row * 64 + col]; the running total over the slabs stays in registers.
__global__ __launch_bounds__(syrk::THREADS) void fisher_gram_kernel(const double* __restrict__ shifted, const double* __restrict__ q,
                                                                    long long N, int P, int T, long long slab, long long per_wg,
                                                                    double q_floor, double* __restrict__ part) {
  extern __shared__ double fg_lds[];                                   // [SLAB_MAX] r, then As, Bs: [2][FG_T][PITCH] each
  double* __restrict__ As = fg_lds + syrk::SLAB_MAX;
  int ti, tj;
  syrk::tile_pair(blockIdx.x, T, ti, tj);
  FisherRows rows(shifted, q, fg_lds, N, P, ti, tj, q_floor);
  syrk::split_k<FG_MT>(rows, As, As + 2 * FG_T * syrk::PITCH, slab, per_wg, part);
}

// grid (tiles): F_ab = F_ba = the G partials of entry (a <= b) added in index order.
__global__ __launch_bounds__(syrk::THREADS) void fisher_finish_kernel(const double* __restrict__ part, int P, int T, int G,
                                                                      double* __restrict__ F) {
  int ti, tj;
  syrk::tile_pair(blockIdx.x, T, ti, tj);
  const long long stride = (long long)gridDim.x * (FG_T * FG_T);
  const double* __restrict__ pt = part + (long long)blockIdx.x * (FG_T * FG_T);
  for (int e = threadIdx.x; e < FG_T * FG_T; e += syrk::THREADS) {
    const int a = ti * FG_T + e / FG_T, b = tj * FG_T + e % FG_T;
    if (a >= P || b >= P || a > b) continue;
    const double sum = syrk::sum_partials(pt + e, G, stride);
    F[(long long)a * P + b] = sum;
    F[(long long)b * P + a] = sum;
  }
}

// ------------------------------------------------------------------------------------------------ score-rows Gram
// The plain row source of syrk::split_k: row p of the block is X[p][0 .. ld), both sides get it as it is; rows past R
// read as zero.
struct PlainRows {
  int lrow, lk;
  const double* ag[FG_MT];
  const double* bg[FG_MT];
  bool aok[FG_MT], bok[FG_MT];
  d2 av[FG_MT], bv[FG_MT];

  __device__ __forceinline__ PlainRows(const double* __restrict__ X, long long ld, int R, int ti, int tj)
      : lrow(threadIdx.x >> 3), lk((threadIdx.x & 7) * 2) {
#pragma unroll
    for (int u = 0; u < FG_MT; ++u) {
      const int pa = ti * FG_T + lrow + 32 * u, pb = tj * FG_T + lrow + 32 * u;
      aok[u] = pa < R;
      bok[u] = pb < R;
      ag[u] = X + (long long)(aok[u] ? pa : 0) * ld + lk;
      bg[u] = X + (long long)(bok[u] ? pb : 0) * ld + lk;
    }
  }
  __device__ __forceinline__ void load(long long z0, long long k0, long long slab) {
    const bool zok = k0 + lk < slab;
    const long long zoff = z0 + k0;
#pragma unroll
    for (int u = 0; u < FG_MT; ++u) {
      av[u] = zok && aok[u] ? *reinterpret_cast<const d2*>(ag[u] + zoff) : (d2){0.0, 0.0};
      bv[u] = zok && bok[u] ? *reinterpret_cast<const d2*>(bg[u] + zoff) : (d2){0.0, 0.0};
    }
  }
  __device__ __forceinline__ void begin_slab(long long, long long, long long) {}
  __device__ __forceinline__ void store(double* __restrict__ As, double* __restrict__ Bs, int buf, long long) const {
#pragma unroll
    for (int u = 0; u < FG_MT; ++u) {
      *reinterpret_cast<d2*>(As + ((buf * FG_T + lrow + 32 * u) * syrk::PITCH + lk)) = av[u];
      *reinterpret_cast<d2*>(Bs + ((buf * FG_T + lrow + 32 * u) * syrk::PITCH + lk)) = bv[u];
    }
  }
};

// grid (tiles, G, nblocks).  Block j: rows X + j R ld, partials part + j G tiles 4096.
__global__ __launch_bounds__(syrk::THREADS) void score_gram_kernel(const double* __restrict__ X, long long ld, int R, int T,
                                                                   long long slab, long long per_wg, double* __restrict__ part) {
  __shared__ double sg_lds[4 * FG_T * syrk::PITCH];                    // As, Bs: [2][FG_T][PITCH] each (36 KiB)
  int ti, tj;
  syrk::tile_pair(blockIdx.x, T, ti, tj);
  PlainRows rows(X + (long long)blockIdx.z * R * ld, ld, R, ti, tj);
  syrk::split_k<FG_MT>(rows, sg_lds, sg_lds + 2 * FG_T * syrk::PITCH, slab, per_wg,
                       part + (long long)blockIdx.z * gridDim.y * gridDim.x * (FG_T * FG_T));
}

// grid (tiles, nblocks): F[j]_ab = F[j]_ba = (the G partials of entry (a <= b) added in index order) / B.
__global__ __launch_bounds__(syrk::THREADS) void score_gram_finish_kernel(const double* __restrict__ part, int R, int T, int G, double Bd,
                                                                     double* __restrict__ F) {
  int ti, tj;
  syrk::tile_pair(blockIdx.x, T, ti, tj);
  const long long stride = (long long)gridDim.x * (FG_T * FG_T);
  const double* __restrict__ pt = part + ((long long)blockIdx.y * G * gridDim.x + blockIdx.x) * (FG_T * FG_T);
  double* __restrict__ Fj = F + (long long)blockIdx.y * R * R;
  for (int e = threadIdx.x; e < FG_T * FG_T; e += syrk::THREADS) {
    const int a = ti * FG_T + e / FG_T, b = tj * FG_T + e % FG_T;
    if (a >= R || b >= R || a > b) continue;
    const double v = syrk::sum_partials(pt + e, G, stride) / Bd;
    Fj[(long long)a * R + b] = v;
    Fj[(long long)b * R + a] = v;
  }
}

// ------------------------------------------------------------------------------------------------ SPD solve
constexpr int SS_NB = 16, SS_PITCH = 17, SS_MAX_P = 1024;

struct SsLds {
  double* pan;    // [P][SS_PITCH]
  double* ys;     // [P]
  double* diag;   // [SS_NB][SS_PITCH]
  double* red;    // [16 waves][SS_NB]
  double* sums;   // [SS_NB]
};

// L y = v (forward) or L^T x = v (backward) for one diagonal block in LDS, by the first nb lanes of wave 0.
__device__ __forceinline__ void ss_diag_solve(const double* __restrict__ diag, double* __restrict__ ys, int k0, int nb,
                                              const double* __restrict__ sums, bool backward) {
  const int lane = threadIdx.x;
  if (lane >= 64) return;
  const int r = lane < nb ? lane : 0;
  double v = lane < nb ? ys[k0 + r] - (sums ? sums[r] : 0.0) : 0.0;
  if (!backward) {
    for (int c = 0; c < nb; ++c) {
      const double piv = __shfl(v, c) / diag[c * SS_PITCH + c];
      if (lane == c) v = piv;
      else if (lane > c && lane < nb) v -= diag[r * SS_PITCH + c] * piv;
    }
  } else {
    for (int c = nb - 1; c >= 0; --c) {
      const double piv = __shfl(v, c) / diag[c * SS_PITCH + c];
      if (lane == c) v = piv;
      else if (lane < c) v -= diag[c * SS_PITCH + r] * piv;
    }
  }
  if (lane < nb) ys[k0 + r] = v;
}

// BATCHED = false: bornvi_spd_solve, grid 1.  BATCHED = true: bornvi_spd_solve_batched, grid nb: workgroup j moves to
// system j's A, b, x, info and P x P slice of the workspace and then runs the same body.
template <bool BATCHED>
__global__ __launch_bounds__(1024) void spd_solve_kernel(const double* __restrict__ A, int P, double damping,
                                                         const double* __restrict__ b, double* __restrict__ x,
                                                         int* __restrict__ info, double* __restrict__ W) {
  extern __shared__ double ss_lds[];
  __shared__ int ss_flag;
  if (BATCHED) {
    const long long j = blockIdx.x;
    A += j * P * P;
    b += j * P;
    x += j * P;
    info += j;
    W += j * P * P;
  }
  SsLds L;
  L.pan = ss_lds;
  L.ys = L.pan + (size_t)P * SS_PITCH;
  L.diag = L.ys + P;
  L.red = L.diag + SS_NB * SS_PITCH;
  L.sums = L.red + 16 * SS_NB;
  const int t = threadIdx.x, nt = blockDim.x;
  int fail = 0;
  // b: finite?  (a uniform decision: every thread reads the flag after the barrier)
  if (t == 0) ss_flag = 0;
  __syncthreads();
  for (int i = t; i < P; i += nt) {
    const double v = b[i];
    L.ys[i] = v;
    if (!(fabs(v) <= 1.79769313486231570815e308)) ss_flag = 1;
  }
  // W (lower, row-major) <- the upper triangle of A, damping on the diagonal
  for (long long idx = t; idx < (long long)P * P; idx += nt) {
    const int i = (int)(idx / P), j = (int)(idx % P);
    if (j <= i) W[idx] = A[(long long)j * P + i] + (i == j ? damping : 0.0);
  }
  __syncthreads();
  if (ss_flag) fail = P + 1;
  if (!fail) {
    for (int k0 = 0; k0 < P; k0 += SS_NB) {
      const int nb = P - k0 < SS_NB ? P - k0 : SS_NB, m = P - k0;
      for (int idx = t; idx < m * SS_NB; idx += nt) {
        const int r = idx / SS_NB, c = idx % SS_NB;
        if (c < nb && c <= r) L.pan[r * SS_PITCH + c] = W[(long long)(k0 + r) * P + k0 + c];
      }
      __syncthreads();
      for (int c = 0; c < nb; ++c) {
        const double piv = L.pan[c * SS_PITCH + c];
        if (!(piv > 0.0) || !(piv <= 1.79769313486231570815e308)) { fail = k0 + c + 1; break; }
        const double s = sqrt(piv);
        __syncthreads();                                   // (everybody has read the pivot)
        for (int r = t; r < m; r += nt) {
          if (r > c) L.pan[r * SS_PITCH + c] = L.pan[r * SS_PITCH + c] / s;
          else if (r == c) L.pan[c * SS_PITCH + c] = s;
        }
        __syncthreads();
        for (int r = t; r < m; r += nt) {
          if (r > c) {
            const double lrc = L.pan[r * SS_PITCH + c];
            const int jend = r < nb - 1 ? r : nb - 1;
            for (int j = c + 1; j <= jend; ++j) L.pan[r * SS_PITCH + j] -= lrc * L.pan[j * SS_PITCH + c];
          }
        }
        __syncthreads();
      }
      if (fail) break;
      for (int idx = t; idx < m * SS_NB; idx += nt) {
        const int r = idx / SS_NB, c = idx % SS_NB;
        if (c < nb && c <= r) W[(long long)(k0 + r) * P + k0 + c] = L.pan[r * SS_PITCH + c];
      }
      // trailing update W22 -= L21 L21^T (lower triangle), interleaved 4 x 4 register blocks
      const int mt = m - nb;
      if (mt > 0) {
        const int S = (mt + 3) / 4;
        const double* __restrict__ p21 = L.pan + nb * SS_PITCH;
        double* __restrict__ W22 = W + (long long)(k0 + nb) * P + k0 + nb;
        for (int idx = t; idx < S * S; idx += nt) {
          const int ib = idx / S, jb = idx % S;
          const bool dg = jb <= ib;
          int ri[4], rj[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            ri[u] = ib + u * S < mt ? ib + u * S : mt - 1;           // (clamped rows are computed and not stored)
            rj[u] = jb + u * S < mt ? jb + u * S : mt - 1;
          }
          double acc[4][4];
#pragma unroll
          for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = 0.0;
          for (int c = 0; c < nb; ++c) {
            double a[4], bb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = p21[ri[u] * SS_PITCH + c]; bb[u] = p21[rj[u] * SS_PITCH + c]; }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
              for (int jj = 0; jj < 4; ++jj)
                if (jj < ii || (jj == ii && dg)) acc[ii][jj] += a[ii] * bb[jj];
          }
#pragma unroll
          for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
              if ((jj < ii || (jj == ii && dg)) && ib + ii * S < mt && jb + jj * S < mt)
                W22[(long long)(ib + ii * S) * P + jb + jj * S] -= acc[ii][jj];
        }
      }
      __syncthreads();
    }
  }
  if (!fail) {
    // forward: L y = b
    for (int k0 = 0; k0 < P; k0 += SS_NB) {
      const int nb = P - k0 < SS_NB ? P - k0 : SS_NB;
      for (int idx = t; idx < SS_NB * SS_NB; idx += nt) {
        const int r = idx / SS_NB, c = idx % SS_NB;
        if (r < nb && c <= r) L.diag[r * SS_PITCH + c] = W[(long long)(k0 + r) * P + k0 + c];
      }
      __syncthreads();
      ss_diag_solve(L.diag, L.ys, k0, nb, nullptr, false);
      __syncthreads();
      for (int i = k0 + nb + t; i < P; i += nt) {
        const double* __restrict__ row = W + (long long)i * P + k0;
        double v = L.ys[i];
        for (int c = 0; c < nb; ++c) v -= row[c] * L.ys[k0 + c];
        L.ys[i] = v;
      }
      __syncthreads();
    }
    // backward: L^T x = y
    const int last = (P - 1) / SS_NB * SS_NB;
    for (int k0 = last; k0 >= 0; k0 -= SS_NB) {
      const int nb = P - k0 < SS_NB ? P - k0 : SS_NB;
      double pr[SS_NB];
#pragma unroll
      for (int c = 0; c < SS_NB; ++c) pr[c] = 0.0;
      for (int i = k0 + nb + t; i < P; i += nt) {          // (nb == 16 whenever a row lies below the block)
        const double* __restrict__ row = W + (long long)i * P + k0;
        const double xi = L.ys[i];
#pragma unroll
        for (int c = 0; c < SS_NB; ++c) pr[c] += row[c] * xi;
      }
#pragma unroll
      for (int c = 0; c < SS_NB; ++c) {
        const double w = wave_sum(pr[c]);
        if ((t & 63) == 0) L.red[(t >> 6) * SS_NB + c] = w;
      }
      for (int idx = t; idx < SS_NB * SS_NB; idx += nt) {
        const int r = idx / SS_NB, c = idx % SS_NB;
        if (r < nb && c <= r) L.diag[r * SS_PITCH + c] = W[(long long)(k0 + r) * P + k0 + c];
      }
      __syncthreads();
      if (t < SS_NB) {
        double s = 0.0;
        for (int w = 0; w < nt / 64; ++w) s += L.red[w * SS_NB + t];
        L.sums[t] = s;
      }
      __syncthreads();
      ss_diag_solve(L.diag, L.ys, k0, nb, L.sums, true);
      __syncthreads();
    }
    if (t == 0) ss_flag = 0;
    __syncthreads();
    for (int i = t; i < P; i += nt)
      if (!(fabs(L.ys[i]) <= 1.79769313486231570815e308)) ss_flag = 1;
    __syncthreads();
    if (ss_flag) fail = P + 2;
  }
  for (int i = t; i < P; i += nt) x[i] = fail ? b[i] : L.ys[i];
  if (t == 0) *info = fail;
}

LdsRaised fg_lds_raised, ss_lds_raised, ssb_lds_raised;
}  // namespace

size_t fisher_workspace_bytes(int n, int n_shift) { return syrk::workspace_bytes(syrk::geom(1ll << n, n_shift, FG_T), FG_T); }

hipError_t launch_fisher_gram(int n, const double* shifted, int n_shift, const double* q, double q_floor, double* F, void* ws,
                              hipStream_t st) {
  const syrk::Geom g = syrk::geom(1ll << n, n_shift, FG_T);
  const size_t lds = syrk::SLAB_MAX * sizeof(double) + syrk::tiles_lds_bytes(FG_T);
  hipError_t e = raise_lds_once(reinterpret_cast<const void*>(fisher_gram_kernel), lds, fg_lds_raised);
  if (e != hipSuccess) return e;
  double* part = (double*)ws_align(ws);
  fisher_gram_kernel<<<dim3((unsigned)g.tiles, (unsigned)g.G), syrk::THREADS, lds, st>>>(shifted, q, 1ll << n, n_shift, g.T, g.slab,
                                                                                         g.per_wg, q_floor, part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  fisher_finish_kernel<<<dim3((unsigned)g.tiles), syrk::THREADS, 0, st>>>(part, n_shift, g.T, g.G, F);
  return hipGetLastError();
}

size_t score_fisher_workspace_bytes(int R, int nblocks, long long ld) {
  const syrk::Geom g = syrk::geom(ld, R, FG_T);
  return (size_t)nblocks * g.G * g.tiles * FG_T * FG_T * sizeof(double) + 512;
}

hipError_t launch_score_fisher_gram(int R, int nblocks, long long B, long long ld, const double* rows, double* F, void* ws,
                                    hipStream_t st) {
  const syrk::Geom g = syrk::geom(ld, R, FG_T);
  double* part = (double*)ws_align(ws);
  score_gram_kernel<<<dim3((unsigned)g.tiles, (unsigned)g.G, (unsigned)nblocks), syrk::THREADS, 0, st>>>(rows, ld, R, g.T, g.slab,
                                                                                                         g.per_wg, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  score_gram_finish_kernel<<<dim3((unsigned)g.tiles, (unsigned)nblocks), syrk::THREADS, 0, st>>>(part, R, g.T, g.G, (double)B, F);
  return hipGetLastError();
}

size_t spd_solve_workspace_bytes(int P) { return (size_t)P * P * sizeof(double) + 512; }

hipError_t launch_spd_solve(int P, const double* A, double damping, const double* b, double* x, int* info, void* ws, hipStream_t st) {
  const size_t fixed = SS_NB * SS_PITCH + 16 * SS_NB + SS_NB;
  const size_t lds = ((size_t)P * SS_PITCH + P + fixed) * sizeof(double);
  hipError_t e = raise_lds_once(reinterpret_cast<const void*>(spd_solve_kernel<false>),
                                ((size_t)SS_MAX_P * SS_PITCH + SS_MAX_P + fixed) * sizeof(double), ss_lds_raised);
  if (e != hipSuccess) return e;
  const int threads = P <= 64 ? 64 : (P <= 256 ? 256 : 1024);
  spd_solve_kernel<false><<<1, threads, lds, st>>>(A, P, damping, b, x, info, (double*)ws_align(ws));
  return hipGetLastError();
}

size_t spd_solve_batched_workspace_bytes(int P, int nb) { return (size_t)nb * P * P * sizeof(double) + 512; }

hipError_t launch_spd_solve_batched(int P, int nb, const double* A, double damping, const double* b, double* x, int* info, void* ws,
                                    hipStream_t st) {
  const size_t fixed = SS_NB * SS_PITCH + 16 * SS_NB + SS_NB;
  const size_t lds = ((size_t)P * SS_PITCH + P + fixed) * sizeof(double);
  hipError_t e = raise_lds_once(reinterpret_cast<const void*>(spd_solve_kernel<true>),
                                ((size_t)SS_MAX_P * SS_PITCH + SS_MAX_P + fixed) * sizeof(double), ssb_lds_raised);
  if (e != hipSuccess) return e;
  const int threads = P <= 64 ? 64 : (P <= 256 ? 256 : 1024);
  spd_solve_kernel<true><<<(unsigned)nb, threads, lds, st>>>(A, P, damping, b, x, info, (double*)ws_align(ws));
  return hipGetLastError();
}

}  // namespace bornvi
