// Natural-gradient pieces (gfx950): the classical Fisher matrix of a Born distribution from the stored parameter-shift
// rows (bornvi_fisher_gram) and the damped Cholesky solve of the natural-gradient step (bornvi_spd_solve).
//
// ---- bornvi_fisher_gram: F_ab = sum_z d_a(z) d_b(z) r_z,  d_a = 1/2 (row_{2a} - row_{2a+1}),  r_z = 1/q_z where
// q_z >= q_floor, else 0 (a state under the floor contributes nothing: both factors of its products are stored as 0).
// A split-K SYRK on v_mfma_f64_16x16x4_f64, grid (upper-triangle tile pairs) x (G groups of z-slabs):
//   output tile 64 x 64 per workgroup of 4 waves (2 x 2; a wave owns 32 x 32 = 2 x 2 MFMA tiles, 32 accumulator VGPRs
//   plus 32 for the running total over the workgroup's slabs);
//   a slab is at most 4096 entries of z (geometry: fg_geom); its reciprocals r_z go to LDS once (one IEEE division per
//   entry and slab, not per k-step); k-step 16, LDS double-buffered, one barrier per k-step, the next k-step's rows in
//   flight in registers during the MFMAs (16-byte loads: 8 of rows and none of q per thread and k-step);
//   on the way into LDS the thread forms d (one subtraction, the halving is exact) and stores e = d r on the row side
//   (As) and d on the column side (Bs): ONE side is scaled, so a product e_a d_b carries the roundings of d_a, d_b, r,
//   e and the product itself (C_TERM = 5 half-units; tests/test_gpu_fisher_kernel.py);
//   LDS rows padded to 18 doubles (pitch 144 bytes, 16-byte aligned for the b128 stores): the 16 rows x 2 k a half-wave
//   reads with ds_read_b64 sit at dwords 36 r + 2 k mod 64 -- 32 distinct 8-byte slots, no bank conflict;
//   LDS: 32 KiB of r + 36 KiB of tiles = 68 KiB (two workgroups per CU); no scratch (build.py holds the budget).
// Each slab starts from a zero accumulator (a chain of at most 4096 additions inside the MFMAs), the workgroup adds its
// slabs' results one after the other, and fisher_finish_kernel adds the G <= 256 (64 up to n = 28) partial tiles of an entry in index order:
// no atomics, bitwise reproducible.  Only tiles with tile_i <= tile_j are computed and, inside a diagonal tile, only the
// entries a <= b are used; the finishing launch writes F_ab and F_ba from the same sum: F == F^T bitwise.
// Fragment layout of the f64 MFMA as in kernels_batched.hip: A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15], D[row = (lane >> 4) + 4 r][col = lane & 15].
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
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>

#include "kernels.hpp"

namespace bornvi {

namespace {
// ------------------------------------------------------------------------------------------------ Fisher Gram
constexpr int FG_T = 64, FG_BK = 16, FG_PITCH = 18, FG_THREADS = 256;
constexpr int FG_SLAB_MAX = 4096, FG_GROUPS = 64;
typedef double fg_d4 __attribute__((ext_vector_type(4)));
typedef double fg_d2 __attribute__((ext_vector_type(2)));

struct FgGeom {
  long long slab;      // entries of z per slab (<= 4096)
  long long per_wg;    // slabs a workgroup adds up one after the other
  int G;               // workgroups along z = partial tiles per entry
  int T;               // 64-row tiles per side
  int tiles;           // T (T + 1) / 2
};

FgGeom fg_geom(int n, int n_shift) {
  const long long N = 1ll << n;
  FgGeom g;
  g.slab = N <= 256 ? N : (N / 64 < 256 ? 256 : (N / 64 > FG_SLAB_MAX ? FG_SLAB_MAX : N / 64));
  const long long nslab = N / g.slab;
  const long long gmax = nslab / 1024 > FG_GROUPS ? nslab / 1024 : FG_GROUPS;     // (per_wg <= 1024: n >= 29 takes more groups)
  g.G = (int)(nslab < gmax ? nslab : gmax);
  g.per_wg = nslab / g.G;
  g.T = (n_shift + FG_T - 1) / FG_T;
  g.tiles = g.T * (g.T + 1) / 2;
  return g;
}

// grid (tiles, G).  part[(g * tiles + tile) * 4096 + row * 64 + col]
__global__ __launch_bounds__(FG_THREADS) void fisher_gram_kernel(const double* __restrict__ shifted, const double* __restrict__ q,
                                                                 long long N, int P, int T, long long slab, long long per_wg,
                                                                 double q_floor, double* __restrict__ part) {
  extern __shared__ double fg_lds[];
  double* __restrict__ rs = fg_lds;                                    // [FG_SLAB_MAX]
  double* __restrict__ As = fg_lds + FG_SLAB_MAX;                      // [2][FG_T][FG_PITCH]: e = d r
  double* __restrict__ Bs = As + 2 * FG_T * FG_PITCH;                  // [2][FG_T][FG_PITCH]: d
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wi = wave & 1, wj = wave >> 1;
  int ti = 0, rem = blockIdx.x;                                       // tile pair (ti <= tj) number blockIdx.x, row by row
  while (rem >= T - ti) { rem -= T - ti; ++ti; }
  const int tj = ti + rem;
  const int lrow = t >> 3, lk = (t & 7) * 2;
  const int pa0 = ti * FG_T + lrow, pa1 = pa0 + 32, pb0 = tj * FG_T + lrow, pb1 = pb0 + 32;
  const bool aok0 = pa0 < P, aok1 = pa1 < P, bok0 = pb0 < P, bok1 = pb1 < P;      // parameters past P read as zero
  const double* __restrict__ Ag0 = shifted + (long long)(2 * (aok0 ? pa0 : 0)) * N + lk;
  const double* __restrict__ Ag1 = shifted + (long long)(2 * (aok1 ? pa1 : 0)) * N + lk;
  const double* __restrict__ Bg0 = shifted + (long long)(2 * (bok0 ? pb0 : 0)) * N + lk;
  const double* __restrict__ Bg1 = shifted + (long long)(2 * (bok1 ? pb1 : 0)) * N + lk;
  const long long len16 = (slab + FG_BK - 1) / FG_BK * FG_BK;         // (a slab shorter than a k-step: n <= 3)
  const long long nk = len16 / FG_BK;
  const fg_d2 zero2 = (fg_d2){0.0, 0.0};
  fg_d2 ap0, am0, ap1, am1, bp0, bm0, bp1, bm1;
#define FG_LOAD(ok, ptr, p, m)                                                   \
  if (zok && (ok)) {                                                             \
    p = *reinterpret_cast<const fg_d2*>((ptr) + zoff);                           \
    m = *reinterpret_cast<const fg_d2*>((ptr) + N + zoff);                       \
  } else {                                                                       \
    p = m = zero2;                                                               \
  }
#define FG_LOAD_TILES(z0, k0)                                                    \
  {                                                                              \
    const bool zok = (k0) + lk < slab;                                           \
    const long long zoff = (z0) + (k0);                                          \
    FG_LOAD(aok0, Ag0, ap0, am0) FG_LOAD(aok1, Ag1, ap1, am1)                    \
    FG_LOAD(bok0, Bg0, bp0, bm0) FG_LOAD(bok1, Bg1, bp1, bm1)                    \
  }
  // d = 1/2 (plus - minus); the row side stores e = d r, the column side d; both 0 where r is 0 (under the floor)
#define FG_STORE(u, ap, am, bp, bm)                                              \
  {                                                                              \
    fg_d2 e, d;                                                                  \
    e.x = r.x != 0.0 ? (0.5 * (ap.x - am.x)) * r.x : 0.0;                        \
    e.y = r.y != 0.0 ? (0.5 * (ap.y - am.y)) * r.y : 0.0;                        \
    d.x = r.x != 0.0 ? 0.5 * (bp.x - bm.x) : 0.0;                                \
    d.y = r.y != 0.0 ? 0.5 * (bp.y - bm.y) : 0.0;                                \
    *reinterpret_cast<fg_d2*>(As + ((buf_ * FG_T + lrow + 32 * (u)) * FG_PITCH + lk)) = e;  \
    *reinterpret_cast<fg_d2*>(Bs + ((buf_ * FG_T + lrow + 32 * (u)) * FG_PITCH + lk)) = d;  \
  }
#define FG_STORE_TILES(buf, k0)                                                  \
  {                                                                              \
    const int buf_ = (buf);                                                      \
    const fg_d2 r = *reinterpret_cast<const fg_d2*>(rs + (k0) + lk);             \
    FG_STORE(0, ap0, am0, bp0, bm0) FG_STORE(1, ap1, am1, bp1, bm1)              \
  }
  fg_d4 total[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) total[mi][ni] = (fg_d4){0.0, 0.0, 0.0, 0.0};
  const int fr = lane & 15, fk = lane >> 4;
#pragma unroll 1
  for (long long s = 0; s < per_wg; ++s) {
    const long long z0 = ((long long)blockIdx.y * per_wg + s) * slab;
    FG_LOAD_TILES(z0, 0)
    // (the previous slab's last k-step ended with a barrier: nobody reads rs or the tiles any more)
    for (long long i = 2 * t; i < len16; i += 2 * FG_THREADS) {
      fg_d2 qv = (fg_d2){0.0, 0.0};
      if (i < slab) qv = *reinterpret_cast<const fg_d2*>(q + z0 + i);
      fg_d2 r;
      r.x = qv.x >= q_floor ? 1.0 / qv.x : 0.0;                       // (a NaN q fails the comparison: no contribution)
      r.y = qv.y >= q_floor ? 1.0 / qv.y : 0.0;
      *reinterpret_cast<fg_d2*>(rs + i) = r;
    }
    __syncthreads();
    FG_STORE_TILES(0, 0)
    __syncthreads();
    fg_d4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = (fg_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (long long kt = 0; kt < nk; ++kt) {
      const int cur = (int)(kt & 1);
      if (kt + 1 < nk) FG_LOAD_TILES(z0, (kt + 1) * FG_BK)           // in flight during this k-step's MFMAs
      const double* __restrict__ Ac = As + (cur * FG_T + wi * 32 + fr) * FG_PITCH + fk;
      const double* __restrict__ Bc = Bs + (cur * FG_T + wj * 32 + fr) * FG_PITCH + fk;
#pragma unroll
      for (int ks = 0; ks < FG_BK / 4; ++ks) {
        double a[2], b[2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) a[mi] = Ac[mi * 16 * FG_PITCH + ks * 4];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) b[ni] = Bc[ni * 16 * FG_PITCH + ks * 4];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
      }
      if (kt + 1 < nk) FG_STORE_TILES(cur ^ 1, (kt + 1) * FG_BK)
      __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) total[mi][ni] += acc[mi][ni];
  }
  // D[row = fk + 4 r][col = fr] of MFMA tile (mi, ni): tile entry (wi * 32 + mi * 16 + fk + 4 r, wj * 32 + ni * 16 + fr)
  double* __restrict__ pt = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (FG_T * FG_T);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) pt[(wi * 32 + mi * 16 + fk + 4 * r) * FG_T + wj * 32 + ni * 16 + fr] = total[mi][ni][r];
}

#undef FG_LOAD
#undef FG_LOAD_TILES
#undef FG_STORE
#undef FG_STORE_TILES

// grid (tiles): F_ab = F_ba = the G partials of entry (a <= b) added in index order.
__global__ __launch_bounds__(FG_THREADS) void fisher_finish_kernel(const double* __restrict__ part, int P, int T, int G,
                                                                   double* __restrict__ F) {
  int ti = 0, rem = blockIdx.x;
  while (rem >= T - ti) { rem -= T - ti; ++ti; }
  const int tj = ti + rem;
  const long long stride = (long long)gridDim.x * (FG_T * FG_T);
  const double* __restrict__ pt = part + (long long)blockIdx.x * (FG_T * FG_T);
  for (int e = threadIdx.x; e < FG_T * FG_T; e += FG_THREADS) {
    const int a = ti * FG_T + e / FG_T, b = tj * FG_T + e % FG_T;
    if (a >= P || b >= P || a > b) continue;
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += pt[g * stride + e];
    F[(long long)a * P + b] = sum;
    F[(long long)b * P + a] = sum;
  }
}

// ------------------------------------------------------------------------------------------------ SPD solve
constexpr int SS_NB = 16, SS_PITCH = 17, SS_MAX_P = 1024;

__device__ __forceinline__ double ss_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

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

__global__ __launch_bounds__(1024) void spd_solve_kernel(const double* __restrict__ A, int P, double damping,
                                                         const double* __restrict__ b, double* __restrict__ x,
                                                         int* __restrict__ info, double* __restrict__ W) {
  extern __shared__ double ss_lds[];
  __shared__ int ss_flag;
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
        const double w = ss_wave_sum(pr[c]);
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

// More than 64 KiB of dynamic LDS needs the kernel's attribute raised, once per device (idempotent, so a race between two
// threads' first calls is harmless).  Later calls -- the ones a stream capture may record -- touch no function attribute.
constexpr int FS_MAX_DEVICES = 64;
hipError_t fs_allow_lds(const void* fn, size_t bytes, std::atomic<unsigned char>* done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool known = dev >= 0 && dev < FS_MAX_DEVICES;
  if (known && done[dev].load(std::memory_order_acquire)) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess && known) done[dev].store(1, std::memory_order_release);
  return e;
}
std::atomic<unsigned char> fg_lds_done[FS_MAX_DEVICES], ss_lds_done[FS_MAX_DEVICES];

char* fs_align(void* p) { return (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }
}  // namespace

size_t fisher_workspace_bytes(int n, int n_shift) {
  const FgGeom g = fg_geom(n, n_shift);
  return (size_t)g.G * g.tiles * FG_T * FG_T * sizeof(double) + 512;
}

hipError_t launch_fisher_gram(int n, const double* shifted, int n_shift, const double* q, double q_floor, double* F, void* ws,
                              hipStream_t st) {
  const FgGeom g = fg_geom(n, n_shift);
  const size_t lds = (size_t)(FG_SLAB_MAX + 4 * FG_T * FG_PITCH) * sizeof(double);
  hipError_t e = fs_allow_lds(reinterpret_cast<const void*>(fisher_gram_kernel), lds, fg_lds_done);
  if (e != hipSuccess) return e;
  double* part = (double*)fs_align(ws);
  fisher_gram_kernel<<<dim3((unsigned)g.tiles, (unsigned)g.G), FG_THREADS, lds, st>>>(shifted, q, 1ll << n, n_shift, g.T, g.slab,
                                                                                      g.per_wg, q_floor, part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  fisher_finish_kernel<<<dim3((unsigned)g.tiles), FG_THREADS, 0, st>>>(part, n_shift, g.T, g.G, F);
  return hipGetLastError();
}

size_t spd_solve_workspace_bytes(int P) { return (size_t)P * P * sizeof(double) + 512; }

hipError_t launch_spd_solve(int P, const double* A, double damping, const double* b, double* x, int* info, void* ws, hipStream_t st) {
  const size_t fixed = SS_NB * SS_PITCH + 16 * SS_NB + SS_NB;
  const size_t lds = ((size_t)P * SS_PITCH + P + fixed) * sizeof(double);
  hipError_t e = fs_allow_lds(reinterpret_cast<const void*>(spd_solve_kernel),
                              ((size_t)SS_MAX_P * SS_PITCH + SS_MAX_P + fixed) * sizeof(double), ss_lds_done);
  if (e != hipSuccess) return e;
  const int threads = P <= 64 ? 64 : (P <= 256 ? 256 : 1024);
  spd_solve_kernel<<<1, threads, lds, st>>>(A, P, damping, b, x, info, (double*)fs_align(ws));
  return hipGetLastError();
}

}  // namespace bornvi
