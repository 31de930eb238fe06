// Squared maximum mean discrepancy with a kernel of the Hamming distance (bornvi_mmd.h).
//
// 1. bornvi_mmd_weights (enumerated families).  A kernel kappa[d_H(z, z')] is diagonalised by the Walsh-Hadamard transform:
//    K = 2^-n H diag(lam[popcount k]) H.  With d = q - target:  loss = d^T K d = 2^-n sum_k lam[pop k] dhat_k^2, dhat = H d, and
//    w = 2 K d.  Two transforms of 2^n doubles, no 4^n object.
//    A pass holds a tile of 2^MMD_TILE_BITS doubles in LDS and transforms some of the index bits: the low pass the bits
//    [0, MMD_TILE_BITS) of a contiguous tile; a high pass up to MMD_HIGH_BITS bits [lo, lo + hb) of a tile of 2^hb rows, each row
//    2^(MMD_TILE_BITS - hb) >= 8 contiguous doubles (64 bytes), the rows 2^lo doubles apart.  The butterflies run radix-16 in
//    registers between LDS round trips (four bits a round); the LDS index is padded by one double in 16 (i + (i >> 4)) so that the
//    three access patterns of a round (stride 16, stride 1, stride 256 between lanes) all spread over the banks.
//    The first pass forms d on load.  The pass that completes the forward transform multiplies by lam[pop k] (one rounding),
//    adds its workgroup's partial of sum lam dhat^2 in the fixed order of reduce_dev.hpp, applies 2^(1-n) exactly and goes
//    straight on with the inverse butterflies of its own bits: the spectrum never reaches HBM unscaled.  The remaining passes
//    run the other bit groups again (H is its own inverse up to the power of two).  2 P - 1 launches for P bit groups, and a
//    one-workgroup launch that adds the partials when there is more than one.  Every pass after the first works in place.
//
// 2. bornvi_hamming_pairs_rowsum (sampled families, n <= 63).  cnt_a[d] = #{j : popcount(za_a xor zb_j) = d}: one row per lane,
//    the columns streamed through LDS in tiles of 512 words, a histogram column per lane in LDS laid out bin-major
//    ([d][lane]: the lanes of a wave hit distinct banks), integer LDS adds.  The columns are split into G ranges over
//    blockIdx.y; the ranges' integer counts are added by the finishing launch (integer addition: no order), which forms
//    r_a = sum_d kappa[d] * cnt_a[d] in ascending d with separately rounded multiply and add.  total = sum_a r_a in the fixed
//    order: per workgroup of 256 rows, then over the workgroups.  No floating-point atomics anywhere.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bornvi_mmd.h"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace bornvi {

namespace {
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MW_T = BORNVI_MMD_TILE_BITS;        // 2^12 doubles = 32 KiB (34 KiB padded): four workgroups per CU
constexpr int MW_H = BORNVI_MMD_HIGH_BITS;        // rows of a high pass keep 2^(12 - 9) = 8 doubles = 64 contiguous bytes
constexpr int MW_THREADS = 256;
constexpr int MW_WAVES = MW_THREADS / 64;
constexpr int MW_PER = (1 << MW_T) / 2 / MW_THREADS;     // double2 loads per thread of a full tile: 8
constexpr int MW_LDS = (1 << MW_T) + ((1 << MW_T) >> 4);  // padded doubles

__device__ __forceinline__ int mw_pad(int i) { return i + (i >> 4); }

// bit groups of the transform: group 0 = [0, min(n, T)), then groups of at most MW_H bits
struct MmdPlan {
  int P;
  int lo[8], nb[8];
};
MmdPlan mmd_plan(int n) {
  MmdPlan p;
  p.P = 1;
  p.lo[0] = 0;
  p.nb[0] = n < MW_T ? n : MW_T;
  int rest = n - p.nb[0], lo = p.nb[0];
  const int groups = (rest + MW_H - 1) / MW_H;
  for (int i = 0; i < groups; ++i) {      // as even as the bits allow, so that rows stay long
    const int nb = (rest + (groups - i) - 1) / (groups - i);
    p.lo[p.P] = lo;
    p.nb[p.P] = nb;
    ++p.P;
    lo += nb;
    rest -= nb;
  }
  return p;
}

// one round of R butterfly stages over the tile-local bits [s, s + R) of 2^tb doubles in LDS
template <int R>
__device__ __forceinline__ void mw_round(double* __restrict__ tile, int tb, int s) {
  const int groups = 1 << (tb - R);
  const int lowmask = (1 << s) - 1;
  for (int g = threadIdx.x; g < groups; g += MW_THREADS) {
    const int base = ((g >> s) << (s + R)) | (g & lowmask);
    double v[1 << R];
#pragma unroll
    for (int j = 0; j < (1 << R); ++j) v[j] = tile[mw_pad(base + (j << s))];
#pragma unroll
    for (int b = 0; b < R; ++b) {
#pragma unroll
      for (int j = 0; j < (1 << R); ++j) {
        if (!(j & (1 << b))) {
          const double x = v[j], y = v[j | (1 << b)];
          v[j] = x + y;
          v[j | (1 << b)] = x - y;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < (1 << R); ++j) tile[mw_pad(base + (j << s))] = v[j];
  }
  __syncthreads();
}

// all stages of the tile-local bits [s0, s0 + nb): rounds of four bits, the last one shorter.  The tile must be visible
// (a barrier behind its last write); it is visible again on return.
__device__ __forceinline__ void mw_transform(double* __restrict__ tile, int tb, int s0, int nb) {
  int s = s0, left = nb;
  while (left >= 4) {
    mw_round<4>(tile, tb, s);
    s += 4;
    left -= 4;
  }
  if (left == 3) mw_round<3>(tile, tb, s);
  else if (left == 2) mw_round<2>(tile, tb, s);
  else if (left == 1) mw_round<1>(tile, tb, s);
}

// grid: one workgroup per tile.  The tile: 2^tb doubles, tile-local index i = (row << cb) | col; global index
// = hi_part(g) | (row << lo) | mid_part(g) | col with the bits [cb, lo) and [lo + nb, n) taken from the tile number g.
// (low pass: cb = 0, lo = 0, nb = tb.)  mode bit 0: subtract `target` on load (first pass); bit 1: the pass completes the forward
// transform (scale, partial, inverse); out may be null with bit 1 (loss only).  in == out is allowed (same tile, same lanes).
__global__ __launch_bounds__(MW_THREADS) void mmd_pass_kernel(const double* in, const double* __restrict__ target, double* out,
                                                              const double* __restrict__ lam, int n, int tb, int cb, int lo, int nb,
                                                              int mode, double scale, double loss_scale, double* __restrict__ part) {
  __shared__ double tile[MW_LDS];
  __shared__ double red[MW_WAVES];
  const long long g = blockIdx.x;
  const int midbits = lo - cb;                                   // tile-number bits that sit between the columns and the rows
  const long long gbase = (cb == 0 && lo == 0) ? (g << tb)
                                               : (((g >> midbits) << (lo + nb)) | ((g & ((1ll << midbits) - 1)) << cb));
  const int npairs = 1 << (tb - 1);                              // tb >= 1
  const int colmask = (1 << cb) - 1;
  const bool low = (lo == 0);

  double2 v[MW_PER];
#pragma unroll
  for (int it = 0; it < MW_PER; ++it) {
    const int p = threadIdx.x + it * MW_THREADS;
    if (p < npairs) {
      const int i = 2 * p;
      const long long a = low ? gbase + i : gbase + ((long long)(i >> cb) << lo) + (i & colmask);
      v[it] = *reinterpret_cast<const double2*>(in + a);
      if ((mode & 1) && target) {
        const double2 t = *reinterpret_cast<const double2*>(target + a);
        v[it].x -= t.x;
        v[it].y -= t.y;
      }
    }
  }
#pragma unroll
  for (int it = 0; it < MW_PER; ++it) {
    const int p = threadIdx.x + it * MW_THREADS;
    if (p < npairs) {
      const int q = mw_pad(2 * p);
      tile[q] = v[it].x;
      tile[q + 1] = v[it].y;
    }
  }
  __syncthreads();
  mw_transform(tile, tb, cb, nb);

  if (mode & 2) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int p = threadIdx.x; p < npairs; p += MW_THREADS) {
      const int i = 2 * p;
      const long long a = low ? gbase + i : gbase + ((long long)(i >> cb) << lo) + (i & colmask);
      const int q = mw_pad(i);
      const int pc = __popcll((unsigned long long)a);            // a is even: a + 1 has one bit more
      const double x0 = tile[q], x1 = tile[q + 1];
      const double y0 = lam[pc] * x0, y1 = lam[pc + 1] * x1;
      const double t0 = y0 * x0, t1 = y1 * x1;
      acc = (acc + t0) + t1;
      tile[q] = y0 * scale;                                      // a power of two: exact
      tile[q + 1] = y1 * scale;
    }
    acc = block_sum<MW_WAVES>(acc, red);                         // (its barriers make the scaled tile visible)
    if (threadIdx.x == 0) part[g] = gridDim.x == 1 ? acc * loss_scale : acc;
    if (!out) return;
    mw_transform(tile, tb, cb, nb);
  }

#pragma unroll
  for (int it = 0; it < MW_PER; ++it) {
    const int p = threadIdx.x + it * MW_THREADS;
    if (p < npairs) {
      const int i = 2 * p;
      const long long a = low ? gbase + i : gbase + ((long long)(i >> cb) << lo) + (i & colmask);
      const int q = mw_pad(i);
      double2 o;
      o.x = tile[q];
      o.y = tile[q + 1];
      *reinterpret_cast<double2*>(out + a) = o;
    }
  }
}

// one workgroup: loss = 2^-n * (the partials in the fixed order)
__global__ __launch_bounds__(MW_THREADS) void mmd_finish_kernel(const double* __restrict__ part, int count, double loss_scale,
                                                                double* __restrict__ loss) {
  __shared__ double red[MW_WAVES];
  const double s = sum_partials<MW_THREADS>(part, count, red);
  if (threadIdx.x == 0) loss[0] = s * loss_scale;
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int HP_THREADS = 128;                   // rows of a workgroup: a histogram column of up to 64 bins each = 32 KiB
constexpr int HP_TILE = 512;                      // columns of an LDS tile
constexpr int HP_BINS = 64;
constexpr long long HP_TARGET_WG = 1024;          // workgroups aimed at: the columns are split until there are about as many
constexpr int HF_THREADS = 256;
constexpr int HF_WAVES = HF_THREADS / 64;

struct HpGeom {
  long long row_blocks, cols;   // columns per range (a multiple of HP_TILE)
  int G;                        // column ranges
};
HpGeom hp_geom(long long A, long long B) {
  HpGeom g;
  g.row_blocks = (A + HP_THREADS - 1) / HP_THREADS;
  long long max_wg = HP_TARGET_WG / g.row_blocks;
  if (max_wg < 1) max_wg = 1;
  const ChunkGeom c = chunk_geom(B, HP_TILE, max_wg, HP_TILE);
  g.cols = c.chunk;
  g.G = c.G;
  return g;
}

// grid (row blocks, G).  part int32 [G][n + 1][A]: the counts of this column range, every entry written.
__global__ __launch_bounds__(HP_THREADS) void hamming_pairs_kernel(int n, long long A, const long long* __restrict__ za, long long B,
                                                                   const long long* __restrict__ zb, long long cols, int skip,
                                                                   int* __restrict__ part) {
  __shared__ int hist[HP_BINS * HP_THREADS];
  __shared__ unsigned long long tile[HP_TILE];
  const int lane = threadIdx.x;
  const long long a = (long long)blockIdx.x * HP_THREADS + lane;
  const unsigned long long mask = n >= 64 ? ~0ull : ((1ull << n) - 1ull);     // n <= 63: at most 63 set bits, bins 0 .. n
  const unsigned long long x = a < A ? ((unsigned long long)za[a] & mask) : 0ull;
  for (int d = 0; d <= n; ++d) hist[d * HP_THREADS + lane] = 0;
  const long long c0 = (long long)blockIdx.y * cols, c1 = c0 + cols < B ? c0 + cols : B;
  for (long long t0 = c0; t0 < c1; t0 += HP_TILE) {
    const int cnt = (int)(c1 - t0 < HP_TILE ? c1 - t0 : HP_TILE);
    __syncthreads();                                             // the tile's readers of the round before
    for (int j = lane; j < cnt; j += HP_THREADS) tile[j] = (unsigned long long)zb[t0 + j] & mask;
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < cnt; ++j) {
      const int d = __popcll(x ^ tile[j]);
      atomicAdd(&hist[d * HP_THREADS + lane], 1);                // an integer LDS add on the lane's own column
    }
  }
  if (skip && a < A && a >= c0 && a < c1) {                      // the pair with the row's own index lies in this range
    const int d = __popcll(x ^ ((unsigned long long)zb[a] & mask));
    atomicAdd(&hist[d * HP_THREADS + lane], -1);
  }
  if (a < A)
    for (int d = 0; d <= n; ++d) part[((long long)blockIdx.y * (n + 1) + d) * A + a] = hist[d * HP_THREADS + lane];
}

// grid (ceil(A / 256)): the ranges' counts added, r_a, the optional counts [A, n + 1], one partial of the total per workgroup
__global__ __launch_bounds__(HF_THREADS) void hamming_pairs_finish_kernel(int n, long long A, int G, const int* __restrict__ part,
                                                                          const double* __restrict__ kappa, double* __restrict__ r,
                                                                          int* __restrict__ counts, double* __restrict__ tpart) {
  // (no fused multiply-add: the header states a separately rounded multiply and add, which a NumPy mirror reproduces)
#pragma clang fp contract(off)
  __shared__ double red[HF_WAVES];
  const long long a = (long long)blockIdx.x * HF_THREADS + threadIdx.x;
  double acc = 0.0;
  if (a < A) {
    for (int d = 0; d <= n; ++d) {
      int c = 0;
      for (int g = 0; g < G; ++g) c += part[((long long)g * (n + 1) + d) * A + a];
      if (counts) counts[a * (n + 1) + d] = c;
      const double term = kappa[d] * (double)c;      // (plain operators: the pragma above governs them, not a callee's body)
      acc = acc + term;
    }
    r[a] = acc;
  }
  acc = block_sum<HF_WAVES>(acc, red);
  if (threadIdx.x == 0) tpart[blockIdx.x] = acc;
}

__global__ __launch_bounds__(HF_THREADS) void hamming_pairs_total_kernel(const double* __restrict__ tpart, int count,
                                                                         double* __restrict__ total) {
  __shared__ double red[HF_WAVES];
  const double s = sum_partials<HF_THREADS>(tpart, count, red);
  if (threadIdx.x == 0) total[0] = s;
}

}  // namespace

// ---- bornvi_mmd_weights ---------------------------------------------------------------------------------------------
int mmd_passes(int n) { return 2 * mmd_plan(n).P - 1; }

static long long mmd_partials(int n) { return n <= MW_T ? 1 : (1ll << (n - MW_T)); }

size_t mmd_workspace_bytes(int n) {
  // partials of the pass that completes the forward transform; the 2^n doubles between passes when w is not given
  const size_t scratch = n > MW_T ? ws_round(sizeof(double) << n) : 0;
  return ws_round((size_t)mmd_partials(n) * sizeof(double)) + scratch + 256;
}

hipError_t launch_mmd_weights(int n, const double* q, const double* target, const double* lam, double* loss, double* w, void* ws,
                              hipStream_t st) {
  const MmdPlan pl = mmd_plan(n);
  double* part = (double*)ws_align(ws);
  double* buf = w ? w : (double*)((char*)part + ws_round((size_t)mmd_partials(n) * sizeof(double)));
  const double scale = std::ldexp(1.0, 1 - n), loss_scale = std::ldexp(1.0, -n);
  if (pl.P == 1) {     // the whole vector is one tile
    mmd_pass_kernel<<<1, MW_THREADS, 0, st>>>(q, target, w, lam, n, n, 0, 0, n, 3, scale, loss_scale, loss);
    return hipGetLastError();
  }
  const unsigned tiles = (unsigned)(1ll << (n - MW_T));
  auto pass = [&](int gi, const double* in, double* out, int mode) {
    const int cb = gi == 0 ? 0 : MW_T - pl.nb[gi];
    mmd_pass_kernel<<<tiles, MW_THREADS, 0, st>>>(in, target, out, lam, n, MW_T, cb, pl.lo[gi], pl.nb[gi], mode, scale, loss_scale, part);
  };
  pass(0, q, buf, 1);
  for (int gi = 1; gi < pl.P - 1; ++gi) pass(gi, buf, buf, 0);
  pass(pl.P - 1, buf, w ? buf : nullptr, 2);
  mmd_finish_kernel<<<1, MW_THREADS, 0, st>>>(part, (int)tiles, loss_scale, loss);
  if (w)
    for (int gi = pl.P - 2; gi >= 0; --gi) pass(gi, buf, buf, 0);
  return hipGetLastError();
}

// ---- bornvi_hamming_pairs_rowsum ------------------------------------------------------------------------------------
size_t hamming_pairs_workspace_bytes(int n, long long A, long long B) {
  const HpGeom g = hp_geom(A, B);
  const size_t finish_wg = (size_t)((A + HF_THREADS - 1) / HF_THREADS);
  return ws_round((size_t)g.G * (n + 1) * A * sizeof(int)) + ws_round(finish_wg * sizeof(double)) + 256;
}

hipError_t launch_hamming_pairs_rowsum(int n, long long A, const long long* za, long long B, const long long* zb, int skip_same_index,
                                       const double* kappa, double* r, double* total, int* counts, void* ws, hipStream_t st) {
  const HpGeom g = hp_geom(A, B);
  int* part = (int*)ws_align(ws);
  double* tpart = (double*)((char*)part + ws_round((size_t)g.G * (n + 1) * A * sizeof(int)));
  const unsigned finish_wg = (unsigned)((A + HF_THREADS - 1) / HF_THREADS);
  hamming_pairs_kernel<<<dim3((unsigned)g.row_blocks, (unsigned)g.G), HP_THREADS, 0, st>>>(n, A, za, B, zb, g.cols, skip_same_index, part);
  hamming_pairs_finish_kernel<<<finish_wg, HF_THREADS, 0, st>>>(n, A, g.G, part, kappa, r, counts, tpart);
  hamming_pairs_total_kernel<<<1, HF_THREADS, 0, st>>>(tpart, (int)finish_wg, total);
  return hipGetLastError();
}

}  // namespace bornvi
