// The split-K SYRK core of the two Gram kernels (gfx950): bornvi_fisher_gram (kernels_fisher.hip) instantiates all of it;
// bornvi_qfi_gram (kernels_qfi.hip) takes its geometry, tile-pair decode, MFMA k-step and finisher sum and keeps the slab
// loop of split_k written out (reason: there).  G = X X^T over R rows of K columns on v_mfma_f64_16x16x4_f64, grid
// (upper-triangle tile pairs) x (G groups of column slabs):
//   output tile T x T, T = 32 MT, per workgroup of 4 waves (2 x 2; a wave owns MT x MT MFMA tiles of 16 x 16);
//   a slab is at most 4096 columns (geometry: geom); k-step 16, LDS double-buffered, one barrier per k-step, the next
//   k-step's operands in flight in registers during the MFMAs (16-byte loads: a thread owns MT rows of each side and
//   two columns of the k-step);
//   LDS rows padded to 18 doubles (pitch 144 bytes, 16-byte aligned for the b128 stores): the 16 rows x 2 k a half-wave
//   reads with ds_read_b64 sit at dwords 36 r + 2 k mod 64 -- 32 distinct 8-byte slots, no bank conflict.
// Each slab starts from a zero accumulator (a chain of at most 4096 additions inside the MFMAs), the workgroup adds its
// slabs' results one after the other -- split_k: in registers; the QFI kernel: in its partial tile in the workspace --
// and the finishing launch adds the G <= 256 (64 up to 2^28 columns) partial tiles of an entry in index order
// (sum_partials): no atomics, bitwise reproducible.  Only tiles with tile_i <= tile_j are computed.
// What an instantiation of split_k supplies is its "row source", which owns what goes into LDS:
//   load(z0, k0, slab)        this k-step's operands (columns z0 + k0 ..) into the source's registers;
//   begin_slab(z0, slab, len) once per slab, after the first load and before the first store (per-slab tables);
//   store(As, Bs, buf, k0)    the registers into buffer `buf` of As (row side) and Bs (column side).
// Fragment layout of the f64 MFMA as in kernels_batched.hip: A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15], D[row = (lane >> 4) + 4 r][col = lane & 15].
#pragma once
#include <hip/hip_runtime.h>

namespace bornvi {
namespace syrk {

constexpr int BK = 16, PITCH = 18, THREADS = 256;
constexpr int SLAB_MAX = 4096, GROUPS = 64;
typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

struct Geom {
  long long slab;      // columns per slab (<= 4096)
  long long per_wg;    // slabs a workgroup adds up one after the other
  int G;               // workgroups along the columns = partial tiles per entry
  int T;               // tiles per side
  int tiles;           // T (T + 1) / 2
};

// K columns (a power of two), R rows, tiles of `edge` rows.
inline Geom geom(long long K, int R, int edge) {
  Geom g;
  g.slab = K <= 256 ? K : (K / 64 < 256 ? 256 : (K / 64 > SLAB_MAX ? SLAB_MAX : K / 64));
  const long long nslab = K / g.slab;
  const long long gmax = nslab / 1024 > GROUPS ? nslab / 1024 : GROUPS;     // (per_wg <= 1024: 2^29 columns take more groups)
  g.G = (int)(nslab < gmax ? nslab : gmax);
  g.per_wg = nslab / g.G;
  g.T = (R + edge - 1) / edge;
  g.tiles = g.T * (g.T + 1) / 2;
  return g;
}
inline size_t workspace_bytes(const Geom& g, int edge) { return (size_t)g.G * g.tiles * edge * edge * sizeof(double) + 512; }
constexpr size_t tiles_lds_bytes(int edge) { return (size_t)(4 * edge * PITCH) * sizeof(double); }   // As and Bs, two buffers each

// Tile pair (ti <= tj) number `pair`, row by row, and back.
__device__ __forceinline__ void tile_pair(int pair, int T, int& ti, int& tj) {
  int rem = pair;
  ti = 0;
  while (rem >= T - ti) { rem -= T - ti; ++ti; }
  tj = ti + rem;
}
__device__ __forceinline__ long long tile_pair_index(int ti, int tj, int T) {
  return (long long)ti * T - (long long)ti * (ti - 1) / 2 + (tj - ti);
}

// One k-step of a wave: acc[mi][ni] += A tile mi x B tile ni over the BK columns in LDS, Ac / Bc the lane's fragment
// addresses in the current buffer.
template <int MT>
__device__ __forceinline__ void mfma_k_step(const double* __restrict__ Ac, const double* __restrict__ Bc, d4 (&acc)[MT][MT]) {
#pragma unroll
  for (int ks = 0; ks < BK / 4; ++ks) {
    double a[MT], b[MT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) a[mi] = Ac[mi * 16 * PITCH + ks * 4];
#pragma unroll
    for (int ni = 0; ni < MT; ++ni) b[ni] = Bc[ni * 16 * PITCH + ks * 4];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < MT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
  }
}

// grid (tiles, G).  part[(g * tiles + tile) * T * T + row * T + col], T = 32 MT.  As, Bs: [2][T][PITCH] each.
template <int MT, class Rows>
__device__ __forceinline__ void split_k(Rows& rows, double* __restrict__ As, double* __restrict__ Bs, long long slab,
                                        long long per_wg, double* __restrict__ part) {
  constexpr int T = 32 * MT, W = 16 * MT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = wave & 1, wj = wave >> 1;
  const long long len16 = (slab + BK - 1) / BK * BK;                  // (a slab shorter than a k-step)
  const long long nk = len16 / BK;
  const int fr = lane & 15, fk = lane >> 4;
  // D[row = fk + 4 r][col = fr] of MFMA tile (mi, ni): tile entry (wi * W + mi * 16 + fk + 4 r, wj * W + ni * 16 + fr)
  double* __restrict__ tile = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (T * T);
  const int mine = (wi * W + fk) * T + wj * W + fr;
  d4 total[MT][MT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < MT; ++ni) total[mi][ni] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (long long s = 0; s < per_wg; ++s) {
    const long long z0 = ((long long)blockIdx.y * per_wg + s) * slab;
    rows.load(z0, 0, slab);
    // (the previous slab's last k-step ended with a barrier: nobody reads the tiles or the source's tables any more)
    rows.begin_slab(z0, slab, len16);
    rows.store(As, Bs, 0, 0);
    __syncthreads();
    d4 acc[MT][MT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < MT; ++ni) acc[mi][ni] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (long long kt = 0; kt < nk; ++kt) {
      const int cur = (int)(kt & 1);
      if (kt + 1 < nk) rows.load(z0, (kt + 1) * BK, slab);            // in flight during this k-step's MFMAs
      const double* __restrict__ Ac = As + (cur * T + wi * W + fr) * PITCH + fk;
      const double* __restrict__ Bc = Bs + (cur * T + wj * W + fr) * PITCH + fk;
      mfma_k_step<MT>(Ac, Bc, acc);
      if (kt + 1 < nk) rows.store(As, Bs, cur ^ 1, (kt + 1) * BK);
      __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < MT; ++ni) total[mi][ni] += acc[mi][ni];
  }
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < MT; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[mine + (mi * 16 + 4 * r) * T + ni * 16] = total[mi][ni][r];
}

// One entry of the finishing launches: its G partials (`stride` doubles apart) added in index order.
__device__ __forceinline__ double sum_partials(const double* __restrict__ p, int G, long long stride) {
  double sum = 0.0;
  for (int g = 0; g < G; ++g) sum += p[g * stride];
  return sum;
}

}  // namespace syrk
}  // namespace bornvi
