// Sampled KSD: the Stein score of p at sampled states and the B x B pairwise Stein kernel of the
// samples reduced to row sums.  Nothing here touches 2^n of anything: 1 <= n <= 63.
//
// bornvi_bn_score_samples:  S[b, i] = 1 - prod_v max(f_v(flip_i z_b), p_floor) / max(f_v(z_b), p_floor), one lane per sample.
//   Only node i's own factor and its children's differ from 1: a 64-bit node mask per latent position, built once per
//   workgroup in LDS from the descriptor's parent lists.  The product runs over the mask's nodes in descriptor order, one
//   quotient per node (k quotients, k - 1 products, one subtraction).  logp, when asked for, is bn_logjoint_kernel's
//   expression in its order: the two outputs are bit-equal.  No |p| < 1e-12 -> zero-row rule (at n = 60 every joint is
//   below 1e-12).  A summed-out node makes the sample's outputs NaN (the host refuses it where it can look).
//
// bornvi_stein_pairs_rowsum:  r_b = sum_{b' != b} k_p(z_b, z_b'),  total = sum_b r_b;  b' != b by SAMPLE INDEX.
//   With a = exp(-1/(n l)), h = sinh(1/(n l)), m = 1 - cosh(1/(n l)) = -2 sinh^2(1/(2 n l)), sigma = 1 - 2 z, t = sigma s,
//   d = popcount(idx ^ idx'):
//     k_p = a^d [ s.s' - h t.t' + h (t - sigma).(t' - sigma') + h (n - 2 d) + m (n - sum s) + m (n - sum s') ]
//   -- one Gram over 3 n features per sample (inner dimension padded to 4 KS, KS = 12, 24, 36, 48 for n <= 16, 32, 48, 63),
//   a popcount, a row constant and a column constant.  The sum of the absolute values of these terms is at most 4 x the
//   closed form's (tests/test_ksd_sampled_host.py) for n l >= 1, which is why n l < 1 is refused.
//   stein_pairs_prep_kernel: rc[b] = m (n - sum_i s_bi), i in order.
//   stein_pairs_kernel, grid (ceil(B / 64), G): a workgroup of four waves owns 64 rows, 16 per wave, whose feature rows
//   [s, t, t - sigma] stay in registers as the A fragments of v_mfma_f64_16x16x4_f64 (KS doubles per lane), and walks its
//   range of 32-column tiles.  A tile's feature rows [s', -h t', h (t' - sigma')] are built in LDS from idx and S (the next
//   tile's S and idx are in flight in registers during the MFMAs): no [B, 3 n] array goes to memory.  LDS rows have pitch
//   4 KS + 2 doubles: the 16 columns x 2 k a half-wave reads with ds_read_b64 sit at dwords 4 c + 2 k mod 64.
//   Epilogue per 16 x 16 tile: d by a 64-bit popcount, a^d and h (n - 2 d) from 64-entry tables in LDS (made on the host in
//   long double), kappa = pw[d] (((acc + hd[d]) + rc_row) + rc_col), masked by row != col, row < B, col < B, added to the
//   lane's four row sums: tiles in order, the two MFMA tiles of a tile in order.  After the last tile a butterfly over the 16
//   lanes of a row (offsets 8, 4, 2, 1) and one store per row into part[g][row].
//   stein_pairs_finish_kernel, one workgroup: r_b = part[0][b] + part[1][b] + ... in index order; total: every thread adds
//   its r_b (b = t, t + 256, ...) in order, a 64-lane butterfly, the four waves in order.
//   G depends on B only (kp_geom).  No atomics, no allocation, no synchronisation: capturable, two calls bitwise equal.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace bornvi {

namespace {
constexpr int KP_ROWS = 64;          // rows of a workgroup: 16 per wave
constexpr int KP_TC = 32;            // columns of a tile
constexpr int KP_THREADS = 256;
constexpr int KP_GMAX = 64;          // column ranges (= partial rows in the workspace) at most
constexpr int KP_TARGET_WG = 1024;   // workgroups the column split aims for

typedef double kp_d4 __attribute__((ext_vector_type(4)));

struct KpConsts {
  double pw[64];   // a^d
  double hd[64];   // h (n - 2 d)
  double h, m;
};

struct KpGeom {
  int rb, tiles, per, G;   // row blocks, column tiles, tiles per column range, column ranges
};

KpGeom kp_geom(long long B) {
  KpGeom g;
  g.rb = (int)((B + KP_ROWS - 1) / KP_ROWS);
  g.tiles = (int)((B + KP_TC - 1) / KP_TC);
  int want = (KP_TARGET_WG + g.rb - 1) / g.rb;
  if (want > KP_GMAX) want = KP_GMAX;
  if (want > g.tiles) want = g.tiles;
  if (want < 1) want = 1;
  g.per = (g.tiles + want - 1) / want;
  g.G = (g.tiles + g.per - 1) / g.per;
  return g;
}

__device__ __forceinline__ double bn_factor(const bornvi_bn_desc& bn, int v, unsigned long long vals) {
  int cfg = 0;
  const int np = bn.n_parents[v];
  for (int p = 0; p < np; ++p) cfg = cfg * 2 + (int)((vals >> bn.parents[v * bn.max_parents + p]) & 1ull);
  return bn.cpt[bn.cpt_off[v] + 2 * cfg + (int)((vals >> v) & 1ull)];
}

// ---- scores of p at sampled states -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_score_samples_kernel(bornvi_bn_desc bn, int n, long long B, const long long* __restrict__ idx,
                                                               double p_floor, double* __restrict__ S, double* __restrict__ logp) {
  __shared__ unsigned long long mask[64];   // latent position i: node i itself and its children
  __shared__ int node_of[64];
  const int t = threadIdx.x;
  if (t < 64) {
    int vi = -1;
    unsigned long long mk = 0ull;
    if (t < n) {
      for (int v = 0; v < bn.num_nodes; ++v)
        if (bn.role[v] == t) vi = v;
      if (vi >= 0) {
        mk = 1ull << vi;
        for (int v = 0; v < bn.num_nodes; ++v) {
          const int np = bn.n_parents[v];
          for (int p = 0; p < np; ++p)
            if (bn.parents[v * bn.max_parents + p] == vi) mk |= 1ull << v;
        }
      }
    }
    node_of[t] = vi;
    mask[t] = mk;
  }
  __syncthreads();
  const long long b = (long long)blockIdx.x * blockDim.x + t;
  if (b >= B) return;
  const unsigned long long z = (unsigned long long)idx[b];
  unsigned long long vals = 0;   // bit v = value of node v
  bool bad = false;
  for (int v = 0; v < bn.num_nodes; ++v) {
    const int role = bn.role[v];
    unsigned long long bit = 0ull;
    if (role >= 0 && role < n) bit = (z >> (n - 1 - role)) & 1ull;
    else if (role == -2) bit = 1ull;
    else if (role != -1) bad = true;           // a summed-out node: the host refuses it where it can look
    vals |= bit << v;
  }
  if (logp) {
    double sum = 0.0;
    for (int v = 0; v < bn.num_nodes; ++v) sum += log(fmax(bn_factor(bn, v, vals), p_floor));
    logp[b] = bad ? __builtin_nan("") : sum;
  }
  for (int i = 0; i < n; ++i) {
    const int vi = node_of[i];
    unsigned long long mk = mask[i];
    const unsigned long long flipped = vi >= 0 ? vals ^ (1ull << vi) : vals;
    double ratio = 1.0;
    while (mk) {
      const int v = __builtin_ctzll(mk);
      mk &= mk - 1ull;
      ratio *= fmax(bn_factor(bn, v, flipped), p_floor) / fmax(bn_factor(bn, v, vals), p_floor);
    }
    S[b * n + i] = bad ? __builtin_nan("") : 1.0 - ratio;
  }
}

// ---- pairwise Stein kernel, row sums ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stein_pairs_prep_kernel(int n, long long B, const double* __restrict__ S, double m,
                                                               double* __restrict__ rc) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double sum = 0.0;
  for (int i = 0; i < n; ++i) sum += S[b * n + i];
  rc[b] = m * ((double)n - sum);
}

template <int KS>
__global__ __launch_bounds__(KP_THREADS) void stein_pairs_kernel(int n, long long B, int tiles, int per,
                                                                 const long long* __restrict__ idx, const double* __restrict__ S,
                                                                 const double* __restrict__ rc, KpConsts c,
                                                                 double* __restrict__ part) {
  constexpr int P = 4 * KS + 2;        // LDS row pitch in doubles
  constexpr int NE = KS / 6;           // S values of a tile per thread: 32 n <= 256 NE
  __shared__ double Bs[KP_TC * P];
  __shared__ unsigned long long Cz[KP_TC];
  __shared__ double Cc[KP_TC];
  __shared__ double pw[64];
  __shared__ double hd[64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fr = lane & 15, fk = lane >> 4;
  const int n3 = 3 * n;
  const unsigned long long zmask = (1ull << n) - 1ull;
  const long long total_s = B * n;
  // the wave's 16 rows as A fragments: A[row = fr][k = 4 ks + fk], feature f = c n + i: s_i, t_i, t_i - sigma_i
  const long long wrow0 = (long long)blockIdx.x * KP_ROWS + wave * 16;
  double a[KS];
  {
    const long long row = wrow0 + fr;
    const bool ok = row < B;
    const unsigned long long z = ok ? (unsigned long long)idx[row] : 0ull;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int f = 4 * ks + fk;
      double v = 0.0;
      if (ok && f < n3) {
        const int cls = f >= 2 * n ? 2 : (f >= n ? 1 : 0);
        const int i = f - cls * n;
        const double s = S[row * n + i];
        const double sg = ((z >> (n - 1 - i)) & 1ull) ? -1.0 : 1.0;
        const double ts = sg * s;
        v = cls == 0 ? s : (cls == 1 ? ts : ts - sg);
      }
      a[ks] = v;
    }
  }
  // the lane's four output rows: D[row = fk + 4 r][col = fr]
  unsigned long long rz[4];
  double rcr[4], rs[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long row = wrow0 + fk + 4 * r;
    rz[r] = row < B ? (unsigned long long)idx[row] : 0ull;
    rcr[r] = row < B ? rc[row] : 0.0;
    rs[r] = 0.0;
  }
  if (t < 64) {
    pw[t] = c.pw[t];
    hd[t] = c.hd[t];
  }
  for (int e = t; e < KP_TC * P; e += KP_THREADS) Bs[e] = 0.0;      // the padding features stay 0
  const int tile0 = blockIdx.y * per;
  const int tile1 = tile0 + per < tiles ? tile0 + per : tiles;
  // registers of the tile in flight
  double sv[NE];
  unsigned long long zv[NE];
  int colv[NE];
  unsigned long long zc = 0ull;
  double cc = 0.0;
  auto load = [&](int tile) {
    const long long c0 = (long long)tile * KP_TC;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int e = t + KP_THREADS * j;
      const int col = e / n;
      const long long g = c0 * n + e;
      const bool ok = col < KP_TC && g < total_s;
      colv[j] = col < KP_TC ? col : -1;
      sv[j] = ok ? S[g] : 0.0;
      zv[j] = ok ? (unsigned long long)idx[c0 + col] : 0ull;
      if (!ok && col < KP_TC) colv[j] = -2 - col;                  // a column past B: zeros
    }
    if (t < KP_TC) {
      const bool ok = c0 + t < B;
      zc = ok ? (unsigned long long)idx[c0 + t] : 0ull;
      cc = ok ? rc[c0 + t] : 0.0;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int cv = colv[j];
      if (cv == -1) continue;
      const bool ok = cv >= 0;
      const int col = ok ? cv : -2 - cv;
      const int i = t + KP_THREADS * j - col * n;
      const double s = sv[j];
      const double sg = ((zv[j] >> (n - 1 - i)) & 1ull) ? -1.0 : 1.0;
      const double ts = sg * s;
      double* dst = Bs + col * P + i;
      dst[0] = ok ? s : 0.0;
      dst[n] = ok ? -(c.h * ts) : 0.0;
      dst[2 * n] = ok ? c.h * (ts - sg) : 0.0;
    }
    if (t < KP_TC) {
      Cz[t] = zc;
      Cc[t] = cc;
    }
  };
  if (tile0 < tile1) load(tile0);
  __syncthreads();                     // the zeros are down before the first tile's features
  if (tile0 < tile1) store();
  __syncthreads();
#pragma unroll 1
  for (int tile = tile0; tile < tile1; ++tile) {
    if (tile + 1 < tile1) load(tile + 1);                           // in flight during this tile's MFMAs
    kp_d4 acc[2];
    acc[0] = (kp_d4){0.0, 0.0, 0.0, 0.0};
    acc[1] = (kp_d4){0.0, 0.0, 0.0, 0.0};
    const double* __restrict__ Bc = Bs + fr * P + fk;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const double b0 = Bc[4 * ks], b1 = Bc[16 * P + 4 * ks];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b1, acc[1], 0, 0, 0);
    }
    const long long c0 = (long long)tile * KP_TC;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long long col = c0 + 16 * j + fr;
      const unsigned long long cz = Cz[16 * j + fr];
      const double ccol = Cc[16 * j + fr];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long row = wrow0 + fk + 4 * r;
        const int d = __popcll((rz[r] ^ cz) & zmask);          // (bits above n never index past the tables)
        const double kap = pw[d] * (((acc[j][r] + hd[d]) + rcr[r]) + ccol);
        if (row < B && col < B && row != col) rs[r] += kap;
      }
    }
    __syncthreads();                   // everybody is done with this tile
    if (tile + 1 < tile1) store();
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double v = rs[r];     // (a 16-lane sum written out: as a call the kernel's instruction stream differs, profiles/reduce_core_isa.txt)
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const long long row = wrow0 + fk + 4 * r;
    if (fr == 0 && row < B) part[(long long)blockIdx.y * B + row] = v;
  }
}

__global__ __launch_bounds__(KP_THREADS) void stein_pairs_finish_kernel(long long B, int G, const double* __restrict__ part,
                                                                        double* __restrict__ r, double* __restrict__ total) {
  __shared__ double red[KP_THREADS / 64];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (long long b = t; b < B; b += KP_THREADS) {
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += part[(long long)g * B + b];
    r[b] = sum;
    acc += sum;
  }
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) total[0] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct KpLayout {
  size_t rc, part, total;
};
KpLayout kp_layout(long long B, int G) {
  KpLayout L;
  size_t o = 0;
  L.rc = o;   o += ws_round((size_t)B * sizeof(double));
  L.part = o; o += ws_round((size_t)G * B * sizeof(double));
  L.total = o;
  return L;
}
}  // namespace

size_t stein_pairs_workspace_bytes(long long B) { return kp_layout(B, kp_geom(B).G).total + 256; }

void stein_pairs_geometry(long long B, int* per_tiles, int* G) {
  const KpGeom g = kp_geom(B);
  *per_tiles = g.per;
  *G = g.G;
}

hipError_t launch_bn_score_samples(const bornvi_bn_desc& bn, int n, long long B, const long long* idx, double p_floor, double* S,
                                   double* logp, hipStream_t st) {
  bn_score_samples_kernel<<<(unsigned)((B + 255) / 256), 256, 0, st>>>(bn, n, B, idx, p_floor, S, logp);
  return hipGetLastError();
}

hipError_t launch_stein_pairs_rowsum(int n, long long B, double length_scale, const long long* idx, const double* S, double* r,
                                     double* total, void* ws, hipStream_t st) {
  const KpGeom g = kp_geom(B);
  const KpLayout L = kp_layout(B, g.G);
  char* base = ws_align(ws);
  double* rc = (double*)(base + L.rc);
  double* part = (double*)(base + L.part);
  // the constants in long double, rounded once
  KpConsts c;
  const long double x = 1.0L / ((long double)n * (long double)length_scale);
  const long double hl = sinhl(x), sh = sinhl(0.5L * x);
  for (int d = 0; d < 64; ++d) {
    c.pw[d] = (double)expl(-(long double)d * x);
    c.hd[d] = (double)(hl * (long double)(n - 2 * d));
  }
  c.h = (double)hl;
  c.m = (double)(-2.0L * sh * sh);
  stein_pairs_prep_kernel<<<(unsigned)((B + 255) / 256), 256, 0, st>>>(n, B, S, c.m, rc);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)g.rb, (unsigned)g.G);
  if (n <= 16) stein_pairs_kernel<12><<<grid, KP_THREADS, 0, st>>>(n, B, g.tiles, g.per, idx, S, rc, c, part);
  else if (n <= 32) stein_pairs_kernel<24><<<grid, KP_THREADS, 0, st>>>(n, B, g.tiles, g.per, idx, S, rc, c, part);
  else if (n <= 48) stein_pairs_kernel<36><<<grid, KP_THREADS, 0, st>>>(n, B, g.tiles, g.per, idx, S, rc, c, part);
  else stein_pairs_kernel<48><<<grid, KP_THREADS, 0, st>>>(n, B, g.tiles, g.per, idx, S, rc, c, part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  stein_pairs_finish_kernel<<<1, KP_THREADS, 0, st>>>(B, g.G, part, r, total);
  return hipGetLastError();
}

}  // namespace bornvi
