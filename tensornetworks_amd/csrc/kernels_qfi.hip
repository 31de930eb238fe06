// Quantum natural gradient (gfx950): phase-coherent statevectors of the pi-shifted circuits out of the batched circuit
// engine (the helpers of bornvi_paramshift_states) and the quantum Fisher information matrix (bornvi_qfi_gram).
//
// ---- helpers of bornvi_paramshift_states (api.hip).  The batched engine runs a "state plan" (plan.cpp: make_state_plan)
// with RAW fused matrices -- no pivot normalisation, so no phase is lost -- on the 16-amplitude or the generic pass kernel;
// its last pass writes the state BEFORE the gates that end the circuit (the CNOT ring and the CZs after the last
// rotation), which the probability plans fold into the outcome index or drop.
//   pi_shift_thetas_kernel: thetas[c][p] = theta[p] + (p == parameter of circuit c ? pi : 0): the batch of parameter
//     vectors the engine's own gate builder (build_gates_kernel, untouched) turns into matrices;
//   state_tail_kernel: out[y] = s(y) in[A y] -- the tail gates as ONE GF(2)-linear gather (the CNOTs) and one sign (the
//     CZs, a quadratic form over the bits of y), from the engine's ping-pong buffer into the caller's rows, canonical
//     order: 16-byte gathers, coalesced 16-byte stores, one thread per amplitude.
//
// ---- bornvi_qfi_gram: Q_ab = Re<phi_a|phi_b> - Re(conj(c_a) c_b), c_a = <psi|phi_a>.  A complex128 row of 2^n amplitudes
// is a real row of K = 2^(n+1) doubles, Re<phi_a|phi_b> the real dot product of two such rows, Re c_a the dot product
// with psi and Im c_a the one with i psi = (-Im psi, Re psi): ONE real SYRK over R = P + 2 rows (phi_0 .. phi_{P-1}, psi,
// i psi) -- the split-K SYRK of syrk_f64.hpp (layout, barriers, order of the sums: there; this kernel writes split_k's
// slab loop out and shares the rest), with
//   output tile 128 x 128 (a wave owns 64 x 64 = 4 x 4 MFMA tiles: one ds_read_b64 feeds two MFMAs, 128 accumulator
//   registers; with the operands of a whole k-step in flight the kernel takes 256 VGPRs + 228 AGPRs, ONE wave per SIMD
//   -- held to two waves it spills 84 registers or more, so it is not);
//   what goes into LDS: the rows as they are (row i psi: the pair exchanged and one sign flipped, exact), so a product
//   carries the rounding of the product alone; 8 16-byte loads per thread and k-step; 2 x 2 x 128 x 18 x 8 = 72 KiB;
//   the running total over a workgroup's slabs in ITS partial tile in the workspace (first slab: stores, later slabs:
//   adds) -- in L2, not in 128 more registers;
//   a finisher, qfi_finish_kernel, that forms the projection term from the sums of the entries (a, psi), (a, i psi),
//   (b, psi), (b, i psi) (recomputed per workgroup, from the same partials in the same order: the same bits everywhere)
//   and writes Q_ab and Q_ba from the same value.  No atomics; bitwise reproducible; Q == Q^T bitwise.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "syrk_f64.hpp"

namespace bornvi {

namespace {
// ------------------------------------------------------------------------------------------------ state helpers
__global__ void pi_shift_thetas_kernel(const double* __restrict__ theta, int P, int row0, int include_base, int p_begin,
                                       int bc, double* __restrict__ thetas) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)bc * P) return;
  const int c = (int)(idx / P), p = (int)(idx % P);
  const int r = row0 + c - include_base;                 // < 0: the base circuit
  thetas[idx] = theta[p] + ((r >= 0 && p == p_begin + r) ? 3.14159265358979323846 : 0.0);
}

typedef double qs_d2 __attribute__((ext_vector_type(2)));

// grid (blocks over y, circuits).  out row c, entry y = s(y) * in row c, entry x(y); bit b of x = parity(y & T.row[b]);
// s(y) = (-1)^(sum_b y_b popcount(y & T.cz[b])).
__global__ __launch_bounds__(256) void state_tail_kernel(const qs_d2* __restrict__ in, qs_d2* __restrict__ out, int n, StateTail T) {
  const long long N = 1ll << n;
  const long long y = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= N) return;
  const unsigned yu = (unsigned)y;
  unsigned x = 0, sg = 0;
  for (int b = 0; b < n; ++b) {
    x |= (unsigned)(__popc(yu & T.row[b]) & 1) << b;
    sg ^= ((yu >> b) & 1u) & (unsigned)__popc(yu & T.cz[b]);
  }
  qs_d2 v = in[(long long)blockIdx.y * N + x];
  if (sg & 1u) v = -v;
  out[(long long)blockIdx.y * N + y] = v;
}

// ------------------------------------------------------------------------------------------------ QFI Gram
constexpr int QG_MT = 4, QG_T = 32 * QG_MT;                           // wave tile 4 x 4 MFMA tiles, workgroup tile 128 x 128
using syrk::d2;

// grid (tiles, G).  part[(g * tiles + tile) * 16384 + row * 128 + col].  Row r of the SYRK: r < P: phi row r; r == P:
// psi; r == P + 1: i psi; beyond: zero.  The slab loop is syrk::split_k's, written out: through the template and a row
// source the compiler took four more AGPRs (232) and bornvi_qfi_gram measured 0.6 % slower at n = 20, outside the span
// of two runs of the hand-written loop.
__global__ __launch_bounds__(syrk::THREADS) void qfi_gram_kernel(const double* __restrict__ phi, const double* __restrict__ psi,
                                                              long long K, int P, int T, long long slab, long long per_wg,
                                                              double* __restrict__ part) {
  extern __shared__ double qg_lds[];
  double* __restrict__ As = qg_lds;                                    // [2][QG_T][syrk::PITCH]
  double* __restrict__ Bs = As + 2 * QG_T * syrk::PITCH;               // [2][QG_T][syrk::PITCH]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wi = wave & 1, wj = wave >> 1;
  int ti, tj;
  syrk::tile_pair(blockIdx.x, T, ti, tj);
  const int lrow = t >> 3, lk = (t & 7) * 2;
  // the thread's 4 rows of each side: pointer (null: a zero row) and whether the row is i psi
  const double* ag[4];
  const double* bg[4];
  bool arot[4], brot[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int ra = ti * QG_T + lrow + 32 * u, rb = tj * QG_T + lrow + 32 * u;
    ag[u] = ra < P ? phi + (long long)ra * K + lk : (ra < P + 2 ? psi + lk : nullptr);
    bg[u] = rb < P ? phi + (long long)rb * K + lk : (rb < P + 2 ? psi + lk : nullptr);
    arot[u] = ra == P + 1;
    brot[u] = rb == P + 1;
  }
  const long long len16 = (slab + syrk::BK - 1) / syrk::BK * syrk::BK;         // (a slab shorter than a k-step: n <= 2)
  const long long nk = len16 / syrk::BK;
  const d2 zero2 = (d2){0.0, 0.0};
  d2 av[4], bv[4];
#define QG_LOAD_TILES(z0, k0)                                                                \
  {                                                                                          \
    const bool zok = (k0) + lk < slab;                                                       \
    const long long zoff = (z0) + (k0);                                                      \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                          \
      av[u] = (zok && ag[u]) ? *reinterpret_cast<const d2*>(ag[u] + zoff) : zero2;           \
      bv[u] = (zok && bg[u]) ? *reinterpret_cast<const d2*>(bg[u] + zoff) : zero2;           \
    }                                                                                        \
  }
  // (i psi)[2 z] = -Im psi_z, (i psi)[2 z + 1] = Re psi_z: lk is even, so a thread's pair is one amplitude
#define QG_STORE_TILES(buf)                                                                  \
  {                                                                                          \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                          \
      const d2 a = arot[u] ? (d2){-av[u].y, av[u].x} : av[u];                                \
      const d2 b = brot[u] ? (d2){-bv[u].y, bv[u].x} : bv[u];                                \
      *reinterpret_cast<d2*>(As + (((buf) * QG_T + lrow + 32 * u) * syrk::PITCH + lk)) = a;  \
      *reinterpret_cast<d2*>(Bs + (((buf) * QG_T + lrow + 32 * u) * syrk::PITCH + lk)) = b;  \
    }                                                                                        \
  }
  const int fr = lane & 15, fk = lane >> 4;
  // D[row = fk + 4 r][col = fr] of MFMA tile (mi, ni): tile entry (wi * 64 + mi * 16 + fk + 4 r, wj * 64 + ni * 16 + fr)
  double* __restrict__ pt = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (QG_T * QG_T) +
                            (wi * 64 + fk) * QG_T + wj * 64 + fr;
#pragma unroll 1
  for (long long s = 0; s < per_wg; ++s) {
    const long long z0 = ((long long)blockIdx.y * per_wg + s) * slab;
    QG_LOAD_TILES(z0, 0)
    // (the previous slab's last k-step ended with a barrier: nobody reads the tiles any more)
    QG_STORE_TILES(0)
    __syncthreads();
    syrk::d4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (syrk::d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (long long kt = 0; kt < nk; ++kt) {
      const int cur = (int)(kt & 1);
      if (kt + 1 < nk) QG_LOAD_TILES(z0, (kt + 1) * syrk::BK)            // in flight during this k-step's MFMAs
      const double* __restrict__ Ac = As + (cur * QG_T + wi * 64 + fr) * syrk::PITCH + fk;
      const double* __restrict__ Bc = Bs + (cur * QG_T + wj * 64 + fr) * syrk::PITCH + fk;
      syrk::mfma_k_step<QG_MT>(Ac, Bc, acc);
      if (kt + 1 < nk) QG_STORE_TILES(cur ^ 1)
      __syncthreads();
    }
    // the workgroup's running total: its own partial tile (nobody else touches it; the same thread owns an entry
    // in every slab, so the additions are ordered by the program)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double* __restrict__ e = pt + (mi * 16 + 4 * r) * QG_T + ni * 16;
          *e = s == 0 ? acc[mi][ni][r] : *e + acc[mi][ni][r];
        }
  }
}

#undef QG_LOAD_TILES
#undef QG_STORE_TILES

// grid (tiles): Q_ab = Q_ba = (the G partials of entry (a <= b) in index order) - (re_a re_b + im_a im_b), re_a / im_a
// the sums of the entries (a, P) / (a, P + 1), which lie in the upper triangle too (a < P).
__global__ __launch_bounds__(syrk::THREADS) void qfi_finish_kernel(const double* __restrict__ part, int P, int T, int G,
                                                                   double* __restrict__ Q) {
  __shared__ double proj[2][2][QG_T];                                  // [side: rows of ti / of tj][re / im][row]
  int ti, tj;
  syrk::tile_pair(blockIdx.x, T, ti, tj);
  const long long stride = (long long)gridDim.x * (QG_T * QG_T);
  for (int e = threadIdx.x; e < 2 * 2 * QG_T; e += syrk::THREADS) {
    const int side = e / (2 * QG_T), c = (e / QG_T) & 1, row = e % QG_T;
    const int tr = side ? tj : ti, a = tr * QG_T + row, col = P + c;
    double sum = 0.0;                                                  // (the tile of (a, col) is in the triangle: col >= P > a)
    if (a < P) sum = syrk::sum_partials(part + syrk::tile_pair_index(tr, col / QG_T, T) * (QG_T * QG_T) + row * QG_T + col % QG_T, G, stride);
    proj[side][c][row] = sum;
  }
  __syncthreads();
  const double* __restrict__ pt = part + (long long)blockIdx.x * (QG_T * QG_T);
  for (int e = threadIdx.x; e < QG_T * QG_T; e += syrk::THREADS) {
    const int ra = e / QG_T, rb = e % QG_T;
    const int a = ti * QG_T + ra, b = tj * QG_T + rb;
    if (a >= P || b >= P || a > b) continue;
    const double q = syrk::sum_partials(pt + e, G, stride) - (proj[0][0][ra] * proj[1][0][rb] + proj[0][1][ra] * proj[1][1][rb]);
    Q[(long long)a * P + b] = q;
    Q[(long long)b * P + a] = q;
  }
}

LdsRaised qg_lds_raised;
}  // namespace

hipError_t launch_pi_shift_thetas(const double* theta, int P, int row0, int include_base, int p_begin, int bc, double* thetas,
                                  hipStream_t st) {
  const long long total = (long long)bc * P;
  if (total == 0) return hipSuccess;
  pi_shift_thetas_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(theta, P, row0, include_base, p_begin, bc, thetas);
  return hipGetLastError();
}

hipError_t launch_state_tail(const double* in, double* out, int n, int bc, const StateTail& T, hipStream_t st) {
  if (bc <= 0) return hipSuccess;
  const long long N = 1ll << n;
  state_tail_kernel<<<dim3((unsigned)((N + 255) / 256), (unsigned)bc), dim3(256), 0, st>>>(
      reinterpret_cast<const qs_d2*>(in), reinterpret_cast<qs_d2*>(out), n, T);
  return hipGetLastError();
}

size_t qfi_workspace_bytes(int n, int P) { return syrk::workspace_bytes(syrk::geom(2ll << n, P + 2, QG_T), QG_T); }

hipError_t launch_qfi_gram(int n, int P, const double* phi, const double* psi, double* Q, void* ws, hipStream_t st) {
  const syrk::Geom g = syrk::geom(2ll << n, P + 2, QG_T);             // a complex row: K = 2^(n+1) real columns
  const size_t lds = syrk::tiles_lds_bytes(QG_T);
  hipError_t e = raise_lds_once(reinterpret_cast<const void*>(qfi_gram_kernel), lds, qg_lds_raised);
  if (e != hipSuccess) return e;
  double* part = (double*)ws_align(ws);
  qfi_gram_kernel<<<dim3((unsigned)g.tiles, (unsigned)g.G), syrk::THREADS, lds, st>>>(phi, psi, 2ll << n, P, g.T, g.slab, g.per_wg, part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  qfi_finish_kernel<<<dim3((unsigned)g.tiles), syrk::THREADS, 0, st>>>(part, P, g.T, g.G, Q);
  return hipGetLastError();
}

}  // namespace bornvi
