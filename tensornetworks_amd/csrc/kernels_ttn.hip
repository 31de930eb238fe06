// Sampled Born machine on a binary tree tensor network (include/bornvi_ttn.h).
//
// Tree.  h = max(1, ceil(log2 n)), L = 2^h leaf positions, 1 <= n <= 63, so L <= 64.  Position j < n holds tuple position j:
//   z_{j+1}, bit n - 1 - j of the int64 outcome index, the real family's bit order.  Positions j >= n are padding and carry
//   the fixed value 0.  Nodes are heap-numbered v = 1 .. L - 1, their children are 2 v and 2 v + 1; nodes v >= L / 2 are
//   bottom nodes, their children are the positions 2 (v - L / 2) and 2 (v - L / 2) + 1.
// Parameter.  cores dev float64 [L - 1, D, D, D]: cores[v - 1] = T_v[p, a, b], p the parent bond, a, b the left and right
//   child bonds.  2 <= D <= 8, 1 <= B <= 2^24.  A leaf is the one-hot vector e_z in
//   R^D, so a bottom node is an ordinary node whose children are one-hot.
// Dead entries.  Never read, and their gradient is exactly 0.0: the root at p >= 1; a bottom node at a >= 2 or b >= 2; a
//   bottom node at the value 1 of a padding child.
// Amplitude.  x_v[p] = sum_{a,b} T_v[p, a, b] x_{2v}[a] x_{2v+1}[b], contracted as M = T x_{2v} over a, then M x_{2v+1} over b;
//   psi(z) = x_1[0];  Z = sum_z psi(z)^2;  q = psi^2 / Z.
// Environments.  Up densities: U_v = sum_{z in the subtree} x_v x_v^T (padding values are not summed over).  Down densities:
//   V_1 = e0 e0^T,  V_{2v}[a, a'] = sum V_v[p, p'] T[p, a, b] T[p', a', b'] U_{2v+1}[b, b'],  V_{2v+1} the same with U_{2v}.
//   Z = U_1[0, 0].  dZ/dT_v[p, a, b] = 2 sum V_v[p, p'] T_v[p', a', b'] U_{2v}[a, a'] U_{2v+1}[b, b'].
// Per-sample down vectors.  y_1 = e0,  y_{2v}[a] = sum y_v[p] T[p, a, b] x_{2v+1}[b],  y_{2v+1}[b] = sum y_v[p] T[p, a, b] x_{2v}[a].
// Gradient of sum_b w_b log q(z_b).  Block v receives sum_b (2 w_b / psi_b) y_{b,v} (x) x_{b,2v} (x) x_{b,2v+1} and loses
//   (sum_b w_b) dZ/dT_v / Z.
// Rescaling.  Every vector and density is multiplied after every step by 2^-e, e the ilogb of its largest magnitude (exact; 0
//   when that is 0 or not finite), and the running sum of the e's is carried beside it, as in section 6g; a node's exponent
//   is its own plus its children's.
// Sampler.  Depth first, positions left to right, exact.  Node v has the density P_v of everything outside its subtree (drawn
//   positions as pure vectors, undrawn ones traced), P_1 = e0 e0^T.  At a node:
//   P_{2v}[a, a'] = sum P_v[p, p'] T[p, a, b] T[p', a', b'] U_{2v+1}[b, b'];  descend left, which returns x_{2v};  M = T x_{2v},
//   P_{2v+1} = M^T P_v M;  descend right;  return x_v = M x_{2v+1}.  A position with density P has the masses m_0 = P[0, 0],
//   m_1 = P[1, 1] and draws z = [U (m_0 + m_1) >= m_0]; a padding position draws nothing and is 0.  U for position j is
//   bornvi_mps_sample's Philox4x32-10 uniform at (seed, epoch, b, k = j + 1).
//
// ttn_env_kernel: ONE workgroup of 256 threads walks the levels, bottom level first for U, then top level first for V; the
//   work is at most 63 nodes of a few D^4 products, so it is launch latency and a launch per level would pay it h times
//   over.  The nodes of a level are independent: the threads take (node, entry) pairs of the whole level, and every
//   intermediate lives in the workspace (a level of D = 8 does not fit LDS), published by the workgroup's barriers.  Per
//   node, each entry one fma chain in index order:
//     A_v[p, a', b] = sum_a T[p, a, b] U^_{2v}[a, a'],   R_v[p, a, b'] = sum_b T[p, a, b] U^_{2v+1}[b, b']   (the sampler's T U)
//     W_v[p, a', b'] = sum_b A_v[p, a', b] U^_{2v+1}[b, b'],   U_v[p, p'] = sum_{a', b'} W_v[p, a', b'] T[p', a', b'] (a' outer)
//     Y[p', a, b'] = sum_p V^_v[p, p'] R_v[p, a, b'],   V_{2v}[a, a'] = sum_{p', b'} Y[p', a, b'] T[p', a', b'] (p' outer)
//     Y'[p', a', b] = sum_p V^_v[p, p'] A_v[p, a', b],  V_{2v+1}[b, b'] = sum_{p', a'} Y'[p', a', b] T[p', a', b'] (p' outer)
//   each density then times 2^-e.  A leaf's U is diag(1, 1, 0, ..) and a padding leaf's diag(1, 0, ..), exponent 0.
// ttn_sample_kernel<DP>: one sample per lane, one wave per workgroup, at most G workgroups walking the tiles wg, wg + G, ...
//   The depth-first walk is a loop over (node, phase), the same for every lane: phase 0 enters a node and makes P_{2v}, phase 1
//   comes back from the left child and makes P_{2v+1}, phase 2 comes back from the right child and makes x_v (ttn_node_up).
//   The stack holds per level the density P_v (DP^2 doubles a sample), the left child's vector and its exponent: in LDS for
//   DP <= 4 (49 + 12 KiB), in the workgroup's slice of the workspace for DP = 8 ([level][entry][lane], 216 KiB).  T_v and
//   R_v are shared through LDS.  The two D^4 contractions of P_{2v} run row by row:  for a:  Y[p', b'] = sum_p P[p, p'] R[p, a, b']
//   (P and Y in registers, 2 DP^2 doubles), then P'[a, a'] = sum_{p', b'} Y[p', b'] T[p', a', b'] for every a' (p' outer).  A
//   bottom node makes the rows a = 0, 1 only and keeps m_0 = P'[0, 0], m_1 = P'[1, 1] in registers.  P_{2v+1}:  M in registers,
//   for p':  N[b] = sum_p P[p, p'] M[p, b],  P'[b, b'] += N[b] M[p', b'].  The densities' own exponents are dropped: the
//   draw is homogeneous in P.
// ttn_score_kernel<DP>: the same tiling.  Up sweep v = L - 1 .. 1 (ttn_node_up), x^_v and its exponent into the slice
//   [node][entry][lane]; logq; with a gradient the down sweep v = 1 .. L - 1:  N[a][b] = sum_p y[p] T[p, a, b],
//   y_{2v}[a] = sum_b N[a][b] x_{2v+1}[b],  y_{2v+1}[b] = sum_a N[a][b] x_{2v}[a], into the slice too.  The sample term of node v is
//   the product [c_b y_{b,v}[p]] (16 x 64, p zero-padded) times [x_{b,2v}[a] x_{b,2v+1}[b']] (64 x DP^2) on v_mfma_f64_16x16x4_f64:
//   the lanes' vectors are transposed through LDS (pitch 68: the 16 rows of a K-step fall on distinct banks), lane l feeds
//   A[p = l & 15][sample 4 kk + (l >> 4)] and B[sample][pair 16 t + (l & 15)], 16 K-steps per N tile t of 16 pairs, and the
//   accumulator tile (register j: p = 4 j + (l >> 4)) starts from the workgroup's own partial [L - 1, D, D, D] (0.0 in its
//   first tile) and goes back to it: one chain over the workgroup's samples in sample order.
//   c_b = (2 w_b / x^_1[0]) 2^(ey_v + ex_2v + ex_2v+1 - ex_1), 0 where the sample does not count.
// ttn_score_finish_kernel, one workgroup per node: the partials in workgroup order, sum_b w_b, and the environment term
//   2 sum_p' V^_v[p, p'] W_v[p', a, b] 2^(eV_v + eU_2v + eU_2v+1 - eU_1) / U^_1[0, 0]; exactly 0.0 into every dead entry.
//
// No atomics, no allocation, no synchronisation: capturable, and two calls are bitwise equal.  The status word is cleared by
// the one-lane kernel of kernels_mps_sample.hip in front of the launch and set by plain stores.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bornvi_ttn.h"
#include "kernels.hpp"
#include "ttn_dev.hpp"

namespace bornvi {

namespace {
constexpr int TT_DMAX = BORNVI_TTN_MAX_BOND;
constexpr int TT_PITCH = 68;               // row pitch of the transposed operands in the score kernel's LDS
static_assert(TT_DMAX == 8, "the kernels are instantiated for DP = 2, 4, 8");

struct TtLayout {
  int h, L, DP, G;
  size_t slice, islice;                                        // doubles / ints of a workgroup's slice
  size_t hdr, U, V, eU, eV, A, R, W, Yl, Yr, raw, slices, islices, parts, wpart, total;   // byte offsets from the aligned base
};

TtLayout tt_layout(int n, int D, long long B) {
  TtLayout S;
  S.h = ttn_height(n);
  S.L = 1 << S.h;
  S.DP = bond_dp(D);
  const long long tiles = (B + TT_LANES - 1) / TT_LANES;
  S.G = (int)(tiles < BORNVI_TTN_MAX_WG ? tiles : BORNVI_TTN_MAX_WG);
  const size_t L = S.L, DD = (size_t)D * D, D3 = DD * D, DP = S.DP;
  const size_t stack = DP > 4 ? (size_t)TT_MAX_H * (DP * DP + DP) * TT_LANES : 0;      // the sampler's, where LDS does not hold it
  const size_t xy = 2 * L * DP * TT_LANES;                                             // the score call's x^_v and y^_v
  S.slice = stack > xy ? stack : xy;
  S.islice = 2 * L * TT_LANES;
  size_t o = 0;
  S.hdr = o;     o += 256;
  S.U = o;       o += ws_round(2 * L * DD * sizeof(double));      // heap index u < 2 L: nodes, then leaves
  S.V = o;       o += ws_round(2 * L * DD * sizeof(double));
  S.eU = o;      o += ws_round(2 * L * sizeof(int));
  S.eV = o;      o += ws_round(2 * L * sizeof(int));
  S.A = o;       o += ws_round(L * D3 * sizeof(double));
  S.R = o;       o += ws_round(L * D3 * sizeof(double));
  S.W = o;       o += ws_round(L * D3 * sizeof(double));
  S.Yl = o;      o += ws_round(L * D3 * sizeof(double));
  S.Yr = o;      o += ws_round(L * D3 * sizeof(double));
  S.raw = o;     o += ws_round(2 * L * DD * sizeof(double));
  S.slices = o;  o += ws_round((size_t)S.G * S.slice * sizeof(double));
  S.islices = o; o += ws_round((size_t)S.G * S.islice * sizeof(int));
  S.parts = o;   o += ws_round((size_t)S.G * (L - 1) * D3 * sizeof(double));
  S.wpart = o;   o += ws_round((size_t)BORNVI_TTN_MAX_WG * sizeof(double));
  S.total = o;
  return S;
}

// ---- environments ----------------------------------------------------------------------------------------------
struct TtEnv {
  double *U, *V, *A, *R, *W, *Yl, *Yr, *raw, *hdr;
  int *eU, *eV;
};

// X[u] <- raw[u] 2^-e for the `cnt` matrices from heap index `first`, e into own[] (every thread of a matrix finds the same e)
__device__ __forceinline__ void tt_env_rescale(int first, int cnt, int DD, const double* raw, double* X, int* own) {
  for (int i = threadIdx.x; i < cnt * DD; i += MS_ENV_THREADS) {
    const int u = first + i / DD, r = i % DD;
    double mx = 0.0;
    for (int k = 0; k < DD; ++k) mx = fmax(mx, fabs(raw[u * DD + k]));
    const int e = ms_exponent(mx);
    X[u * DD + r] = ldexp(raw[u * DD + r], -e);
    if (r == 0) own[u] = e;
  }
}

__global__ __launch_bounds__(MS_ENV_THREADS) void ttn_env_kernel(const double* __restrict__ cores, int n, int D, int h, TtEnv E,
                                                               double* __restrict__ logZ_out) {
  __shared__ int own[2 * (1 << TT_MAX_H)];
  const int L = 1 << h, DD = D * D, D3 = DD * D, t = threadIdx.x;
  for (int i = t; i < L * DD; i += MS_ENV_THREADS) {          // the leaves: diag over the allowed values
    const int j = i / DD, a = (i % DD) / D, b = i % D;
    E.U[(L + j) * DD + i % DD] = (a == b && (a == 0 || (a == 1 && j < n))) ? 1.0 : 0.0;
  }
  for (int i = t; i < L; i += MS_ENV_THREADS) E.eU[L + i] = 0;
  __syncthreads();
  for (int lev = h - 1; lev >= 0; --lev) {
    const int first = 1 << lev, cnt = 1 << lev;
    for (int i = t; i < cnt * D3; i += MS_ENV_THREADS) {
      const int v = first + i / D3, r = i % D3, p = r / DD, q = (r / D) % D, s = r % D;
      const double *Ul = E.U + 2 * v * DD, *Ur = Ul + DD;
      double al = 0.0, ar = 0.0;
      for (int c = 0; c < D; ++c) {
        al = fma(ttn_core(cores, v, p, c, s, D, L, n), Ul[c * D + q], al);      // A[p, a' = q, b = s]
        ar = fma(ttn_core(cores, v, p, q, c, D, L, n), Ur[c * D + s], ar);      // R[p, a = q, b' = s]
      }
      E.A[v * D3 + r] = al;
      E.R[v * D3 + r] = ar;
    }
    __syncthreads();
    for (int i = t; i < cnt * D3; i += MS_ENV_THREADS) {
      const int v = first + i / D3, r = i % D3, pq = r / D, s = r % D;
      const double* Ur = E.U + (2 * v + 1) * DD;
      double acc = 0.0;
      for (int c = 0; c < D; ++c) acc = fma(E.A[v * D3 + pq * D + c], Ur[c * D + s], acc);
      E.W[v * D3 + r] = acc;
    }
    __syncthreads();
    for (int i = t; i < cnt * DD; i += MS_ENV_THREADS) {
      const int v = first + i / DD, p = (i % DD) / D, pp = i % D;
      double acc = 0.0;
      for (int a = 0; a < D; ++a)
        for (int b = 0; b < D; ++b) acc = fma(E.W[v * D3 + (p * D + a) * D + b], ttn_core(cores, v, pp, a, b, D, L, n), acc);
      E.raw[v * DD + i % DD] = acc;
    }
    __syncthreads();
    tt_env_rescale(first, cnt, DD, E.raw, E.U, own);
    __syncthreads();
    for (int i = t; i < cnt; i += MS_ENV_THREADS) {
      const int v = first + i;
      E.eU[v] = own[v] + E.eU[2 * v] + E.eU[2 * v + 1];
    }
    __syncthreads();
  }
  for (int i = t; i < DD; i += MS_ENV_THREADS) E.V[DD + i] = i == 0 ? 1.0 : 0.0;
  if (t == 0) E.eV[1] = 0;
  __syncthreads();
  for (int lev = 0; lev < h - 1; ++lev) {
    const int first = 1 << lev, cnt = 1 << lev;
    for (int i = t; i < cnt * D3; i += MS_ENV_THREADS) {
      const int v = first + i / D3, r = i % D3, pp = r / DD, rest = r % DD;
      double yl = 0.0, yr = 0.0;
      for (int p = 0; p < D; ++p) {
        const double vv = E.V[v * DD + p * D + pp];
        yl = fma(vv, E.R[v * D3 + p * DD + rest], yl);      // Y[p', a, b']
        yr = fma(vv, E.A[v * D3 + p * DD + rest], yr);      // Y'[p', a', b]
      }
      E.Yl[v * D3 + r] = yl;
      E.Yr[v * D3 + r] = yr;
    }
    __syncthreads();
    for (int i = t; i < cnt * 2 * DD; i += MS_ENV_THREADS) {
      const int v = first + i / (2 * DD), right = (i / DD) & 1, x = (i % DD) / D, xp = i % D;
      double acc = 0.0;
      for (int pp = 0; pp < D; ++pp)
        for (int c = 0; c < D; ++c)
          acc = right ? fma(E.Yr[v * D3 + (pp * D + c) * D + x], ttn_core(cores, v, pp, c, xp, D, L, n), acc)      // sum_{p', a'}
                      : fma(E.Yl[v * D3 + (pp * D + x) * D + c], ttn_core(cores, v, pp, xp, c, D, L, n), acc);     // sum_{p', b'}
      E.raw[(2 * v + right) * DD + i % DD] = acc;
    }
    __syncthreads();
    tt_env_rescale(2 * first, 2 * cnt, DD, E.raw, E.V, own);
    __syncthreads();
    for (int i = t; i < 2 * cnt; i += MS_ENV_THREADS) {
      const int c = 2 * first + i;
      E.eV[c] = own[c] + E.eV[c >> 1] + E.eU[c ^ 1];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double Zh = E.U[DD];
    const double lz = log(Zh) + (double)E.eU[1] * MS_LN2;
    E.hdr[0] = lz;
    E.hdr[1] = Zh;
    E.hdr[2] = (double)E.eU[1];
    if (logZ_out) logZ_out[0] = lz;
  }
}

// ---- sampler ---------------------------------------------------------------------------------------------------
// rows a < na of P'[a, a'] = sum P[p, p'] R[p, a, b'] T[p', a', b'] from the slot Pv.  STORE: into the slot Pn, times 2^-e;
// else (a bottom node) only m0 = P'[0, 0] and m1 = P'[1, 1] are kept.  STAGE (the stack is in the workspace): P_v goes through
// the lane's column of Wl first, so that every turn of a reads it from LDS and not from registers or global memory.
template <int DP, bool STORE, bool STAGE>
__device__ __forceinline__ void tt_density_left(const double* Pv, const double* Ts, const double* Rs, double* Wl, int lane, int na,
                                                double* Pn, double& m0, double& m1) {
  const double* Ps = Pv;
  if (STAGE) {
#pragma unroll 8
    for (int i = 0; i < DP * DP; ++i) Wl[i * TT_LANES + lane] = Pv[i * TT_LANES + lane];
    Ps = Wl;
  }
  double mx = 0.0;
#pragma unroll 1
  for (int a = 0; a < na; ++a) {
    asm volatile("" ::: "memory");      // P_v, T_v and R_v are read from LDS in every turn, not kept in registers across them
    double Y[DP][DP];
#pragma unroll
    for (int pp = 0; pp < DP; ++pp)
#pragma unroll
      for (int bp = 0; bp < DP; ++bp) Y[pp][bp] = 0.0;
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      double Pr[DP];
#pragma unroll
      for (int pp = 0; pp < DP; ++pp) Pr[pp] = Ps[(p * DP + pp) * TT_LANES + lane];
#pragma unroll
      for (int bp = 0; bp < DP; ++bp) {
        const double r = Rs[(p * DP + a) * DP + bp];
#pragma unroll
        for (int pp = 0; pp < DP; ++pp) Y[pp][bp] = fma(Pr[pp], r, Y[pp][bp]);
      }
    }
#pragma unroll
    for (int ap = 0; ap < DP; ++ap) {
      if (!STORE && ap >= 2) continue;      // a bottom node keeps P'[0, 0] and P'[1, 1] only
      double acc = 0.0;
#pragma unroll
      for (int pp = 0; pp < DP; ++pp)
#pragma unroll
        for (int bp = 0; bp < DP; ++bp) acc = fma(Y[pp][bp], Ts[(pp * DP + ap) * DP + bp], acc);
      if (STORE) {
        Pn[(a * DP + ap) * TT_LANES + lane] = acc;
        mx = fmax(mx, fabs(acc));
      } else {
        if (ap == 0) m0 = a == 0 ? acc : m0;
        if (ap == 1) m1 = a == 1 ? acc : m1;
      }
    }
  }
  if (STORE) {
    const int e = ms_exponent(mx);
#pragma unroll 8
    for (int i = 0; i < DP * DP; ++i) Pn[i * TT_LANES + lane] = ldexp(Pn[i * TT_LANES + lane], -e);
  }
}

// P' = M^T P M, M[p][b] = sum_a T[p, a, b] x[a].  STAGE: M lives in the lane's column of Wl and the loop over p' is rolled; else M is
// in registers.
template <int DP, bool STORE, bool STAGE>
__device__ __forceinline__ void tt_density_right(const double* Pv, const double* Ts, const double (&x)[DP], double* Wl, int lane,
                                                 double* Pn, double& m0, double& m1) {
  double Mr[STAGE ? 1 : DP][STAGE ? 1 : DP], Q[DP][DP];
#pragma unroll
  for (int p = 0; p < DP; ++p)
#pragma unroll
    for (int b = 0; b < DP; ++b) {
      double m = 0.0;
#pragma unroll
      for (int a = 0; a < DP; ++a) m = fma(Ts[(p * DP + a) * DP + b], x[a], m);
      if constexpr (STAGE) Wl[(p * DP + b) * TT_LANES + lane] = m;
      else Mr[p][b] = m;
      Q[p][b] = 0.0;
    }
  constexpr int UNROLL_PP = STAGE ? 1 : DP;
#pragma unroll UNROLL_PP
  for (int pp = 0; pp < DP; ++pp) {
    if (STAGE) asm volatile("" ::: "memory");
    double N[DP];
#pragma unroll
    for (int b = 0; b < DP; ++b) N[b] = 0.0;
#pragma unroll
    for (int p = 0; p < DP; ++p) {
      const double pv = Pv[(p * DP + pp) * TT_LANES + lane];
#pragma unroll
      for (int b = 0; b < DP; ++b) {
        double m;
        if constexpr (STAGE) m = Wl[(p * DP + b) * TT_LANES + lane];
        else m = Mr[p][b];
        N[b] = fma(pv, m, N[b]);
      }
    }
#pragma unroll
    for (int bp = 0; bp < DP; ++bp) {
      double m;
      if constexpr (STAGE) m = Wl[(pp * DP + bp) * TT_LANES + lane];
      else m = Mr[pp][bp];
#pragma unroll
      for (int b = 0; b < DP; ++b) Q[b][bp] = fma(N[b], m, Q[b][bp]);
    }
  }
  if (STORE) {
    double mx = 0.0;
#pragma unroll
    for (int b = 0; b < DP; ++b)
#pragma unroll
      for (int bp = 0; bp < DP; ++bp) mx = fmax(mx, fabs(Q[b][bp]));
    const int e = ms_exponent(mx);
#pragma unroll
    for (int b = 0; b < DP; ++b)
#pragma unroll
      for (int bp = 0; bp < DP; ++bp) Pn[(b * DP + bp) * TT_LANES + lane] = ldexp(Q[b][bp], -e);
  } else {
    m0 = Q[0][0];
    m1 = Q[1][1];
  }
}

// the draw of position j from its masses (a padding position draws nothing and is 0): the real sampler's rule and uniforms
__device__ __forceinline__ bool tt_draw(int j, int n, long long b, uint32_t ep, uint32_t seed_lo, uint32_t seed_hi, double m0, double m1,
                                        bool active, double& Unext, bool& dead, unsigned long long& z, int* status) {
  if (j >= n) return false;
  const int k = j + 1;
  double U = Unext;
  if (k & 1) {
    const uint4 w = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)((k + 1) / 2 - 1), MS_PHILOX_DOMAIN, ep), seed_lo, seed_hi);
    U = unit53(w.x, w.y);
    Unext = unit53(w.z, w.w);
  }
  const double tot = m0 + m1;
  if (!dead && !(tot > 0.0 && isfinite(tot))) {
    dead = true;
    if (active) *status = 1;
  }
  const bool bit = !dead && (U * tot >= m0);
  z |= (bit ? 1ull : 0ull) << (n - 1 - j);
  return bit;
}

template <int DP>
__global__ __launch_bounds__(TT_LANES) void ttn_sample_kernel(const double* __restrict__ cores, int n, int D, int h, long long B,
                                                              long long ntiles, const double* __restrict__ Renv,
                                                              const double* __restrict__ hdr, uint32_t seed_lo, uint32_t seed_hi,
                                                              const long long* __restrict__ epoch_dev, long long* __restrict__ idx,
                                                              double* __restrict__ logq, int* status, double* slices,
                                                              size_t slice) {
  constexpr int DD = DP * DP, D3 = DD * DP;
  constexpr bool IN_LDS = DP <= 4;
  __shared__ double Ts[D3], Rs[D3];
  __shared__ double Pl[IN_LDS ? TT_MAX_H * DD * TT_LANES : 1];
  __shared__ double Xl[IN_LDS ? TT_MAX_H * DP * TT_LANES : 1];
  __shared__ int El[TT_MAX_H * TT_LANES];
  __shared__ double Wl[IN_LDS ? 1 : DD * TT_LANES];                     // a lane's matrix in flight, where the stack is not in LDS
  double* Pst = IN_LDS ? Pl : slices + (size_t)blockIdx.x * slice;      // [level][DD][lane]
  double* Xst = IN_LDS ? Xl : Pst + TT_MAX_H * DD * TT_LANES;           // [level][DP][lane]
  const int lane = threadIdx.x, L = 1 << h, Dc = D * D * D;
  const uint32_t ep = (uint32_t)(unsigned long long)(*epoch_dev);
  const double Zh = hdr[1], eU1 = hdr[2];
#pragma unroll 1
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long b = tile * TT_LANES + lane;
    const bool active = b < B;
#pragma unroll 1
    for (int i = 0; i < DD; ++i) Pst[i * TT_LANES + lane] = i == 0 ? 1.0 : 0.0;
    unsigned long long z = 0;
    bool dead = false;
    double Unext = 0.0;             // the second uniform of a Philox call, for the next (even) k
    double xc[DP];                  // the vector the last finished subtree returned, and its exponent
    ms_fill<DP>(xc, 1.0);
    int ec = 0;
    int v = 1, lev = 0, phase = 0;
#pragma unroll 1
    while (true) {
      const bool bottom = 2 * v >= L;
      double* Pv = Pst + (size_t)lev * DD * TT_LANES;
      __syncthreads();
      ttn_load_node<DP>(cores, v, D, L, n, Ts, phase == 0 ? Renv + (size_t)v * Dc : nullptr, Rs);
      __syncthreads();
      if (phase == 0) {
        double m0 = 0.0, m1 = 0.0;
        if (bottom) {
          tt_density_left<DP, false, !IN_LDS>(Pv, Ts, Rs, Wl, lane, 2, nullptr, m0, m1);
          const bool bit = tt_draw(2 * v - L, n, b, ep, seed_lo, seed_hi, m0, m1, active, Unext, dead, z, status);
          ttn_leaf_bit<DP>(xc, bit);
          ec = 0;
          phase = 1;
        } else {
          tt_density_left<DP, true, !IN_LDS>(Pv, Ts, Rs, Wl, lane, DP, Pv + DD * TT_LANES, m0, m1);
          v = 2 * v;
          ++lev;
        }
      } else if (phase == 1) {
        ttn_slot_store<DP>(Xst + (size_t)lev * DP * TT_LANES, lane, xc);
        El[lev * TT_LANES + lane] = ec;
        double m0 = 0.0, m1 = 0.0;
        if (bottom) {
          tt_density_right<DP, false, !IN_LDS>(Pv, Ts, xc, Wl, lane, nullptr, m0, m1);
          const bool bit = tt_draw(2 * v - L + 1, n, b, ep, seed_lo, seed_hi, m0, m1, active, Unext, dead, z, status);
          ttn_leaf_bit<DP>(xc, bit);
          ec = 0;
          phase = 2;
        } else {
          tt_density_right<DP, true, !IN_LDS>(Pv, Ts, xc, Wl, lane, Pv + DD * TT_LANES, m0, m1);
          v = 2 * v + 1;
          ++lev;
          phase = 0;
        }
      } else {
        double xl[DP], xn[DP];
        ttn_slot_load<DP>(Xst + (size_t)lev * DP * TT_LANES, lane, xl);
        const int e = ttn_node_up<DP>(Ts, xl, xc, xn);
        ec = e + El[lev * TT_LANES + lane] + ec;
#pragma unroll
        for (int a = 0; a < DP; ++a) xc[a] = xn[a];
        if (v == 1) break;
        phase = (v & 1) ? 2 : 1;
        v >>= 1;
        --lev;
      }
    }
    if (active) {
      idx[b] = (long long)z;
      logq[b] = dead ? NAN : ms_logq(xc[0], ec, Zh, eU1);
    }
  }
}

// ---- score -----------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(TT_LANES) void ttn_score_kernel(const double* __restrict__ cores, int n, int D, int h, long long B,
                                                             long long ntiles, const long long* __restrict__ idx,
                                                             const double* __restrict__ wgt, const double* __restrict__ hdr,
                                                             double* __restrict__ logq, int* status, double* slices, size_t slice,
                                                             int* islices, size_t islice, double* parts,
                                                             double* __restrict__ wpart, int want_grad) {
  constexpr int DD = DP * DP, D3 = DD * DP, NT = DD < 16 ? 1 : DD / 16;
  __shared__ double Ts[D3];
  __shared__ double Ay[16 * TT_PITCH], Xa[DP * TT_PITCH], Xb[DP * TT_PITCH];
  const int lane = threadIdx.x, L = 1 << h, fr = lane & 15, fk = lane >> 4, Dc = D * D * D;
  double* X = slices + (size_t)blockIdx.x * slice;          // x^_v: [node][DP][lane]
  double* Y = X + (size_t)L * DP * TT_LANES;                // y^_v
  int* eX = islices + (size_t)blockIdx.x * islice;          // [node][lane]
  int* eY = eX + L * TT_LANES;
  double* part = parts + (size_t)blockIdx.x * (L - 1) * Dc;
  const double Zh = hdr[1], eU1 = hdr[2];
  const bool Zok = ms_norm_ok(Zh);
  for (int i = lane; i < 16 * TT_PITCH; i += TT_LANES) Ay[i] = 0.0;      // rows p >= DP stay 0
  double wacc = 0.0;
  bool first = true;
#pragma unroll 1
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x, first = false) {
    const long long b = tile * TT_LANES + lane;
    const bool active = b < B;
    const unsigned long long z = active ? (unsigned long long)idx[b] : 0ull;
    const double w = (active && want_grad) ? wgt[b] : 0.0;
    wacc += w;
    // a child's vector and exponent: a position's one-hot vector, or x^ of the node below
    auto child = [&](int c, double (&x)[DP]) -> int {
      if (c >= L) {
        ttn_leaf<DP>(x, z, c - L, n);
        return 0;
      }
      ttn_slot_load<DP>(X + (size_t)c * DP * TT_LANES, lane, x);
      return eX[c * TT_LANES + lane];
    };
    double x1[DP];
    int ex1 = 0;
#pragma unroll 1
    for (int v = L - 1; v >= 1; --v) {
      __syncthreads();
      ttn_load_node<DP>(cores, v, D, L, n, Ts, nullptr, nullptr);
      __syncthreads();
      double xl[DP], xr[DP];
      const int el = child(2 * v, xl), er = child(2 * v + 1, xr);
      ex1 = ttn_node_up<DP>(Ts, xl, xr, x1) + el + er;
      ttn_slot_store<DP>(X + (size_t)v * DP * TT_LANES, lane, x1);
      eX[v * TT_LANES + lane] = ex1;
    }
    const double a0 = x1[0];
    const bool good = active && ms_amplitude_ok(a0, Zok);
    if (active) {
      logq[b] = ms_logq(a0, ex1, Zh, eU1);
      if (!good) *status = 2;
    }
    if (!want_grad) continue;
    const double g = good ? (w + w) / a0 : 0.0;
#pragma unroll 1
    for (int v = 1; v < L; ++v) {
      __syncthreads();
      ttn_load_node<DP>(cores, v, D, L, n, Ts, nullptr, nullptr);
      double y[DP], xl[DP], xr[DP];
      int ey = 0;
      if (v == 1) ms_fill<DP>(y, 1.0);
      else {
        ttn_slot_load<DP>(Y + (size_t)v * DP * TT_LANES, lane, y);
        ey = eY[v * TT_LANES + lane];
      }
      const int el = child(2 * v, xl), er = child(2 * v + 1, xr);
      const double c = ms_site_factor(g, ey, el + er, ex1);
#pragma unroll
      for (int p = 0; p < DP; ++p) Ay[p * TT_PITCH + lane] = good ? c * y[p] : 0.0;
#pragma unroll
      for (int a = 0; a < DP; ++a) {
        Xa[a * TT_PITCH + lane] = xl[a];
        Xb[a * TT_PITCH + lane] = xr[a];
      }
      __syncthreads();
      if (2 * v < L) {          // the children's down vectors
        double yl[DP], yr[DP];
#pragma unroll
        for (int a = 0; a < DP; ++a) yl[a] = 0.0;
#pragma unroll
        for (int bb = 0; bb < DP; ++bb) yr[bb] = 0.0;
#pragma unroll
        for (int a = 0; a < DP; ++a)
#pragma unroll
          for (int bb = 0; bb < DP; ++bb) {
            double nn = 0.0;
#pragma unroll
            for (int p = 0; p < DP; ++p) nn = fma(y[p], Ts[(p * DP + a) * DP + bb], nn);
            yl[a] = fma(nn, xr[bb], yl[a]);
            yr[bb] = fma(nn, xl[a], yr[bb]);
          }
        const int e0 = ms_rescale<DP>(yl), e1 = ms_rescale<DP>(yr);
        ttn_slot_store<DP>(Y + (size_t)(2 * v) * DP * TT_LANES, lane, yl);
        ttn_slot_store<DP>(Y + (size_t)(2 * v + 1) * DP * TT_LANES, lane, yr);
        eY[(2 * v) * TT_LANES + lane] = e0 + ey + er;
        eY[(2 * v + 1) * TT_LANES + lane] = e1 + ey + el;
      }
      // the sample term on the matrix cores: accumulator register j of tile t is entry p = 4 j + fk, pair 16 t + fr
      double* pv = part + (size_t)(v - 1) * Dc;
      typedef double d4 __attribute__((ext_vector_type(4)));
      d4 acc[NT];
      int off[NT];
      bool ok[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int pair = 16 * t + fr, a = pair / DP, bb = pair % DP;
        ok[t] = pair < DD && a < D && bb < D;
        off[t] = a * D + bb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = 4 * j + fk;
          acc[t][j] = (!first && ok[t] && p < D) ? pv[p * D * D + off[t]] : 0.0;
        }
      }
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const int s = 4 * kk + fk;
        const double av = Ay[fr * TT_PITCH + s];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int pair = 16 * t + fr, a = pair / DP, bb = pair % DP;
          const double bv = pair < DD ? Xa[a * TT_PITCH + s] * Xb[bb * TT_PITCH + s] : 0.0;
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = 4 * j + fk;
          if (ok[t] && p < D) pv[p * D * D + off[t]] = acc[t][j];
        }
    }
  }
  const double wtot = wave_sum(wacc);
  if (want_grad && lane == 0) wpart[blockIdx.x] = wtot;
}

// grid L - 1: grad[v - 1] = the workgroups' partials in order - (sum_b w_b) dZ/dT_v / Z; 0.0 into the dead entries
__global__ __launch_bounds__(MS_ENV_THREADS) void ttn_score_finish_kernel(int n, int D, int h, int G, const double* __restrict__ parts,
                                                                        const double* __restrict__ wpart, TtEnv E,
                                                                        double* __restrict__ grad) {
  __shared__ double red[MS_ENV_THREADS / 64];
  const int v = blockIdx.x + 1, t = threadIdx.x, L = 1 << h, DD = D * D, D3 = DD * D;
  const double W = sum_partials<MS_ENV_THREADS>(wpart, G, red);
  const int ex = E.eV[v] + E.eU[2 * v] + E.eU[2 * v + 1] - E.eU[1];
  const double Zh = E.hdr[1];
  const size_t stride = (size_t)(L - 1) * D3;
  for (int i = t; i < D3; i += MS_ENV_THREADS) {
    const int p = i / DD, ab = i % DD;
    double out = 0.0;
    if (ttn_live(v, p, ab / D, ab % D, L, n)) {
      double m = 0.0;
      for (int pp = 0; pp < D; ++pp) m = fma(E.V[v * DD + p * D + pp], E.W[v * D3 + pp * DD + ab], m);
      const double env = ldexp(m / Zh, ex);
      double sum = 0.0;
      const double* q = parts + (size_t)(v - 1) * D3 + i;
      for (int g = 0; g < G; ++g) sum += q[g * stride];
      out = sum - W * (env + env);
    }
    grad[(size_t)(v - 1) * D3 + i] = out;
  }
}

TtEnv tt_env(const TtLayout& S, char* base) {
  TtEnv E;
  E.U = (double*)(base + S.U);
  E.V = (double*)(base + S.V);
  E.A = (double*)(base + S.A);
  E.R = (double*)(base + S.R);
  E.W = (double*)(base + S.W);
  E.Yl = (double*)(base + S.Yl);
  E.Yr = (double*)(base + S.Yr);
  E.raw = (double*)(base + S.raw);
  E.hdr = (double*)(base + S.hdr);
  E.eU = (int*)(base + S.eU);
  E.eV = (int*)(base + S.eV);
  return E;
}

}  // namespace

size_t ttn_workspace_bytes(int n, int D, long long B) { return tt_layout(n, D, B).total + 256; }

hipError_t launch_ttn_environments(int n, int D, long long B, const double* cores, double* logZ_out, void* ws, hipStream_t st) {
  const TtLayout S = tt_layout(n, D, B);
  ttn_env_kernel<<<1, MS_ENV_THREADS, 0, st>>>(cores, n, D, S.h, tt_env(S, ws_align(ws)), logZ_out);
  return hipGetLastError();
}

hipError_t launch_ttn_sample(int n, int D, long long B, const double* cores, unsigned long long seed, const long long* epoch_dev,
                             long long* idx, double* logq, int* status, void* ws, hipStream_t st) {
  const TtLayout S = tt_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const long long ntiles = (B + TT_LANES - 1) / TT_LANES;
  switch (S.DP) {
#define TTN_SAMPLE_CASE(DPV)                                                                                                        \
  case DPV:                                                                                                                         \
    ttn_sample_kernel<DPV><<<(unsigned)S.G, TT_LANES, 0, st>>>(cores, n, D, S.h, B, ntiles, (const double*)(base + S.R),            \
                                                               (const double*)(base + S.hdr), (uint32_t)seed, (uint32_t)(seed >> 32), \
                                                               epoch_dev, idx, logq, status, (double*)(base + S.slices), S.slice);  \
    break;
    TTN_SAMPLE_CASE(2)
    TTN_SAMPLE_CASE(4)
    default:
      TTN_SAMPLE_CASE(8)
#undef TTN_SAMPLE_CASE
  }
  return hipGetLastError();
}

hipError_t launch_ttn_score_vjp(int n, int D, long long B, const double* cores, const long long* idx, const double* w, double* logq,
                                double* grad_cores, int* status, void* ws, hipStream_t st) {
  const TtLayout S = tt_layout(n, D, B);
  char* base = ws_align(ws);
  hipError_t e = launch_ms_clear_status(status, st);
  if (e != hipSuccess) return e;
  const long long ntiles = (B + TT_LANES - 1) / TT_LANES;
  const int want = grad_cores != nullptr;
  switch (S.DP) {
#define TTN_SCORE_CASE(DPV)                                                                                                         \
  case DPV:                                                                                                                         \
    ttn_score_kernel<DPV><<<(unsigned)S.G, TT_LANES, 0, st>>>(cores, n, D, S.h, B, ntiles, idx, w, (const double*)(base + S.hdr),    \
                                                              logq, status, (double*)(base + S.slices), S.slice,                    \
                                                              (int*)(base + S.islices), S.islice, (double*)(base + S.parts),        \
                                                              (double*)(base + S.wpart), want);                                     \
    break;
    TTN_SCORE_CASE(2)
    TTN_SCORE_CASE(4)
    default:
      TTN_SCORE_CASE(8)
#undef TTN_SCORE_CASE
  }
  e = hipGetLastError();
  if (e != hipSuccess || !want) return e;
  ttn_score_finish_kernel<<<(unsigned)(S.L - 1), MS_ENV_THREADS, 0, st>>>(n, D, S.h, S.G, (const double*)(base + S.parts),
                                                                      (const double*)(base + S.wpart), tt_env(S, base), grad_cores);
  return hipGetLastError();
}

}  // namespace bornvi
