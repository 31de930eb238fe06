/* bornvi_lps.h -- the sampled MPS Born machine as a LOCALLY PURIFIED STATE (kernels_lps.hip).  The
 * fifth header, in bornvi_cmps.h's subset of C (block comments, plain `#define NAME <decimal>`, declarations
 * `ret bornvi_name(args);`), read by the Python binding with the same parser into tables of its own; the handle, the
 * stream, the status codes and every convention not restated here are bornvi.h's.
 *
 * Parameter layout.  cores dev float64 [n, 2, m, D, D], real: A_k[s, mu] in R^{D x D}, s the bit, mu = 0 .. m - 1 the
 *   purification index that is summed out.  1 <= n <= BORNVI_MPS_SAMPLED_MAX_N, 1 <= D <= BORNVI_LPS_MAX_BOND,
 *   1 <= m <= BORNVI_LPS_MAX_PURIFICATION, 1 <= B <= BORNVI_MPS_SAMPLED_MAX_BATCH.  Bit order, index word and boundary
 *   vectors e0 are those of the real family (bornvi.h): z_k is bit n - k of the index word.
 * Definitions.
 *   Amplitude:  psi(z, mu) = e0^T A_1[z_1, mu_1] ... A_n[z_n, mu_n] e0.
 *   Unnormalised mass:  T(z) = sum_{mu_1 .. mu_n} psi(z, mu)^2.   Normaliser and distribution:  Z = sum_z T(z),  q = T / Z.
 *   Left density:  rho_0 = e0 e0^T,  rho_k = sum_mu A_k[z_k, mu]^T rho_{k-1} A_k[z_k, mu]  (symmetric, positive
 *     semi-definite);  T(z) = rho_n[0, 0].
 *   Right density:  R_n = e0 e0^T,  R_{k-1} = sum_mu A_k[z_k, mu] R_k A_k[z_k, mu]^T.
 *   Environments:  E_n = e0 e0^T,  E_{k-1} = sum_{s,mu} A_k[s, mu] E_k A_k[s, mu]^T;   L_0 = e0 e0^T,
 *     L_k = sum_{s,mu} A_k[s, mu]^T L_{k-1} A_k[s, mu];   Z = E_0[0, 0].
 * Rescaling.  Every matrix (and the sampler's vector) is multiplied after every step by 2^-e, e the ilogb of its largest
 *   magnitude (exact; 0 when that is 0 or not finite), and the running sum of the e's is carried beside it, as in section
 *   6g.  The per-sample densities use the same rule: the largest magnitude of the 16 x 16 tile.
 * Gradient of sum_b w_b log q(z_b).  Sample term: the block [k, z_{b,k}, mu] receives
 *   (2 w_b / T_b) rho_{b,k-1} A_k[z_{b,k}, mu] R_{b,k}.   Environment term: every block [k, s, mu] loses
 *   (sum_b w_b) 2 L_{k-1} A_k[s, mu] E_k / Z.   Entries of the first and last core that do not enter psi get exactly 0.0.
 *
 * bornvi_lps_environments: E, L, their exponents and log Z (log_Z_out dev [1], may be NULL) into the workspace, where they
 *   stay for the two calls below: call those next with the same (n, m, D, B, cores, workspace) on the same stream.  The
 *   chain of an entry is the real family's with (s, mu) as the outer loop, s major: at m = 1 the bits are
 *   bornvi_mps_environments'.
 * bornvi_lps_sample: exact draws of z, by drawing (z_k, mu_k) jointly with pure-state vectors and discarding mu; one
 *   sample per lane.  At site k with l the vector of the (z, mu) drawn so far:  u_{s,mu} = l A_k[s, mu],
 *   m_{s,mu} = u E_k u^T;  M0 = sum_mu m_{0,mu}, M1 likewise, each summed in ascending mu;  M = M0 + M1;
 *   z_k = [U_k M >= M0], U_k the Philox4x32-10 uniform of bornvi_mps_sample at (seed, epoch, b, k), one uniform a site;
 *   mu_k = the number of partial sums c_j = m_{z,0} + ... + m_{z,j}, j < m - 1, with U_k M - z_k M0 >= c_j;
 *   l <- u_{z_k,mu_k} times a power of two.  idx dev [B] int64.  aux dev [B, 2] int64, may be NULL: the mu draws, two bits a
 *   site, site k at bits 2 ((k - 1) mod 32) of word (k - 1) / 32 (sites 1 .. 32 in word 0, 33 .. 63 in word 1), so that a
 *   draw can be replayed.  No logq: the vector's norm is that of the joint (z, mu), not of z.  status dev [1] int32: 1 when
 *   some M was 0 or not finite (that sample's remaining bits and mu's are 0).  epoch_dev dev [1] int64 is read by the kernel.
 * bornvi_lps_score_vjp: logq dev [B] = log T(idx_b) - log Z from the left density sweep (-inf where T is 0).  With
 *   grad_cores (dev [n, 2, m, D, D]) not NULL also the right sweep and the gradient above; with grad_cores NULL logq only,
 *   the same bits, with no right sweep and no gradient work: the family's log_prob.  status: 2 when some T_b was 0 or not
 *   finite (weight 0 in the sample term).
 * The density sweeps and the gradient run on v_mfma_f64_16x16x4_f64, one sample's zero-padded D x D matrix per 16 x 16
 *   tile; a workgroup of four waves takes BORNVI_LPS_SCORE_TILE samples at a time (four each), at most
 *   G = BORNVI_LPS_MAX_WG_SMALL (D <= 8) or BORNVI_LPS_MAX_WG_LARGE (D > 8) workgroups walk the tiles wg, wg + G, ...; the
 *   workspace holds the right densities of the tiles in flight [G][n][BORNVI_LPS_SCORE_TILE][D^2] and one partial gradient
 *   per workgroup: bounded in B, 0.74 GiB at (n, m, D) = (63, 4, 16) and at (63, 4, 8).
 * Draws and logq depend on (cores, seed, epoch, b) only: not on B, the grid or the tiling.  The status word is cleared by a
 * one-lane kernel in front of the launch.  No atomics, fixed-order partials (two calls are bitwise equal), no allocation,
 * synchronisation or read-back (capturable).  Anything out of range, a short workspace included, is
 * BORNVI_ERR_UNSUPPORTED before any launch, with nothing written. */
#ifndef BORNVI_LPS_H
#define BORNVI_LPS_H

#include "bornvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BORNVI_LPS_MAX_BOND 16          /* one 16 x 16 matrix-core tile per density */
#define BORNVI_LPS_MAX_PURIFICATION 4
#define BORNVI_LPS_SCORE_TILE 16        /* samples a workgroup of the score kernel takes at a time */
#define BORNVI_LPS_MAX_WG_SMALL 1024    /* workgroups of the score kernel at most, D <= 8 */
#define BORNVI_LPS_MAX_WG_LARGE 256     /* and for D > 8 */

size_t bornvi_lps_workspace_bytes(bornvi_handle h, int n, int m, int D, long long B);
int bornvi_lps_environments(bornvi_handle h, int n, int m, int D, long long B, const double* cores, double* log_Z_out,
                            void* workspace, size_t workspace_bytes, bornvi_stream stream);
int bornvi_lps_sample(bornvi_handle h, int n, int m, int D, long long B, const double* cores, unsigned long long seed,
                      const long long* epoch_dev, long long* idx, long long* aux, int* status, void* workspace,
                      size_t workspace_bytes, bornvi_stream stream);
int bornvi_lps_score_vjp(bornvi_handle h, int n, int m, int D, long long B, const double* cores, const long long* idx,
                         const double* w, double* logq, double* grad_cores, int* status, void* workspace,
                         size_t workspace_bytes, bornvi_stream stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BORNVI_LPS_H */
