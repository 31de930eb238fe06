/* bornvi_cmps.h -- the sampled MPS Born machine with COMPLEX cores (kernels_cmps.hip).  A header of
 * its own beside bornvi.h, in the same narrow subset of C (block comments, plain `#define NAME <decimal>`, declarations
 * `ret bornvi_name(args);`), read by the Python binding with the same parser into tables of its own; the handle, the
 * stream, the status codes and every convention are bornvi.h's.
 *
 * cores dev float64 [n, 2, D, D, 2], (re, im) last: torch.view_as_real of a complex128 [n, 2, D, D].  A_k[s] = X + iY.
 *   psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0 in C (a plain product, no conjugate),  q(z) = |psi(z)|^2 / Z,  Z = sum_z |psi(z)|^2.
 *   Bit order, index word and boundary vectors are those of the real family (bornvi.h): z_k is bit
 *   n - k of the index word.
 * Environments (Hermitian, positive semi-definite):  E_n = e0 e0^T, E_{k-1} = sum_s A_k[s] E_k A_k[s]^H;  L_0 = e0 e0^T,
 *   L_k = sum_s A_k[s]^T L_{k-1} conj(A_k[s]);  Z = Re E_0[0, 0].  After every step each matrix is multiplied by 2^-e, e the
 *   ilogb of its largest |re| or |im|, the running sum of the e's kept beside it; log Z from the mantissa and the exponents.
 *
 * bornvi_cmps_environments: the environments and log Z (log_Z_out dev [1], may be NULL) into the workspace, where they stay
 *   for the two calls below: call those next with the same (n, D, B, cores, workspace) on the same stream.
 * bornvi_cmps_sample: exact ancestral draws.  At site k with l = e0^T A_1 .. A_{k-1} of the bits drawn so far:
 *   u_s = l A_k[s], m_s = Re(u_s E_k u_s^H), z_k = [U_k (m_0 + m_1) >= m_0], U_k the Philox4x32-10 uniform of
 *   bornvi_mps_sample at (seed, epoch, b, k), the same key and counter; l <- u_{z_k} times a power of two.
 *   idx dev [B] int64, logq dev [B] = log|l_n[0]|^2 - log Z.  A draw depends on (seed, epoch, b, k) and the sample's own
 *   earlier bits only: not on B, the grid or the tiling.  status dev [1] int32: 1 when some m_0 + m_1 was 0 or not finite
 *   (that sample's remaining bits are 0 and its logq NaN).  epoch_dev dev [1] int64 is read by the kernel.
 * bornvi_cmps_score_vjp: grad_cores dev [n, 2, D, D, 2] = the gradient of the real function sum_b w_b log q(idx_b) with
 *   respect to the 2 . 2 n D^2 real numbers of cores (what an optimiser steps):  with T_b = l_{b,k-1}[a] r_{b,k+1}[c] / psi_b
 *   at block [k, z_{b,k}] the sample term is d/dX = 2 w_b Re T_b, d/dY = -2 w_b Im T_b;  with
 *   G_k[s] = L_{k-1} conj(A_k[s]) E_k^T / Z the environment term d log Z / dX = 2 Re G, d log Z / dY = -2 Im G is
 *   subtracted (sum_b w_b) times.  Entries of the first and last core that do not enter psi get exactly 0.0.
 *   logq dev [B] = log q(idx_b) (-inf where psi is 0).  status: 2 when some psi_b was 0 or not finite (weight 0 in the
 *   sample term).
 * With every imaginary part +0.0 the family is the real one: the draws are bornvi_mps_sample's given the same environments,
 *   and the imaginary half of the gradient is exactly 0.0.
 * The status word is cleared by a one-lane kernel in front of the launch.  No atomics (two calls are bitwise equal), no
 * allocation, synchronisation or read-back (capturable).  1 <= n <= BORNVI_MPS_SAMPLED_MAX_N, 1 <= D <=
 * BORNVI_CMPS_MAX_BOND, 1 <= B <= BORNVI_MPS_SAMPLED_MAX_BATCH: anything else, a short workspace included, is
 * BORNVI_ERR_UNSUPPORTED before any launch, with nothing written.  The workspace is bounded in B: at most 256 tiles of
 * 64 samples are in flight. */
#ifndef BORNVI_CMPS_H
#define BORNVI_CMPS_H

#include "bornvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BORNVI_CMPS_MAX_BOND 16  /* a complex lane vector of 16 has the register cost of the real kernels' D = 32 */

size_t bornvi_cmps_workspace_bytes(bornvi_handle h, int n, int D, long long B);
int bornvi_cmps_environments(bornvi_handle h, int n, int D, long long B, const double* cores, double* log_Z_out,
                             void* workspace, size_t workspace_bytes, bornvi_stream stream);
int bornvi_cmps_sample(bornvi_handle h, int n, int D, long long B, const double* cores, unsigned long long seed,
                       const long long* epoch_dev, long long* idx, double* logq, int* status, void* workspace,
                       size_t workspace_bytes, bornvi_stream stream);
int bornvi_cmps_score_vjp(bornvi_handle h, int n, int D, long long B, const double* cores, const long long* idx,
                          const double* w, double* logq, double* grad_cores, int* status, void* workspace,
                          size_t workspace_bytes, bornvi_stream stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BORNVI_CMPS_H */
