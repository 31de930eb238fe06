/* bornvi_twosite.h -- two-site (DMRG-style) sweeps of the sampled MPS Born machine (kernels_mps_twosite.hip, DESIGN.md
 * section 6o).  A header of its own beside bornvi.h, in the same narrow subset of C (block comments, plain
 * `#define NAME <decimal>`, declarations `ret bornvi_name(args);`), read by the Python binding with the same parser into
 * tables of its own; the handle, the stream, the status codes and every convention are bornvi.h's.
 *
 * cores dev [n, 2, D, D] float64, psi(z) = e0^T A_1[z_1] .. A_n[z_n] e0, z_k = bit n - k of the index word.  ON ENTRY the
 * sites 2 .. n are right-canonical and Z = 1: what bornvi_mps_canonicalise writes.  idx dev [B] int64 samples; w dev [B]
 * weights >= 0, or NULL for 1 / B each.
 *
 * bornvi_mps_twosite_sweep is one ROUND TRIP over the bonds, k = 1 .. n - 1 left to right and then n - 1 .. 1 right to left;
 * cores is replaced in place and has the entry gauge again, so calls can be repeated.  At bond (k, k + 1), the j-th visited:
 *   M[s, t] = A_k[s] A_{k+1}[t] (four D x D blocks; in this gauge Z = |M|_F^2);
 *   psi_b = l_b^T M[s_b, t_b] r_b with l_b = e0^T A_1 .. A_{k-1} and r_b = A_{k+2} .. A_n e0 of the sample's own bits;
 *   L = W log |M|^2 - sum_b w_b log psi_b^2, W the sum of the weights of the samples that count (psi_b finite and not 0);
 *   `steps` plain descent steps M <- M - lr dL/dM, each followed by M <- M / |M|_F;  loss[j] = L after the last one;
 *   the split: M unfolded to 2 D x 2 D (rows (s, a), columns (t, c)) = U S V^T by the one-sided Jacobi of the canonicaliser,
 *     the values sorted descending, ties by index, cut by the canonicaliser's rule (the D_keep largest stay, then more go
 *     from the small end for as long as the dropped squares' normalised sum stays <= cutoff, one always stays; the rank
 *     rule's exact zeros go);  going right A_k = U_kept, A_{k+1} = (S_kept / |S_kept|) V_kept^T;  going left
 *     A_k = U_kept S_kept / |S_kept|, A_{k+1} = V_kept^T.  Everything beyond the kept rank is exactly 0.0, the first core's
 *     rows >= 1 and the last core's columns >= 1 included.
 * Outputs: loss dev [2 (n - 1)];  and from the return pass schmidt dev [n - 1, D] (the kept values over their norm,
 * descending, then 0.0), discarded dev [n - 1] (the dropped squares over all squares), rank dev [n - 1] int32.
 * status dev [1] int32, a sum of:  1 a non-finite core entry or a |M| that is not finite and positive (the outputs are NaN);
 * 2 some psi_b was 0 or not finite (that sample is left out at that bond, nothing it touches becomes NaN);  4 a
 * factorisation still rotated in its last allowed sweep;  8 at some bond as formed | |M|^2 - 1 | > 2^-20: the entry gauge
 * was not canonical (the call completes).
 * 2 <= n <= 63, 1 <= D <= 16, 1 <= B <= 2^20, 1 <= steps <= 64, 1 <= D_keep <= D, lr finite and >= 0, 0 <= cutoff < 1:
 * anything else, a short workspace included, is BORNVI_ERR_UNSUPPORTED before any launch, with nothing written.  The
 * launches form one chain on `stream`: no atomics (two calls are bitwise equal), no allocation, synchronisation or
 * read-back (capturable).  The workspace keeps every sample's left or right vector at every site: about 8 n D B bytes. */
#ifndef BORNVI_TWOSITE_H
#define BORNVI_TWOSITE_H

#include "bornvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BORNVI_MPS_TWOSITE_MAX_BOND 16        /* the merged 2D x 2D matrix must fit the factorisation's 64 x 32 */
#define BORNVI_MPS_TWOSITE_MAX_BATCH 1048576  /* 2^20: samples per call */
#define BORNVI_MPS_TWOSITE_MAX_STEPS 64       /* descent steps per bond */

size_t bornvi_mps_twosite_workspace_bytes(bornvi_handle h, int n, int D, long long B);
int bornvi_mps_twosite_sweep(bornvi_handle h, int n, int D, long long B, double* cores, const long long* idx, const double* w,
                             double lr, int steps, int D_keep, double cutoff, double* loss, double* schmidt, double* discarded,
                             int* rank, int* status, void* workspace, size_t workspace_bytes, bornvi_stream stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BORNVI_TWOSITE_H */
