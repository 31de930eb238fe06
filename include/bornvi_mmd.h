/* bornvi_mmd.h -- squared maximum mean discrepancy with a kernel of the Hamming distance (kernels_mmd.hip, DESIGN.md section
 * 6q).  A header of its own beside bornvi.h, in the same narrow subset of C (block comments, plain `#define NAME <decimal>`,
 * declarations `ret bornvi_name(args);`), read by the Python binding with the same parser into tables of its own; the handle,
 * the stream, the status codes and every convention are bornvi.h's.
 *
 * The kernel is a table kappa[d], d = 0 .. n, of the Hamming distance of two states; the callers here use
 *   kappa[d] = sum_c a_c rho_c^d,  rho_c = exp(-1 / (n l_c)),  a_c = 1 / C,  1 <= C <= BORNVI_MMD_MAX_SCALES,
 * whose spectrum under the Walsh-Hadamard transform H = [[1, 1], [1, -1]]^(x n) is
 *   lam[j] = sum_c a_c (1 + rho_c)^(n - j) (1 - rho_c)^j > 0,   K = 2^-n H diag(lam[popcount k]) H,   2^-n sum_k lam[pop k] = kappa[0].
 * Both tables are the caller's, in device memory.  Tuple position p is bit n - 1 - p of the index word, as everywhere.
 *
 * bornvi_mmd_weights (1 <= n <= BORNVI_TABLE_MAX_N): q, target dev [2^n] float64 (target may be NULL: zeros), lam dev [n + 1].
 *   With d = q - target:  loss dev [1] = d^T K d = 2^-n sum_k lam[pop k] dhat_k^2 (dhat = H d; >= 0, and exactly 0.0 when d is 0);
 *   w dev [2^n] = 2 K d = d loss / d q.  w may be NULL: the loss alone, the call stops after the forward transform.
 *   q, target and w are 16-byte aligned.  target may be q itself; w overlaps neither.
 *   A pass keeps a tile of 2^BORNVI_MMD_TILE_BITS doubles in LDS and transforms up to BORNVI_MMD_TILE_BITS low or
 *   BORNVI_MMD_HIGH_BITS high index bits; bornvi_mmd_passes(n) is the number of tile passes of a call with w (1, 3, 5: n <=
 *   12, <= 21, <= 30), 0 for an n out of range.  w is the scratch between passes; the workspace holds the per-tile partials of
 *   the loss, and the 2^n doubles between passes when w is NULL.
 *   Error per entry (both transforms, the scale and the factor 2): |w_z - exact| <= 2 (2 n + 4) eps kappa[0] ||d||_1.
 *
 * bornvi_hamming_pairs_rowsum (1 <= n <= 63, 1 <= A <= BORNVI_HAMMING_PAIRS_MAX_A, 1 <= B <= BORNVI_HAMMING_PAIRS_MAX_B):
 *   za dev [A], zb dev [B] int64 index words, kappa dev [n + 1].
 *   cnt_a[d] = #{ j : popcount(za_a xor zb_j) = d, and, with skip_same_index != 0, j != a }: exact integers.
 *   r dev [A]:  r_a = sum_{d = 0 .. n} kappa[d] * (double)cnt_a[d], in ascending d, multiply and add rounded separately.
 *   total dev [1] = sum_a r_a in the fixed order of the library's reductions.  counts dev [A, n + 1] int32 or NULL.
 *   r_a depends on (za_a, the multiset of zb, kappa) only (with skip_same_index: zb without its entry a): not on A, not on the
 *   grid or the tiling, not on the order of zb.  Duplicated states are counted as often as they occur.
 *   Bits at or above n must be 0 in both arrays; the kernels never look at them.
 *
 * Both calls: anything out of range, a short workspace included, is BORNVI_ERR_UNSUPPORTED before any launch, with nothing
 * written.  No atomics on floating-point data (two calls are bitwise equal), no allocation, synchronisation or read-back
 * (capturable); the workspace is never read before it is written. */
#ifndef BORNVI_MMD_H
#define BORNVI_MMD_H

#include "bornvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BORNVI_MMD_MAX_SCALES 8              /* length scales of a mixture kernel */
#define BORNVI_MMD_TILE_BITS 12              /* 2^12 doubles = 32 KiB of LDS a workgroup: four workgroups per CU */
#define BORNVI_MMD_HIGH_BITS 9               /* a high pass's rows keep 2^(12 - 9) doubles = 64 contiguous bytes */
#define BORNVI_HAMMING_PAIRS_MAX_A 131072    /* 2^17 rows (model samples) */
#define BORNVI_HAMMING_PAIRS_MAX_B 1048576   /* 2^20 columns (data) */

int bornvi_mmd_passes(int n);
size_t bornvi_mmd_workspace_bytes(bornvi_handle h, int n);
int bornvi_mmd_weights(bornvi_handle h, int n, const double* q, const double* target, const double* lam,
                       double* loss, double* w, void* workspace, size_t workspace_bytes, bornvi_stream stream);

size_t bornvi_hamming_pairs_workspace_bytes(bornvi_handle h, int n, long long A, long long B);
int bornvi_hamming_pairs_rowsum(bornvi_handle h, int n, long long A, const long long* za, long long B, const long long* zb,
                                int skip_same_index, const double* kappa, double* r, double* total, int* counts,
                                void* workspace, size_t workspace_bytes, bornvi_stream stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BORNVI_MMD_H */
