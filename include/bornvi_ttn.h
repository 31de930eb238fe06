/* bornvi_ttn.h -- the sampled Born machine on a binary TREE TENSOR NETWORK (kernels_ttn.hip).  The
 * sixth header, in bornvi_lps.h's subset of C (block comments, plain `#define NAME <decimal>`, declarations
 * `ret bornvi_name(args);`), read by the Python binding with the same parser into tables of its own; the handle, the
 * stream, the status codes and every convention not restated here are bornvi.h's.
 *
 * Tree.  h = max(1, ceil(log2 n)), L = 2^h leaf positions, 1 <= n <= 63, so L <= 64.  Position j < n holds tuple position j:
 *   z_{j+1}, bit n - 1 - j of the int64 outcome index, the real family's bit order.  Positions j >= n are padding and carry
 *   the fixed value 0.  Nodes are heap-numbered v = 1 .. L - 1, their children are 2 v and 2 v + 1; nodes v >= L / 2 are
 *   bottom nodes, their children are the positions 2 (v - L / 2) and 2 (v - L / 2) + 1.
 * Parameter.  cores dev float64 [L - 1, D, D, D]: cores[v - 1] = T_v[p, a, b], p the parent bond, a, b the left and right
 *   child bonds.  2 <= D <= BORNVI_TTN_MAX_BOND, 1 <= B <= BORNVI_MPS_SAMPLED_MAX_BATCH.  A leaf is the one-hot vector e_z in
 *   R^D, so a bottom node is an ordinary node whose children are one-hot.
 * Dead entries.  Never read, and their gradient is exactly 0.0: the root at p >= 1; a bottom node at a >= 2 or b >= 2; a
 *   bottom node at the value 1 of a padding child.
 * Amplitude.  x_v[p] = sum_{a,b} T_v[p, a, b] x_{2v}[a] x_{2v+1}[b], contracted as M = T x_{2v} over a, then M x_{2v+1} over b;
 *   psi(z) = x_1[0];  Z = sum_z psi(z)^2;  q = psi^2 / Z.
 * Environments.  Up densities: U_v = sum_{z in the subtree} x_v x_v^T (padding values are not summed over).  Down densities:
 *   V_1 = e0 e0^T,  V_{2v}[a, a'] = sum V_v[p, p'] T[p, a, b] T[p', a', b'] U_{2v+1}[b, b'],  V_{2v+1} the same with U_{2v}.
 *   Z = U_1[0, 0].  dZ/dT_v[p, a, b] = 2 sum V_v[p, p'] T_v[p', a', b'] U_{2v}[a, a'] U_{2v+1}[b, b'].
 * Per-sample down vectors.  y_1 = e0,  y_{2v}[a] = sum y_v[p] T[p, a, b] x_{2v+1}[b],  y_{2v+1}[b] = sum y_v[p] T[p, a, b] x_{2v}[a].
 * Gradient of sum_b w_b log q(z_b).  Block v receives sum_b (2 w_b / psi_b) y_{b,v} (x) x_{b,2v} (x) x_{b,2v+1} and loses
 *   (sum_b w_b) dZ/dT_v / Z.
 * Rescaling.  Every vector and density is multiplied after every step by 2^-e, e the ilogb of its largest magnitude (exact; 0
 *   when that is 0 or not finite), and the running sum of the e's is carried beside it, as in section 6g; a node's exponent
 *   is its own plus its children's.
 * Sampler.  Depth first, positions left to right, exact.  Node v has the density P_v of everything outside its subtree (drawn
 *   positions as pure vectors, undrawn ones traced), P_1 = e0 e0^T.  At a node:
 *   P_{2v}[a, a'] = sum P_v[p, p'] T[p, a, b] T[p', a', b'] U_{2v+1}[b, b'];  descend left, which returns x_{2v};  M = T x_{2v},
 *   P_{2v+1} = M^T P_v M;  descend right;  return x_v = M x_{2v+1}.  A position with density P has the masses m_0 = P[0, 0],
 *   m_1 = P[1, 1] and draws z = [U (m_0 + m_1) >= m_0]; a padding position draws nothing and is 0.  U for position j is
 *   bornvi_mps_sample's Philox4x32-10 uniform at (seed, epoch, b, k = j + 1).
 *
 * bornvi_ttn_environments: U, V, the products T U_{2v+1} and T U_{2v} U_{2v+1}, their exponents and log Z (log_Z_out dev [1], may
 *   be NULL) into the workspace, where they stay for the two calls below: call those next with the same (n, D, B, cores,
 *   workspace) on the same stream.
 * bornvi_ttn_sample: idx dev [B] int64, logq dev [B] = log x_1[0]^2 - log Z: the sampler and the score call share the device
 *   function for x_v, so this logq equals the score call's bit for bit.  status dev [1] int32: 1 when some m_0 + m_1 was 0 or
 *   not finite (that sample's remaining bits are 0 and its logq is NaN).  epoch_dev dev [1] int64 is read by the kernel.
 * bornvi_ttn_score_vjp: logq dev [B]; with grad_cores (dev [L - 1, D, D, D]) not NULL also the down sweep and the gradient
 *   above; with grad_cores NULL logq only, the same bits (then w may be NULL).  status: 2 when some psi_b is 0 or not finite
 *   (weight 0 in the sample term), or Z is not positive and finite.
 * One sample per lane, one wave per workgroup; at most BORNVI_TTN_MAX_WG workgroups walk the tiles of 64 samples wg, wg + G, ...
 *   The workspace holds the environments, per workgroup the vectors of the tile in flight (the sampler's density stack for
 *   D > 4; x_v, y_v of every node for the score call) and one partial gradient: bounded in B, 0.78 GiB at (n, D) = (63, 8).
 * Draws and logq depend on (cores, seed, epoch, b) only: not on B, the grid or the tiling.  The status word is cleared by a
 * one-lane kernel in front of the launch.  No atomics, fixed-order partials (two calls are bitwise equal), no allocation,
 * synchronisation or read-back (capturable).  Anything out of range, a short workspace included, is
 * BORNVI_ERR_UNSUPPORTED before any launch, with nothing written. */
#ifndef BORNVI_TTN_H
#define BORNVI_TTN_H

#include "bornvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BORNVI_TTN_MAX_BOND 8
#define BORNVI_TTN_MAX_WG 1024          /* workgroups of the sampler and of the score kernel at most */

size_t bornvi_ttn_workspace_bytes(bornvi_handle h, int n, int D, long long B);
int bornvi_ttn_environments(bornvi_handle h, int n, int D, long long B, const double* cores, double* log_Z_out,
                            void* workspace, size_t workspace_bytes, bornvi_stream stream);
int bornvi_ttn_sample(bornvi_handle h, int n, int D, long long B, const double* cores, unsigned long long seed,
                      const long long* epoch_dev, long long* idx, double* logq, int* status, void* workspace,
                      size_t workspace_bytes, bornvi_stream stream);
int bornvi_ttn_score_vjp(bornvi_handle h, int n, int D, long long B, const double* cores, const long long* idx,
                         const double* w, double* logq, double* grad_cores, int* status, void* workspace,
                         size_t workspace_bytes, bornvi_stream stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BORNVI_TTN_H */
