// Launchers implemented in the kernels_*.hip files and called from api.hip, and the host helpers those files share
// (workspace alignment, raising a kernel's dynamic-LDS limit once per device).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>

#include "bornvi.h"

namespace bornvi {

// ---- workspaces and launch helpers ---------------------------------------------------------------
// Every launcher carves its caller's workspace from the first 256-byte boundary on, in 256-byte pieces.
inline size_t ws_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline char* ws_align(void* p) { return (char*)ws_round((size_t)(uintptr_t)p); }
// More than 64 KiB of dynamic LDS needs the kernel's attribute raised, once per device (idempotent, so a race between two
// threads' first calls is harmless).  Later calls -- the ones a stream capture may record -- touch no function attribute.
// One LdsRaised object per kernel, at namespace scope.
constexpr int MAX_DEVICES = 64;
struct LdsRaised {
  std::atomic<unsigned char> done[MAX_DEVICES];
};
inline hipError_t raise_lds_once(const void* fn, size_t bytes, LdsRaised& r) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool known = dev >= 0 && dev < MAX_DEVICES;
  if (known && r.done[dev].load(std::memory_order_acquire)) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess && known) r.done[dev].store(1, std::memory_order_release);
  return e;
}

// ---- circuit ------------------------------------------------------------------------------------
// Prefix sharing inside a parameter-shift batch (api.hip: circuit_batch): the circuits of the batch are ordered by
// the first pass their shifted parameter touches, slot 0 holds the base circuit; a pass runs the circuits that
// already differ from the base circuit, and those with index >= fresh_begin read the base circuit's state.
struct PrefixShare {
  long long fresh_begin = (1ll << 62);   // circuits >= fresh_begin read slot 0 of the input buffer
  const int* row_map = nullptr;          // final pass: output row of circuit b (< 0: goes to `trash`); null = row b
  double* trash = nullptr;               // 2^n doubles
};
// shift_tab (or null): per circuit of this launch, parameter * 2 + (1 for the minus shift), < 0 for the base circuit.
// gates: [batch][slots][8] doubles, slots >= nfused + 1.  normalise = 1 (circuit_pass_r3_kernel): pivot-normalised records
// (kernels_circuit.hip: build_gates_kernel) and, in slot nfused, the scale of the circuit's probabilities.
hipError_t launch_build_gates(const uint32_t* plan, int nfused, const double* thetas, long long theta_stride,
                              int shift_mode, int p_begin, int p_stride, int include_base, long long b_offset, int batch,
                              double* gates, const int* shift_tab, int slots, int normalise, hipStream_t st);
hipError_t launch_normalise_gates(double* gates, int count, hipStream_t st);   // raw [count][8] -> records, in place
hipError_t prepare_circuit_kernel(size_t lds_bytes);
hipError_t launch_circuit_pass(const uint32_t* plan, uint32_t pass_off, int n, int k, int threads, size_t lds, int batch,
                               const void* in, void* out, double* probs, const double* gates,
                               long long gate_stride, int max_workgroups, hipStream_t st);
// fast path (plan.hpp: build_fast_tables); persistent grid of at most max_workgroups workgroups
int circuit_fast_workgroups_per_cu(int threads, size_t lds);
hipError_t launch_circuit_pass_fast(const uint32_t* plan, uint32_t pass_off, const uint32_t* fast, uint32_t fast_off,
                                    int n, int k, size_t lds, int batch, const void* in, void* out, double* probs,
                                    const double* gates, long long gate_stride, int max_workgroups, size_t lds_tab_off,
                                    size_t lds_mats2_off, int direct_mask, const PrefixShare& share, hipStream_t st);
// 8 amplitudes per thread, compact tables (kernels_circuit8.hip; plan.hpp: CompactTables)
hipError_t prepare_circuit_r3_kernel(size_t lds_bytes);
int circuit_r3_workgroups_per_cu(int threads, size_t lds);
hipError_t launch_circuit_pass_r3(const uint32_t* plan, uint32_t pass_off, const uint32_t* ctab, uint32_t ct_off,
                                  const uint32_t* hdr_host /* the pass's compact header on the host */, int n, int k,
                                  size_t lds, int batch, const void* in, void* out, double* probs, const double* gates,
                                  long long gate_stride, int max_workgroups, int direct_mask, const PrefixShare& share,
                                  const double* wdot, double* partials, hipStream_t st);
// grad[p] = s * (sum_g partials[(2p) * tiles + g] - sum_g partials[(2p + 1) * tiles + g]),  s = 1/2 (ksd2 == null) or
// 1/2 / sqrt(max(ksd2, 1e-12)) with the clamp's zero gradient below 1e-12; loss_out (or null) = sqrt(max(ksd2, 1e-12))
hipError_t launch_dot_finish(const double* partials, int n_shift, long long tiles, const double* ksd2, double* grad,
                             double* loss_out, hipStream_t st);
hipError_t launch_gate1q(double* state, int n, long long batch, int wire, const double* U, hipStream_t st);
hipError_t launch_cnot(double* state, int n, long long batch, int control, int target, hipStream_t st);
hipError_t launch_born_probs(const double* state, double* probs, int n, long long batch, hipStream_t st);
hipError_t launch_shift_dot(const double* shifted, int n_shift, const double* w, const double* ksd2, int n,
                            double* grad, double* loss_out, hipStream_t st);
hipError_t launch_clip_cast(const double* g64, int P, double max_norm, float* g32, float* norm_out, const double* loss,
                            float* found_inf, hipStream_t st);
hipError_t launch_clip_adam(const double* g64, int P, double max_norm, const double* loss, float* theta, float* g32,
                            double* theta64, float* exp_avg, float* exp_avg_sq, int* counters, const double* lr_table,
                            int n_lr, double beta1, double beta2, double eps, float* norm_out, double* loss_hist,
                            float* norm_hist, hipStream_t st);
hipError_t launch_dldq(const double* y, const double* ksd2, int n, double* dLdq, double* loss_out, hipStream_t st);

// ---- finite-shot measurement (kernels_shots.hip) ------------------------------------------------------
size_t shots_workspace_bytes(int n, long long B);
hipError_t launch_shots_histogram(int n, long long B, const double* probs, double* freq, int shots, unsigned long long seed,
                                  const long long* epoch_dev, int include_base, int p_begin, int p_stride, void* ws,
                                  hipStream_t st);

// ---- classical Born machine, probability-table family (kernels_born_table.hip) -------------------------
size_t born_table_workspace_bytes(int n, long long rows);
hipError_t launch_born_table_probs(int n, long long rows, int mode, const float* w, float* q32, double* q64, float* H,
                                   void* ws, hipStream_t st);
hipError_t launch_born_table_vjp(int n, long long rows, int mode, const float* w, const double* q64, const double* y,
                                 const double* ksd2, double lam, float* grad, double* loss_out, void* ws, hipStream_t st);

// ---- exact ELBO of a Born distribution against a log-joint table (kernels_elbo.hip) --------------------
size_t elbo_workspace_bytes(int n, long long rows);
hipError_t launch_elbo_weights(int n, long long rows, const double* q, const double* log_p, double q_floor, double* w,
                               double* neg_elbo, double* entropy, void* ws, hipStream_t st);

// ---- matrix-product-state Born machine (kernels_mps.hip): cores [n, 2, D, D] -> q, and dL/dq -> dL/dcores ----------
size_t mps_workspace_bytes(int n, int D);
hipError_t launch_mps_probs(int n, int D, const double* cores, double* q64, float* q32, double* psi_out, double* Z_out, void* ws,
                            hipStream_t st);
hipError_t launch_mps_vjp(int n, int D, const double* cores, const double* g, double* grad_cores, void* ws, hipStream_t st);

// ---- sampled MPS Born machine (kernels_mps_sample.hip): environments, exact sampler, score gradient, log joint of samples
size_t mps_sample_workspace_bytes(int n, int D, long long B);
hipError_t launch_mps_environments(int n, int D, long long B, const double* cores, double* logZ_out, void* ws, hipStream_t st);
hipError_t launch_mps_environments_into(int n, int D, const double* cores, double* E, double* L, int* eE, int* eL, double* hdr,
                                        hipStream_t st);
hipError_t launch_mps_sample(int n, int D, long long B, const double* cores, unsigned long long seed, const long long* epoch_dev,
                             long long* idx, double* logq, int* status, void* ws, hipStream_t st);
hipError_t launch_mps_score_vjp(int n, int D, long long B, const double* cores, const long long* idx, const double* w, double* logq,
                                double* grad_cores, int* status, void* ws, hipStream_t st);
hipError_t launch_mps_score_rows(int n, int D, long long B, const double* cores, const long long* idx, int k_begin, int k_count,
                                 long long ld, double* rows, int* status, void* ws, hipStream_t st);
hipError_t launch_ms_clear_status(int* status, hipStream_t st);      // the one-lane clear in front of every status writer
hipError_t launch_mps_score_mu(int n, int D, long long B, const double* cores, void* ws, const double** hdr, const double** mu,
                               hipStream_t st);
hipError_t launch_mps_score_jvp(int n, int D, long long B, const double* cores, const long long* idx, const double* v, double scale,
                                double* t, int* status, void* ws, hipStream_t st);
hipError_t launch_bn_logjoint_samples(const bornvi_bn_desc& bn, int n, long long B, const long long* idx, double p_floor, double* logp,
                                      hipStream_t st);
hipError_t launch_bn_sample(const bornvi_bn_desc& bn, int n, long long B, unsigned long long seed, const long long* epoch_dev,
                            long long* idx, double* logp, int* status, hipStream_t st);

// ---- exact posterior queries of the sampled MPS (kernels_mps_query.hip): log-marginals, clamped sampler, marginals ----
size_t mps_query_workspace_bytes(int n, int D, int Q);
hipError_t launch_mps_log_marginals(int n, int D, int Q, const double* cores, const long long* mask, const long long* value,
                                    double* logm, int* status, void* ws, hipStream_t st);
hipError_t launch_mps_sample_clamped(int n, int D, long long B, const double* cores, const long long* mask, const long long* value,
                                     unsigned long long seed, const long long* epoch_dev, long long* idx, double* logq, double* logm,
                                     int* status, void* ws, hipStream_t st);
hipError_t launch_mps_marginals(int n, int D, const double* cores, double* m1, double* m2, void* ws, hipStream_t st);
// the gradient of weighted log-marginals: groups = the workgroups that take queries = the partials per entry
size_t mps_log_marginals_vjp_workspace_bytes(int n, int D, int Q);
int mps_log_marginals_vjp_groups(int Q);
hipError_t launch_mps_log_marginals_vjp(int n, int D, int Q, const double* cores, const long long* mask, const long long* value,
                                        const double* c, double* grad, double* logm, int* status, void* ws, hipStream_t st);

// ---- canonical form, bond spectra and truncation of an MPS (kernels_mps_canon.hip): one workgroup, two Jacobi sweeps ----
size_t mps_canon_workspace_bytes(int n, int D);
hipError_t launch_mps_canonicalise(int n, int D, int D_out, double cutoff, const double* cores, double* cores_out, double* schmidt,
                                   double* discarded, int* rank, double* log_norm, int* status, void* ws, hipStream_t st);

// ---- two-site sweeps of the sampled MPS (kernels_mps_twosite.hip): one round trip over the bonds, a chain of small launches ----
size_t mps_twosite_workspace_bytes(int n, int D, long long B);
hipError_t launch_mps_twosite_sweep(int n, int D, long long B, double* cores, const long long* idx, const double* w, double lr,
                                    int steps, int D_keep, double cutoff, double* loss, double* schmidt, double* discarded, int* rank,
                                    int* status, void* ws, hipStream_t st);

// ---- sampled MPS Born machine with complex cores (kernels_cmps.hip): cores [n, 2, D, D, 2], D <= 16 ----
size_t cmps_workspace_bytes(int n, int D, long long B);
hipError_t launch_cmps_environments(int n, int D, long long B, const double* cores, double* logZ_out, void* ws, hipStream_t st);
hipError_t launch_cmps_sample(int n, int D, long long B, const double* cores, unsigned long long seed, const long long* epoch_dev,
                              long long* idx, double* logq, int* status, void* ws, hipStream_t st);
hipError_t launch_cmps_score_vjp(int n, int D, long long B, const double* cores, const long long* idx, const double* w, double* logq,
                                 double* grad_cores, int* status, void* ws, hipStream_t st);

// ---- sampled MPS Born machine as a locally purified state (kernels_lps.hip): cores [n, 2, m, D, D], D <= 16, m <= 4 ----
size_t lps_workspace_bytes(int n, int m, int D, long long B);
hipError_t launch_lps_environments(int n, int m, int D, long long B, const double* cores, double* logZ_out, void* ws, hipStream_t st);
hipError_t launch_lps_sample(int n, int m, int D, long long B, const double* cores, unsigned long long seed, const long long* epoch_dev,
                             long long* idx, long long* aux, int* status, void* ws, hipStream_t st);
hipError_t launch_lps_score_vjp(int n, int m, int D, long long B, const double* cores, const long long* idx, const double* w, double* logq,
                                double* grad_cores, int* status, void* ws, hipStream_t st);

// ---- sampled Born machine on a binary tree tensor network (kernels_ttn.hip): cores [L - 1, D, D, D], 2 <= D <= 8 ----
size_t ttn_workspace_bytes(int n, int D, long long B);
hipError_t launch_ttn_environments(int n, int D, long long B, const double* cores, double* logZ_out, void* ws, hipStream_t st);
hipError_t launch_ttn_sample(int n, int D, long long B, const double* cores, unsigned long long seed, const long long* epoch_dev,
                             long long* idx, double* logq, int* status, void* ws, hipStream_t st);
hipError_t launch_ttn_score_vjp(int n, int D, long long B, const double* cores, const long long* idx, const double* w, double* logq,
                                double* grad_cores, int* status, void* ws, hipStream_t st);

// ---- MMD with a Hamming-distance kernel (kernels_mmd.hip): Walsh-Hadamard weights, pair counts by xor + popcount ----
int mmd_passes(int n);       // tile passes of a call with w: 1, 3, 5
size_t mmd_workspace_bytes(int n);
hipError_t launch_mmd_weights(int n, const double* q, const double* target, const double* lam, double* loss, double* w, void* ws,
                              hipStream_t st);
size_t hamming_pairs_workspace_bytes(int n, long long A, long long B);
hipError_t launch_hamming_pairs_rowsum(int n, long long A, const long long* za, long long B, const long long* zb, int skip_same_index,
                                       const double* kappa, double* r, double* total, int* counts, void* ws, hipStream_t st);

// ---- conjugate gradients on the device (kernels_cg.hip): the recurrence of (F + damping I) x = g around a caller's product ----
// state: BORNVI_CG_STATE_DOUBLES doubles -- rr, rr0, iterations, done, relres, fallback, 2 spare
hipError_t launch_cg_init(long long P, const double* g, double* x, double* r, double* p, double* state, int* info, hipStream_t st);
hipError_t launch_cg_step(long long P, double damping, double rel_tol, const double* Fp, double* x, double* r, double* p,
                          double* state, hipStream_t st);
hipError_t launch_cg_finish(long long P, const double* g, double* x, const double* state, int* info, int* iters, double* relres,
                            hipStream_t st);

// ---- sample-space Gram of the sampled MPS's score rows (kernels_mps_sample_gram.hip): T = O O^T / B without the rows ----
size_t mps_sample_gram_workspace_bytes(int n, int D, long long B);
hipError_t launch_mps_score_sample_gram(int n, int D, long long B, const double* cores, const long long* idx, double* T, int* status,
                                        void* env_ws, void* ws, hipStream_t st);

// ---- sampled KSD: scores of p at sampled states, pairwise Stein kernel row sums (kernels_ksd_sampled.hip) ----
size_t stein_pairs_workspace_bytes(long long B);
void stein_pairs_geometry(long long B, int* per_tiles, int* G);
hipError_t launch_bn_score_samples(const bornvi_bn_desc& bn, int n, long long B, const long long* idx, double p_floor, double* S,
                                   double* logp, hipStream_t st);
hipError_t launch_stein_pairs_rowsum(int n, long long B, double length_scale, const long long* idx, const double* S, double* r,
                                     double* total, void* ws, hipStream_t st);

// ---- natural gradient: Fisher matrix of the stored parameter-shift rows, damped Cholesky solve (kernels_fisher.hip)
size_t fisher_workspace_bytes(int n, int n_shift);
hipError_t launch_fisher_gram(int n, const double* shifted, int n_shift, const double* q, double q_floor, double* F, void* ws,
                              hipStream_t st);
size_t spd_solve_workspace_bytes(int P);
hipError_t launch_spd_solve(int P, const double* A, double damping, const double* b, double* x, int* info, void* ws, hipStream_t st);
size_t spd_solve_batched_workspace_bytes(int P, int nb);
hipError_t launch_spd_solve_batched(int P, int nb, const double* A, double damping, const double* b, double* x, int* info, void* ws,
                                    hipStream_t st);
size_t score_fisher_workspace_bytes(int R, int nblocks, long long ld);
hipError_t launch_score_fisher_gram(int R, int nblocks, long long B, long long ld, const double* rows, double* F, void* ws,
                                    hipStream_t st);

// ---- quantum natural gradient (kernels_qfi.hip): coherent states of pi-shifted circuits, quantum Fisher information
// thetas[c][p] = theta[p] + pi where p is the parameter of row row0 + c (row < include_base: the base circuit, no shift)
hipError_t launch_pi_shift_thetas(const double* theta, int P, int row0, int include_base, int p_begin, int bc, double* thetas,
                                  hipStream_t st);
struct StateTail {        // the gates that end a circuit: out[y] = s(y) in[A y] over the PHYSICAL index bits
  unsigned row[32];       // bit b of x = parity(y & row[b])
  unsigned cz[32];        // s(y) = (-1)^(sum_b y_b popcount(y & cz[b])): each CZ pair listed once
};
hipError_t launch_state_tail(const double* in, double* out, int n, int bc, const StateTail& T, hipStream_t st);
size_t qfi_workspace_bytes(int n, int P);
hipError_t launch_qfi_gram(int n, int P, const double* phi, const double* psi, double* Q, void* ws, hipStream_t st);

// ---- classical Born machine, REINFORCE step of the adversarial trainer (kernels_reinforce.hip) ---------
size_t reinforce_workspace_bytes(int n, long long B);
hipError_t launch_reinforce_step(int n, long long B, const long long* idx, const float* logit, const float* log_p,
                                 const float* q32, double* baseline, int first, double decay, double coef, double q_floor,
                                 double* dLdq, float* loss, float* found_inf, void* ws, hipStream_t st);

// ---- adjoint differentiation (kernels_adjoint.hip): gate-block walks over one / two states ------------
struct AdjRotBlock {      // consecutive one-qubit gates of one wire, applied e = 0 first (kinds: plan.hpp GateKind)
  int wire, nrot;
  int kind[4];
  int param[4];           // parameter index or -1
};
constexpr int ADJ_MAX_CZ = 136;     // CZ gates of one entangler block (all_to_all at n = 17: 136 pairs)
struct AdjEntangler {     // psi'[y] = s(y) psi[A y]: rows of A over the PHYSICAL index bits, CZ signs on linear functions of y
  unsigned row[32];       // bit b of x = parity(y & row[b])
  int ncz;
  unsigned za[ADJ_MAX_CZ], zb[ADJ_MAX_CZ];
};
int adjoint_workgroups(int n);   // workgroups of a rotation-block launch (partials per block = 4 * this)
hipError_t launch_adj_init(double* state, int n, hipStream_t st);
hipError_t launch_adj_rot_forward(double* state, int n, const AdjRotBlock& blk, const double* theta, hipStream_t st);
hipError_t launch_adj_rot_backward(double* phi, double* lam, int n, const AdjRotBlock& blk, const double* theta, double* partials,
                                   hipStream_t st);
hipError_t launch_adj_entangle(const double* in, double* out, const double* in2, double* out2, int n, const AdjEntangler& E,
                               int sign_on_src, hipStream_t st);
hipError_t launch_adj_lambda(const double* psi, const double* w, double* lam, int n, hipStream_t st);
hipError_t launch_adj_reduce(const double* partials, const int* slot_param, int nslots, int nwg, double* grad, hipStream_t st);

// ---- Stein ----------------------------------------------------------------------------------------
hipError_t launch_score(const bornvi_bn_desc& bn, int n, double* S, double* pxz, hipStream_t st);
// `ld`: row pitch of K in doubles (>= 2^n, even)
hipError_t launch_gram_build(int n, double length_scale, const double* S, double* K, long long row_begin,
                             long long row_end, long long ld, hipStream_t st);
hipError_t launch_kp_pairs(int n, double length_scale, long long M, const long long* zi, const long long* zj,
                           const double* si, const double* sj, double* out, hipStream_t st);
size_t quadform_partials(long long rows);  // number of per-workgroup partial sums
hipError_t launch_quadform(int n, const double* K, long long row_begin, long long row_end, const double* q,
                           double* y_or_null, double* ksd2, double* partials, hipStream_t st);
// batched Y = K Q^T on the matrix cores (kernels_batched.hip): n >= 8, B >= 2; Y must be given ([B, 2^n])
bool quadform_batched_supported(int n, int B);
hipError_t launch_quadform_batched(int n, const double* K, long long ld, const double* Q, int B, double* Y, double* ksd2, hipStream_t st);
size_t quadform_sym_workspace_doubles(int n);
hipError_t launch_quadform_sym(int n, const double* K, long long ld, const double* q, double* y_or_null, double* ksd2,
                               double* ws, hipStream_t st);
hipError_t launch_quadform_sym_pairs(int n, const double* K_lo, const double* K_hi, long long ld, long long pair_begin,
                                     long long pair_end, const double* q, double* y_or_null, double* ksd2, double* ws,
                                     hipStream_t st);
int quadform_sym_rows_per_strip();
int quadform_sym_min_n();     // below it the symmetric entry point runs the full-matrix kernel, and there are no strip pairs
// matrix-free mat-vec helpers
hipError_t launch_kron_pack(int n, double length_scale, const double* S, const double* q,
                            double* packed /*complex [(n+2)/2, 2^n]*/, double* gate /*[8]*/, hipStream_t st);
hipError_t launch_kron_combine(int n, const double* S, const double* q, const double* packed, double* y,
                               double* partials, double* ksd2, hipStream_t st);
size_t kron_partials(int n);

}  // namespace bornvi
