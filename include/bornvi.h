/*
 * bornvi.h -- C ABI of libbornvi_hip.so, the MI355X (gfx950) backend for the KSD
 * variational-inference hot path of sozoluffy/TensorNetworks.
 *
 * The reference has no FFI: its boundary for this path is the Python API of
 * quantum_born_machine.py / stein_utils.py / ksd_vi_quantum.py.  Each entry point below
 * states which reference lines it replaces; INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions across the boundary;
 *   - return value: 0 (BORNVI_OK) or a negative bornvi_status; text via bornvi_last_error();
 *   - every pointer documented "dev" is device memory owned by the CALLER (PyTorch);
 *     the library never frees it and keeps no reference after the call returns;
 *   - every op is asynchronous on the hipStream_t passed as `stream` (0 = null stream);
 *   - workspace is caller-provided; bornvi_*_workspace_bytes gives the size for the full
 *     batch, a smaller workspace makes the library process the batch in chunks
 *     (it must hold at least one circuit);
 *   - alignment: a pointer needs the alignment of its element type (float64 and int64: 8 bytes,
 *     float32 and int32: 4, complex128: 16) unless its entry point states more, and what an entry
 *     point states it enforces: any other address is refused before any launch.  Where a kernel
 *     reads float64 inputs two at a time (q, y, dLdq, the shifted rows) it uses the device's
 *     unaligned global loads: 8-byte alignment of those pointers is supported, and results do
 *     not depend on where a buffer lies.  A workspace may lie at any 8-byte aligned address (the
 *     library aligns what it carves and the size queries count that) unless its entry point
 *     asks for 16 bytes;
 *   - a handle is bound to one device and is not thread-safe; distinct handles are.
 *   - outcome index i <-> bitstring bin(i).zfill(n): bit position 0 of the tuple is the MOST
 *     significant bit of i and is wire 0 of the circuit (utils.py:77-91).
 *   - accepted n per entry point (anything else is refused with BORNVI_ERR_UNSUPPORTED or
 *     BORNVI_ERR_INVALID before any launch); the BORNVI_* limits are defined below, once, for the
 *     library and for every binding (the Python one reads this file):
 *       circuits, parameter shift (probs, grad, fused dot), adjoint engine,
 *       matrix-free Stein mat-vec ................................. 1 <= n <= BORNVI_CIRCUIT_MAX_N
 *         (plan tile and workgroup indices are 16 bits, tiles at most 2^13 amplitudes;
 *          the 8-amplitude kernel runs n <= 27, the larger states the generic pass kernel);
 *       dense Gram and quadratic forms ............................ 1 <= n <= BORNVI_DENSE_MAX_N;
 *       score from CPTs, k_p pairs, gradient assembly, shots,
 *       ELBO weights, Fisher matrix ............................... 1 <= n <= BORNVI_TABLE_MAX_N;
 *       probability-table Born machine ............................ 0 <= n <= BORNVI_TABLE_MAX_N;
 *       matrix-product-state Born machine
 *         (bond 1 <= D <= BORNVI_MPS_MAX_BOND) .................... 1 <= n <= BORNVI_MPS_MAX_N;
 *       sampled MPS calls, the MPS canonicaliser, log joint and scores of samples,
 *       pairwise Stein kernel row sums (n * length_scale >= 1) ..... 1 <= n <= BORNVI_MPS_SAMPLED_MAX_N;
 *       un-fused gate application ................................. 1 <= n <= BORNVI_GATE_MAX_N.
 */
#ifndef BORNVI_H
#define BORNVI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared in this header are exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BORNVI_VERSION 100 /* 0.1.0 */

/* ---- limits: each accepted range is stated here and nowhere else.  The library's argument checks, the kernels' own
 * bounds and the Python binding (which parses these lines) all use these names.  Plain decimal integers, so that a
 * binding can read them without evaluating C. */
#define BORNVI_CIRCUIT_MAX_N 29               /* circuits, parameter shift, adjoint engine, matrix-free mat-vec: n - 13 <= 16 */
#define BORNVI_DENSE_MAX_N 17                 /* dense Gram and quadratic forms: 8 * 4^n bytes */
#define BORNVI_DENSE_MAX_LD_PAD 4096          /* the `_ld` calls: 2^n <= ld <= 2^n + this, ld even */
#define BORNVI_TABLE_MAX_N 30                 /* everything that walks a table of 2^n entries */
#define BORNVI_GATE_MAX_N 40                  /* un-fused gate application */
#define BORNVI_BN_MAX_NODES 64                /* nodes of a network descriptor: one bit each of a 64-bit word */
#define BORNVI_BORN_TABLE_MAX_ROWS 65535      /* 2^16 - 1: rows of the probability-table Born machine */
#define BORNVI_ELBO_MAX_ROWS 65535            /* 2^16 - 1: rows of bornvi_elbo_weights */
#define BORNVI_REINFORCE_MAX_BATCH 16777216   /* 2^24: samples of bornvi_reinforce_step */
#define BORNVI_SHOTS_MAX 2147483647           /* 2^31 - 1: shots of bornvi_shots_histogram */
#define BORNVI_MPS_MAX_N 26                   /* the enumerated MPS Born machine */
#define BORNVI_MPS_MAX_BOND 32                /* bond dimension D of every MPS call */
#define BORNVI_MPS_SAMPLED_MAX_N 63           /* the sampled MPS calls and the per-sample network calls: an int64 outcome index */
#define BORNVI_MPS_SAMPLED_MAX_BATCH 16777216 /* 2^24: samples per call, and the largest score-row pitch ld */
#define BORNVI_SCORE_MIN_LD 64                /* score-row pitch: a power of two, >= this and >= B */
#define BORNVI_MPS_QUERY_MAX_QUERIES 65536    /* 2^16: evidences per log-marginal call */
#define BORNVI_STEIN_PAIRS_MAX_B 131072       /* 2^17: samples of the pairwise Stein kernel; B^2 is the cost, 1.7e10 pairs here */
#define BORNVI_FISHER_MAX_PARAMS 1024         /* rows of a Fisher / QFI / score Gram block, order of an SPD solve */
#define BORNVI_SAMPLE_GRAM_MAX_BATCH 1024     /* samples of the sample-space Gram: what bornvi_spd_solve factors */
#define BORNVI_SPD_BATCHED_MAX_SYSTEMS 65535  /* 2^16 - 1: systems of bornvi_spd_solve_batched */
#define BORNVI_SCORE_FISHER_MAX_BLOCKS 65535  /* 2^16 - 1: blocks of bornvi_score_fisher_gram */
#define BORNVI_CG_MAX_PARAMS 2147483647       /* 2^31 - 1: vector length of the CG recurrence */
#define BORNVI_CG_STATE_DOUBLES 8             /* doubles of the CG state the caller allocates and the kernels write */

typedef struct bornvi_ctx* bornvi_handle;
typedef void* bornvi_stream; /* hipStream_t */

typedef enum {
  BORNVI_OK = 0,
  BORNVI_ERR_INVALID = -1,     /* bad argument */
  BORNVI_ERR_HIP = -2,         /* a HIP runtime call failed (text has the HIP error) */
  BORNVI_ERR_WORKSPACE = -3,   /* workspace too small for a single circuit */
  BORNVI_ERR_UNSUPPORTED = -4  /* size outside the supported range */
} bornvi_status;

/* ansatz_type strings of QuantumBornMachine (quantum_born_machine.py:31-38, :57-128) */
typedef enum {
  BORNVI_ANSATZ_HARDWARE_EFFICIENT = 0, /* quantum_born_machine.py:58-87  */
  BORNVI_ANSATZ_ALL_TO_ALL = 1,         /* quantum_born_machine.py:90-111 */
  BORNVI_ANSATZ_BASIC = 2               /* quantum_born_machine.py:114-128 */
} bornvi_ansatz;

int bornvi_version(void);

/* One handle per device.  Holds the compiled circuit plans (small device buffers). */
int bornvi_create(int device_ordinal, bornvi_handle* out);
void bornvi_destroy(bornvi_handle h);
/* Text of the last error on this handle (valid until the next call on it). h may be NULL
 * for errors of bornvi_create. */
const char* bornvi_last_error(bornvi_handle h);

/* Tuning knobs of the circuit planner (clears the plan cache): "tile_bits" (4..13, amplitudes per
 * LDS tile = 2^tile_bits, for every n), "tile_bits_multi" (tile size used only when the state needs
 * several tiles; default 0 = chosen per plan: 13 wherever the persistent kernel can run such tiles, else 11), "low_bits" (0..8, contiguous 16-byte elements per HBM run =
 * 2^low_bits), "max_threads" (64..1024).  Engine switches (no effect on results): "fast_path",
 * "fast_workgroups_per_cu", "workgroups_per_cu", "direct_stages", "zero_support" (default 1: the first two passes of a circuit from |0..0> leave out what the support of that state makes
 * known zeros -- tiles nobody reads are not written, slots known to be zero are not loaded), "reg_wires" (default 3: plans with 8 amplitudes per thread for the pass kernel that holds four waves per SIMD, wherever
 * such a plan is eligible; 4: 16 amplitudes per thread, two waves per SIMD -- also the fallback; clears the plan cache),
 * "read_map" (default -1 = by the kernel: the planner may fold phase-0 CNOTs on thread-held wires into a stage's read map --
 * fewer stages, but such a stage needs a barrier between its reads and its write-back: faster with 8 amplitudes per
 * thread, slower with 16; 0 / 1 force it; clears the plan cache), "contig_out" (default 1: the buffer a pass writes keeps that
 * pass's own local wires on its low address bits -- a tile is stored as one contiguous block, the next pass reads runs; 0: both
 * sides move 1-KiB runs; clears the plan cache), "alternate_walk" (default 1: odd passes
 * walk the tiles of the batch from the last to the first, so that a pass starts on the states the previous one wrote last --
 * the ones the memory-side cache still holds), "batched_quadform" (0: bornvi_stein_quadform
 * with B > 1 runs B GEMV passes instead of one matrix-core pass); "grad_engine" (default 0 = the reference's
 * parameter-shift rule; 1 = OPT-IN: bornvi_paramshift_grad answers with adjoint differentiation, see below);
 * "prefix_share" (default 0; 1: in
 * bornvi_paramshift_probs* a shifted circuit starts from the base circuit's state at the first pass
 * its parameter touches instead of |0..0> -- the rows are bit-identical, fewer passes are run). */
int bornvi_set_option(bornvi_handle h, const char* name, long long value);
/* Current value of a planner / engine option: every name bornvi_set_option takes can be read back (one table in the
 * library drives both calls; "workgroups_per_cu" and "max_threads" could be set but not read before that table existed).
 * "reg_wires": 3 = the pass kernel with 8 amplitudes per thread and four waves per SIMD where the plan is eligible,
 * 4 = 16 per thread. */
int bornvi_get_option(bornvi_handle h, const char* name, long long* value);

/* num_ansatz_params (quantum_born_machine.py:31-38) and gate count of the QNode. */
int bornvi_num_params(int ansatz, int n, int layers);
int bornvi_num_gates(int ansatz, int n, int layers);

/* ---- circuit -> Born probabilities (replaces the PennyLane QNode `pqc`, -------------------
 * quantum_born_machine.py:58-128, as called by get_probabilities :132-137).
 * thetas dev [batch, P] float64;  probs dev [batch, 2^n] float64, lexicographic, wire 0 = MSB.
 * workspace: 16-byte aligned (the states are carved from the pointer as given), else
 * BORNVI_ERR_WORKSPACE; the same holds for every bornvi_paramshift_* call below. */
size_t bornvi_circuit_workspace_bytes(bornvi_handle h, int ansatz, int n, int layers, int batch);
int bornvi_circuit_probs(bornvi_handle h, int ansatz, int n, int layers, int batch,
                         const double* thetas, double* probs,
                         void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* ---- parameter-shift evaluations (replaces diff_method="parameter-shift", ------------------
 * quantum_born_machine.py:58,:90,:114, triggered by loss.backward() ksd_vi_quantum.py:150).
 * For p in [p_begin, p_end): circuits theta + pi/2 e_p and theta - pi/2 e_p.
 * probs dev [(include_base ? 1 : 0) + 2 (p_end - p_begin), 2^n]: optional base row first,
 * then rows (+p_begin, -p_begin, +p_begin+1, -p_begin+1, ...).  theta dev [P] float64.
 * The batch for bornvi_circuit_workspace_bytes is that row count. */
int bornvi_paramshift_probs(bornvi_handle h, int ansatz, int n, int layers,
                            const double* theta, int p_begin, int p_end, int include_base,
                            double* probs, void* workspace, size_t workspace_bytes,
                            bornvi_stream stream);
/* The same for the parameters p_begin, p_begin + p_stride, ... (p_count of them): rows (+p_i, -p_i) in that order.
 * One rank of W takes p_begin = rank, p_stride = W: with prefix sharing a parameter of an early layer costs more
 * passes than one of a late layer, and the interleaved deal keeps the ranks level (no reference counterpart: the
 * reference evaluates all shifts in one process). */
int bornvi_paramshift_probs_strided(bornvi_handle h, int ansatz, int n, int layers,
                                    const double* theta, int p_begin, int p_count, int p_stride,
                                    int include_base, double* probs,
                                    void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* grad[p - p_begin] = 1/2 * sum_z dLdq[z] (q(theta + pi/2 e_p)[z] - q(theta - pi/2 e_p)[z]).
 * dLdq dev [2^n], grad dev [p_end - p_begin].  Workspace: the circuit workspace for batch
 * 2 (p_end - p_begin) plus 2 (p_end - p_begin) * 2^n * 8 bytes (bornvi_paramshift_grad_workspace_bytes). */
size_t bornvi_paramshift_grad_workspace_bytes(bornvi_handle h, int ansatz, int n, int layers,
                                              int p_begin, int p_end);
int bornvi_paramshift_grad(bornvi_handle h, int ansatz, int n, int layers,
                           const double* theta, const double* dLdq, int p_begin, int p_end,
                           double* grad, void* workspace, size_t workspace_bytes,
                           bornvi_stream stream);

/* ---- parameter-shift gradient with the dot product FUSED into the last circuit pass (replaces, like
 * bornvi_paramshift_grad, the backward of ksd_vi_quantum.py:150 through diff_method="parameter-shift",
 * quantum_born_machine.py:58): the shifted circuits' probabilities are never written; their last pass accumulates
 * sum_z w_z q(z) per circuit instead (fixed summation order: deterministic).  Two calls around the caller's contraction:
 *   begin : all passes but the last for the base circuit and the 2 p_count shifted ones (parameters p_begin,
 *           p_begin + p_stride, ...), then the base circuit's last pass -> q_out dev [2^n];
 *   (the caller computes y = K_p q, ksd2 = q.y -- any bornvi_stein_* contraction, all-reduced over the ranks)
 *   finish: the shifted circuits' last pass with w = y -> grad dev [p_count]:
 *           grad_p = s * sum_z w_z (q+_p(z) - q-_p(z)),  s = 1/2 if ksd2 == NULL, else 1/2 / sqrt(max(*ksd2, 1e-12)) with the
 *           clamp's zero gradient below 1e-12 (ksd_vi_quantum.py:145); loss_out (or NULL) = sqrt(max(*ksd2, 1e-12)).
 * The SAME workspace (bornvi_paramshift_dot_workspace_bytes, 16-byte aligned) must be passed to both and left alone in
 * between.  Available for multi-pass plans of the 8-amplitude kernel ("reg_wires" = 3) without prefix sharing: the size
 * query returns 0 otherwise (use bornvi_paramshift_probs + bornvi_ksd_grad_finish then). */
size_t bornvi_paramshift_dot_workspace_bytes(bornvi_handle h, int ansatz, int n, int layers, int p_count);
int bornvi_paramshift_dot_begin(bornvi_handle h, int ansatz, int n, int layers, const double* theta, int p_begin,
                                int p_count, int p_stride, double* q_out, void* workspace, size_t workspace_bytes,
                                bornvi_stream stream);
int bornvi_paramshift_dot_finish(bornvi_handle h, int ansatz, int n, int layers, int p_count, const double* w,
                                 const double* ksd2, double* grad, double* loss_out, void* workspace,
                                 size_t workspace_bytes, bornvi_stream stream);

/* ---- un-fused gate application on a batch of statevectors (the gate-apply micro-benchmark of
 * BASELINE.json; one HBM round trip per gate = 32 * 2^n bytes per state).
 * state dev [batch, 2^n] complex128 (re, im interleaved), updated in place.
 * U: HOST pointer to 8 doubles (u00.re, u00.im, u01.re, u01.im, u10.re, ..., u11.im). */
int bornvi_gate1q_apply(bornvi_handle h, int n, long long batch, double* state, int wire,
                        const double* U, bornvi_stream stream);
int bornvi_cnot_apply(bornvi_handle h, int n, long long batch, double* state, int control,
                      int target, bornvi_stream stream);
/* q = |psi|^2 : state dev [batch, 2^n] complex128 -> probs dev [batch, 2^n] float64. */
int bornvi_born_probs(bornvi_handle h, int n, long long batch, const double* state, double* probs,
                      bornvi_stream stream);

/* ---- score function (replaces stein_utils.compute_prob_joint_xz :58-112 and ----------------
 * get_score_function_sp_for_z :115-136 evaluated for all 2^n latent states, i.e.
 * KSDVariationalInference._precompute_all_s_p ksd_vi_quantum.py:70-75, on top of
 * BayesianNetwork.get_joint_probability bayesian_network.py:111-146).
 * All pointers in the descriptor are DEVICE pointers (layout: pack_network() in
 * tensornetworks_amd/bayesian_network.py). */
typedef struct {
  int32_t num_nodes;        /* V <= 64 */
  int32_t max_parents;      /* row length of `parents` (8) */
  const int32_t* role;      /* [V] latent position 0..n-1 | -1 observed=0 | -2 observed=1 | -3 summed out */
  const int32_t* n_parents; /* [V] */
  const int32_t* parents;   /* [V, max_parents] node indices, CPT key order */
  const int32_t* cpt_off;   /* [V] offset in doubles into cpt */
  const double* cpt;        /* table[config][value]; config = parent values, first parent MSB */
} bornvi_bn_desc;
/* S dev [2^n, n] (row z, column b = tuple position b), pxz dev [2^n] or NULL. */
int bornvi_score_from_cpts(bornvi_handle h, const bornvi_bn_desc* bn, int n, double* S,
                           double* pxz, bornvi_stream stream);
/* Log joint of sampled latent states: logp dev [B] float64, logp_b = sum over the nodes, in descriptor order, of
 * log max(CPT_v[parents(z_b, x)][value], p_floor); idx dev [B] int64 outcome indices, 1 <= n <= 63, 1 <= B <= 2^24.  Every
 * FACTOR is floored (the exact-ELBO objective floors the product: at n = 60 legitimate joints lie far below any floor of a
 * product); the two agree whenever no factor is below p_floor and the product is >= p_floor.  A descriptor with a
 * summed-out node (role -3) is refused with BORNVI_ERR_UNSUPPORTED: the roles are read back from the device for that,
 * except while `stream` is being captured, where the kernel writes NaN instead. */
int bornvi_bn_logjoint_samples(bornvi_handle h, const bornvi_bn_desc* bn, int n, long long B, const long long* idx,
                               double p_floor, double* logp, bornvi_stream stream);

/* ---- sampled KSD: no object of size 2^n -------------------------------------------------
 * Stein score of p at sampled states: S dev [B, n] float64,
 *   S[b, i] = 1 - prod_v max(f_v(flip_i z_b), p_floor) / max(f_v(z_b), p_floor),
 * f_v node v's CPT factor, i the tuple position (position 0 = most significant bit of idx), the product over node i and
 * its children only (every other factor cancels).  Every FACTOR is floored, as in bornvi_bn_logjoint_samples and for its
 * reason.  There is NO "|p(x, z)| < 1e-12 -> zero row" rule here (bornvi_score_from_cpts and the reference have one): at
 * n = 60 every legitimate joint lies below 1e-12.  The two agree wherever p(x, z) >= 1e-12 and no factor is below p_floor.
 * logp dev [B] or NULL: when given, bit for bit what bornvi_bn_logjoint_samples writes.  1 <= n <= 63, 1 <= B <= 2^24,
 * else BORNVI_ERR_UNSUPPORTED; a summed-out node is refused as by bornvi_bn_logjoint_samples (NaN while capturing).
 * No allocation, no synchronisation. */
int bornvi_bn_score_samples(bornvi_handle h, const bornvi_bn_desc* bn, int n, long long B, const long long* idx,
                            double p_floor, double* S, double* logp, bornvi_stream stream);

/* Row sums of the pairwise Stein kernel of B samples: r dev [B], r_b = sum_{b' != b} k_p(z_b, z_b' | x), total dev [1] =
 * sum_b r_b; k_p as in bornvi_stein_kp_pairs, idx dev [B] int64, S dev [B, n] the score rows of the samples.  b' != b is
 * by SAMPLE INDEX: a duplicate state z_b' = z_b with b' != b is included with k_p(z, z) (that is what makes
 * total / (B (B - 1)) unbiased for q^T K_p q).  On v_mfma_f64_16x16x4_f64; fixed summation order, no atomics: two calls
 * are bitwise equal; no allocation or synchronisation: capturable.
 * 1 <= n <= 63, 2 <= B <= BORNVI_STEIN_PAIRS_MAX_B, n * length_scale >= 1 (in double), else BORNVI_ERR_UNSUPPORTED,
 * returned before any launch. */
size_t bornvi_stein_pairs_workspace_bytes(bornvi_handle h, int n, long long B);
int bornvi_stein_pairs_rowsum(bornvi_handle h, int n, long long B, double length_scale, const long long* idx,
                              const double* S, double* r, double* total, void* workspace, size_t workspace_bytes,
                              bornvi_stream stream);
/* The geometry the row-sum kernel uses for B samples (a function of B only): 32-column tiles per column range, and the
 * number G of column ranges = partials added per row by the finishing launch.  For error analyses and tests. */
int bornvi_stein_pairs_geometry(long long B, int* tiles_per_range, int* num_ranges);

/* ---- Stein-kernel Gram matrix (replaces the N^2 calls of get_stein_kernel_kp_value, --------
 * stein_utils.py:138-197 with base_hamming_kernel_torch :30-55, made in
 * ksd_vi_quantum.py:125-141).  K dev [2^n, 2^n] float64 row-major, 16-byte aligned (so are K_rows
 * of the two calls below: the kernel stores column pairs, and bornvi_stein_quadform_sym asks the
 * same of the K it reads); anything else is BORNVI_ERR_INVALID before any launch. */
int bornvi_stein_gram_build(bornvi_handle h, int n, double length_scale, const double* S,
                            double* K, bornvi_stream stream);

/* Row block [row_begin, row_end) of K_p, K_rows dev [row_end - row_begin, 2^n]: lets each GPU of a
 * node hold 1/W of the Gram matrix (multi-GPU row shard of the quadratic form). */
int bornvi_stein_gram_build_rows(bornvi_handle h, int n, double length_scale, const double* S,
                                 long long row_begin, long long row_end, double* K_rows,
                                 bornvi_stream stream);

/* Padded row pitch.  K_p with a power-of-two row pitch puts the same column of every row into the same HBM channel and
 * bank, and the symmetric contraction streams 32 rows per wave at the same column; bornvi_stein_gram_ld(n) is the
 * pitch (in doubles, >= 2^n, even) the library recommends: 2^n + 32 for n >= 14, else 2^n (n = 16: 2.56 ms on every
 * allocation against 2.62 ... 2.83 ms dense; 0 for n outside [1, 17]).  The `_ld` entry points take any even pitch in
 * [2^n, 2^n + 4096]; columns >= 2^n of a row are never read or written. */
long long bornvi_stein_gram_ld(int n);
int bornvi_stein_gram_build_rows_ld(bornvi_handle h, int n, double length_scale, const double* S,
                                    long long row_begin, long long row_end, double* K_rows, long long ld,
                                    bornvi_stream stream);

/* k_p(z_i, z_j | x) for M explicit pairs -- the batched form of ONE call of
 * stein_utils.get_stein_kernel_kp_value (:138-197): zi, zj dev int64 [M] outcome indices,
 * si, sj dev [M, n] the score rows sp_at_z1 / sp_at_z2 supplied by the caller, out dev [M]. */
int bornvi_stein_kp_pairs(bornvi_handle h, int n, double length_scale, long long M,
                          const long long* zi, const long long* zj, const double* si,
                          const double* sj, double* out, bornvi_stream stream);

/* ---- quadratic form (replaces the accumulation sum_ij q_i q_j k_p, ksd_vi_quantum.py:123-142).
 * Q dev [B, 2^n]; ksd2 dev [B] = q_b^T K q_b; Y dev [B, 2^n] = K q_b or NULL.
 * Deterministic (no atomics).  Workspace: bornvi_stein_quadform_workspace_bytes. */
size_t bornvi_stein_quadform_workspace_bytes(bornvi_handle h, int n, int B);
int bornvi_stein_quadform(bornvi_handle h, int n, const double* K, const double* Q, int B,
                          double* ksd2, double* Y, void* workspace, size_t workspace_bytes,
                          bornvi_stream stream);
/* The same for a K with row pitch `ld` doubles (bornvi_stein_gram_build_rows_ld; even, 2^n <= ld <= 2^n + 4096): the
 * trainer's padded K_p serves the batched contraction too (no second 32 GiB copy).  With ld > 2^n only the batched
 * matrix-core form exists (n >= 8, B >= 2, option "batched_quadform" = 1), otherwise BORNVI_ERR_UNSUPPORTED; B = 1 on
 * a padded K: bornvi_stein_quadform_sym_ld. */
int bornvi_stein_quadform_ld(bornvi_handle h, int n, const double* K, long long ld, const double* Q, int B,
                             double* ksd2, double* Y, void* workspace, size_t workspace_bytes,
                             bornvi_stream stream);

/* Same result for a SYMMETRIC K (every K from bornvi_stein_gram_build is bitwise symmetric): reads
 * only the upper triangle, i.e. half the HBM traffic of bornvi_stein_quadform; deterministic (column
 * partials in the workspace instead of atomics).  q, y dev [2^n]; ksd2 dev [1].  A dense (unpadded) matrix with
 * n < 14 is handed to the full-matrix kernel: too few 256-row bands to fill the chip, and the matrix is cache-sized
 * (n = 12: 33 us against 93 us); same K q to rounding.  K (K_lo and K_hi of the strip-pair shard) and
 * the workspace: 16-byte aligned, in every bornvi_stein_quadform_sym* call. */
size_t bornvi_stein_quadform_sym_workspace_bytes(bornvi_handle h, int n);
int bornvi_stein_quadform_sym(bornvi_handle h, int n, const double* K, const double* q,
                              double* ksd2, double* y, void* workspace, size_t workspace_bytes,
                              bornvi_stream stream);

/* The same for a K with row pitch `ld` doubles (bornvi_stein_gram_build_rows_ld).  Matrices of fewer than two 256-row
 * bands (n < 9) run the full-matrix kernel, which takes dense rows only: ld > 2^n there is BORNVI_ERR_UNSUPPORTED. */
int bornvi_stein_quadform_sym_ld(bornvi_handle h, int n, const double* K, long long ld, const double* q,
                                 double* ksd2, double* y, void* workspace, size_t workspace_bytes,
                                 bornvi_stream stream);

/* Strip-pair shard of the symmetric form (several GPUs, each reading only its part of the UPPER triangle); n >= 9.
 * The rows are cut into strips ("bands": one workgroup each) of bornvi_stein_sym_strip_rows() = 256 rows; pair p =
 * strips p and n_strips-1-p (a long and a short part of the triangle).  A GPU owning pairs [pair_begin, pair_end) holds K_lo = rows of the strips
 * [pair_begin, pair_end) and K_hi = rows of the strips [n_strips - pair_end, n_strips - pair_begin) (each block
 * built with bornvi_stein_gram_build_rows) and gets y_partial dev [2^n] and ksd2_partial dev [1]: its additive
 * share of K q and of q^T K q; the sum over the GPUs (one all-reduce of 2^n + 1 doubles) is the full result.
 * Workspace as bornvi_stein_quadform_sym. */
int bornvi_stein_sym_strip_rows(void);
int bornvi_stein_quadform_sym_pairs(bornvi_handle h, int n, const double* K_lo, const double* K_hi,
                                    long long pair_begin, long long pair_end, const double* q,
                                    double* ksd2_partial, double* y_partial, void* workspace,
                                    size_t workspace_bytes, bornvi_stream stream);

int bornvi_stein_quadform_sym_pairs_ld(bornvi_handle h, int n, const double* K_lo, const double* K_hi, long long ld,
                                       long long pair_begin, long long pair_end, const double* q,
                                       double* ksd2_partial, double* y_partial, void* workspace,
                                       size_t workspace_bytes, bornvi_stream stream);

/* Row-sharded form: K_rows holds rows [row_begin, row_end); q dev [2^n] (full);
 * y_rows dev [row_end - row_begin] = those rows of K q (or NULL); ksd2_partial dev [1] =
 * sum over them of q_i y_i.  Workspace as bornvi_stein_quadform. */
int bornvi_stein_quadform_rows(bornvi_handle h, int n, const double* K_rows, long long row_begin,
                               long long row_end, const double* q, double* y_rows,
                               double* ksd2_partial, void* workspace, size_t workspace_bytes,
                               bornvi_stream stream);

/* Matrix-free y = K_p q via the Kronecker structure of K_p (needed where the dense Gram does
 * not fit: n = 20 would be 8 TiB).  q, y dev [2^n]; ksd2 dev [1].  workspace: 16-byte aligned (the
 * circuit engine's states are carved from the pointer as given), else BORNVI_ERR_WORKSPACE. */
size_t bornvi_stein_matvec_kron_workspace_bytes(bornvi_handle h, int n);
int bornvi_stein_matvec_kron(bornvi_handle h, int n, double length_scale, const double* S,
                             const double* q, double* y, double* ksd2, void* workspace,
                             size_t workspace_bytes, bornvi_stream stream);

/* ---- loss and gradient assembly (replaces ksd_vi_quantum.py:144-145 and the autograd chain
 * of :150): loss = sqrt(max(ksd2, 1e-12)); dLdq = y / loss (0 when the clamp is active);
 * grad[p] = 1/2 dLdq . (q+_p - q-_p).
 * shifted dev [2 * n_shift, 2^n] rows (+p, -p) as bornvi_paramshift_probs lays them out;
 * y dev [2^n]; ksd2 dev [1]; loss_out dev [1]; dLdq_out dev [2^n] or NULL; grad dev [n_shift]. */
int bornvi_ksd_grad_finish(bornvi_handle h, int n, const double* shifted, int n_shift,
                           const double* y, const double* ksd2, double* loss_out,
                           double* dLdq_out, double* grad, bornvi_stream stream);

/* ---- finite-shot measurement (qml.probs under shots = S): freq dev [B, 2^n] = counts / S of S independent draws from
 * each row of probs dev [B, 2^n] (exact multinomial sampling; every entry an exact count / S, rows sum to S / S).
 * freq == probs (in place) is allowed, any other overlap is not.  Row r is circuit id 0 (the base circuit) if
 * include_base and r == 0, else, with j = r - include_base and p = p_begin + (j / 2) p_stride, id 2p + 1 (+ shift) or
 * 2p + 2 (- shift) for even / odd j: the row layout of bornvi_paramshift_probs_strided.  The draws are a pure function
 * of (seed, *epoch_dev, id, draw index) through Philox4x32-10 (kernels_shots.hip states the exact function), so they do
 * not depend on how the rows are batched or sharded.  epoch_dev: int64 in device memory, read by the kernels (a graph
 * replay sees the value current at replay time; its low 32 bits enter the counter).  A probability-0 entry is never
 * drawn (the pick rule tests the entry's value, not only its cdf: csrc/shots_dev.hpp), so every row with a positive
 * entry sums to exactly S; a row of zeros yields zeros.  1 <= shots <= 2^31 - 1.  Workspace: bornvi_shots_workspace_bytes(h, n, B). */
size_t bornvi_shots_workspace_bytes(bornvi_handle h, int n, int B);
int bornvi_shots_histogram(bornvi_handle h, int n, int B, const double* probs, double* freq, long long shots,
                           unsigned long long seed, const long long* epoch_dev, int include_base, int p_begin,
                           int p_stride, void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* ---- classical Born machine, probability-table family (replaces get_probabilities / entropy of
 * born_machine_classical_sim.py:74-99, :177-181 and the autograd chain of ksd_vi.py:112-145 down to the table or the
 * logits of the conditional network).  w dev [rows, 2^n] float32 raw parameters; mode 0 (use_logits):
 * q = softmax(w - max w), mode 1: q = |w| / sum |w|.  q32 dev [rows, 2^n] float32 = what get_probabilities returns,
 * q64 dev [rows, 2^n] float64 = its exact upcast (the KSD is computed on q32.to(float64)); entropy dev [rows] float32 or
 * NULL = -sum q log max(q, 1e-10) over q32.  0 <= n <= 30, 1 <= rows <= 65535.  Row reductions are fixed-order partials
 * in the workspace (no atomics: bitwise reproducible); no allocation or synchronisation (capturable).  Workspace:
 * bornvi_born_table_workspace_bytes(h, n, rows), valid for both calls. */
size_t bornvi_born_table_workspace_bytes(bornvi_handle h, int n, int rows);
int bornvi_born_table_probs(bornvi_handle h, int n, int rows, int mode, const float* w, float* q32, double* q64,
                            float* entropy, void* workspace, size_t workspace_bytes, bornvi_stream stream);
/* grad dev [rows, 2^n] float32 (may be a parameter's .grad) = d/dw of  sqrt(max(ksd2, 1e-12)) - entropy_weight * H  per
 * row, as torch autograd computes it through the reference's graph: dL/dq = float32(y / loss) (0 while the clamp is
 * active) + entropy_weight (log max(q, 1e-10) + [q >= 1e-10]); softmax VJP q (g - sum q g); mode 1
 * sign(w) (g - sum q g) / sum |w| (sign(0) = 0).  q64 as returned by bornvi_born_table_probs; y dev [rows, 2^n]
 * = K_p q (bornvi_stein_quadform_sym / _matvec_kron) or NULL (no KSD term); ksd2 dev [rows] = q^T K_p q, or NULL with y
 * given: y is then dL/dq itself; entropy_weight = 0: no entropy term.  loss_out dev [rows] or NULL
 * = sqrt(max(ksd2, 1e-12)) (needs ksd2). */
int bornvi_born_table_vjp(bornvi_handle h, int n, int rows, int mode, const float* w, const double* q64,
                          const double* y, const double* ksd2, double entropy_weight, float* grad,
                          double* loss_out, void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* ---- classical Born machine, REINFORCE step of the adversarial (KL) trainer (replaces adversarial_vi.py:200-222 for
 * one observation: raw reward, running baseline, log q of the samples, the loss with its entropy bonus, and the part of
 * loss_q.backward() from the loss down to q, whose index-gather gradient is a scatter-add over the samples).
 * idx dev [B] int64 sampled outcome indices; logit dev [B] float32 classifier logits of the samples; log_p dev [2^n]
 * float32 = log p(x_obs | z) (may hold +-inf); q32 dev [2^n] float32 = the Born machine's probabilities.
 *   raw_b = logit_b - log_p[idx_b];  mean = (1/B) sum raw_b;  baseline (dev [1] float64, in/out) = mean if first, else
 *   baseline_decay * baseline + (1 - baseline_decay) * mean;  w_b = raw_b - baseline + entropy_coef;
 *   loss dev [1] float32 = (1/B) sum_b log max(q32[idx_b], q_floor) * w_b;
 *   dLdq dev [2^n] float64 = [q32[i] >= q_floor] * (sum of w_b over idx_b = i) / (B * q32[i]), 0 where no sample fell:
 * the y of bornvi_born_table_vjp(..., ksd2 = NULL).  found_inf dev [1] float32 = 1 if the loss is NaN or +-Inf (then
 * loss = NaN and dLdq = 0), else 0: the flag torch's fused optimisers consume.  The per-outcome sums are 64-bit
 * fixed-point integer sums (kernels_reinforce.hip states the scale and its error bound) and the means fixed-order
 * partials in the workspace: bitwise reproducible.  An index outside [0, 2^n) is not dereferenced and counts as a sample
 * of reward 0 on no outcome.  1 <= n <= 30, 1 <= B <= 2^24.  No allocation or synchronisation (capturable). */
size_t bornvi_reinforce_workspace_bytes(bornvi_handle h, int n, long long B);
int bornvi_reinforce_step(bornvi_handle h, int n, long long B, const long long* idx, const float* logit,
                          const float* log_p, const float* q32, double* baseline, int first, double baseline_decay,
                          double entropy_coef, double q_floor, double* dLdq, float* loss, float* found_inf,
                          void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* ---- exact ELBO / reverse KL of a Born distribution (no reference counterpart: the reference estimates this quantity
 * through a classifier and REINFORCE, adversarial_vi.py:200-222).  With the log-joint of one observation tabulated,
 *   L = sum_z q_z (log q_z - log p(x, z)) = KL(q || p(.|x)) - log p(x)
 * is exact in O(2^n).  q dev [rows, 2^n] float64; log_p dev [2^n] float64, finite, shared by all rows.  Per row, with
 * l_z = log max(q_z, q_floor):
 *   w dev [rows, 2^n] or NULL:  w_z = l_z - log_p_z + [q_z >= q_floor] = dL/dq_z -- the derivative of q log max(q, floor),
 *     the convention of bornvi_born_table_vjp's entropy term; the weight vector of bornvi_paramshift_dot_finish
 *     (ksd2 = NULL), the dLdq of bornvi_adjoint_vjp and the y of bornvi_born_table_vjp (ksd2 = NULL);
 *   neg_elbo dev [rows] = sum_z q_z (l_z - log_p_z), a term with q_z == 0 being exactly 0;
 *   entropy dev [rows] or NULL = -sum_z q_z l_z.
 * A non-finite log_p entry is not refused: it reaches neg_elbo (unless its q_z is 0), where the optimiser hand-off's
 * guard (bornvi_clip_cast_grad_guard, bornvi_clip_adam_step) skips the update.  The sums are fixed-order partials in the
 * workspace (no atomics: bitwise reproducible); no allocation or synchronisation (capturable).  1 <= n <= 30,
 * 1 <= rows <= 65535, q_floor > 0.  Workspace: bornvi_elbo_workspace_bytes(h, n, rows). */
size_t bornvi_elbo_workspace_bytes(bornvi_handle h, int n, int rows);
int bornvi_elbo_weights(bornvi_handle h, int n, int rows, const double* q, const double* log_p,
                        double q_floor, double* w, double* neg_elbo, double* entropy,
                        void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* ---- matrix-product-state (tensor-train) Born machine (no reference counterpart: the reference's classical family is the
 * 2^n-entry table of born_machine_classical_sim.py; these two calls take its place in a training step, the first that of
 * bornvi_born_table_probs and the second that of bornvi_born_table_vjp with ksd2 = NULL).
 *   psi(z) = e0^T A_1[z_1] A_2[z_2] ... A_n[z_n] e0,   Z = sum_z psi(z)^2,   q_z = psi(z)^2 / Z.
 * cores dev [n, 2, D, D] float64 row-major: A_k[s][a][b], a the left bond, b the right bond, s the value of tuple position
 * k - 1 (position 0 = the most significant bit of the outcome index).  Both boundary vectors are e0: only row 0 of site 1
 * and column 0 of site n enter.  No rescaling between levels.
 * bornvi_mps_probs: q64 dev [2^n] float64; q32 dev [2^n] float32 or NULL = float32(q64); psi dev [2^n] float64 or NULL;
 * Z_out dev [1] float64.  If Z is 0 or not finite, every q is NaN (no error code: the trainers' NaN/Inf guard skips the
 * step).  The call leaves in the workspace what bornvi_mps_vjp needs (the levels of the prefix-doubling sweep, psi, Z): the
 * same workspace goes to both calls and is left alone in between, the convention of bornvi_paramshift_dot_begin/_finish.
 * bornvi_mps_vjp: g dev [2^n] float64 = dL/dq; grad_cores dev [n, 2, D, D] float64 = dL/dcores, same cores as the probs
 * call; the entries of the first and last core that do not enter psi get exactly 0.0.
 * Z, sum q g and the sums over prefixes of the core gradients are fixed-order partials in the workspace plus a finishing
 * step (no atomics: two calls are bitwise equal); no allocation or synchronisation (capturable).  1 <= n <= 26 and
 * 1 <= D <= 32, anything else is BORNVI_ERR_UNSUPPORTED before any launch.  Workspace: bornvi_mps_workspace_bytes(h, n, D)
 * (about 14 D 2^n bytes: the levels are stored, not recomputed). */
size_t bornvi_mps_workspace_bytes(bornvi_handle h, int n, int D);
int bornvi_mps_probs(bornvi_handle h, int n, int D, const double* cores, double* q64, float* q32, double* psi,
                     double* Z_out, void* workspace, size_t workspace_bytes, bornvi_stream stream);
int bornvi_mps_vjp(bornvi_handle h, int n, int D, const double* cores, const double* g, double* grad_cores,
                   void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* ---- sampled MPS Born machine (kernels_mps_sample.hip): no 2^n object anywhere -----------------
 * Same cores layout and conventions as above; 1 <= n <= 63, 1 <= D <= 32, 1 <= B <= 2^24 samples per call, anything else is
 * BORNVI_ERR_UNSUPPORTED before any launch.  A sample is one int64 outcome index, idx = sum_k z_k 2^(n-k) (tuple position 0 =
 * the most significant bit).
 * bornvi_mps_environments: the right environments E_n = e0 e0^T, E_{k-1} = sum_s A_k[s] E_k A_k[s]^T, the left ones
 * L_0 = e0 e0^T, L_k = sum_s A_k[s]^T L_{k-1} A_k[s], each rescaled by an exact power of two after every step with its
 * integer exponent kept beside it, and log Z (Z = E_0[0,0]) -> log_Z_out dev [1] or NULL.  They stay in the workspace: the
 * two calls below need them for the same cores and the same (n, D, B) workspace (the begin/finish convention of
 * bornvi_paramshift_dot_begin/_finish).
 * bornvi_mps_sample: B exact ancestral draws z ~ q -> idx dev [B] int64, logq dev [B] float64 = log psi(z)^2 - log Z.  Draw
 * k of sample b is a pure function of (seed, *epoch_dev, b, k) through Philox4x32-10 (the kernel file states it): it does
 * not depend on B.  status dev [1] int32: 0, or 1 when some sample met conditional masses whose sum is 0 or not finite
 * (its remaining bits are 0 and its logq NaN).
 * bornvi_mps_score_vjp: idx dev [B], w dev [B] float64 -> logq dev [B] and grad_cores dev [n, 2, D, D] = sum_b w_b grad
 * log q(z_b); the entries of the first and last core that do not enter psi get exactly 0.0.  status: 0, or 2 when some
 * psi(z_b) is 0 or not finite (logq -inf / NaN, no contribution to the sample term) or Z is not positive and finite.
 * No atomics (two calls are bitwise equal), no allocation or synchronisation (capturable).  The workspace is bounded in B:
 * at most 256 tiles of 64 samples are in flight (bornvi_mps_sample_workspace_bytes). */
size_t bornvi_mps_sample_workspace_bytes(bornvi_handle h, int n, int D, long long B);
int bornvi_mps_environments(bornvi_handle h, int n, int D, long long B, const double* cores, double* log_Z_out,
                            void* workspace, size_t workspace_bytes, bornvi_stream stream);
int bornvi_mps_sample(bornvi_handle h, int n, int D, long long B, const double* cores, unsigned long long seed,
                      const long long* epoch_dev, long long* idx, double* logq, int* status, void* workspace,
                      size_t workspace_bytes, bornvi_stream stream);
int bornvi_mps_score_vjp(bornvi_handle h, int n, int D, long long B, const double* cores, const long long* idx,
                         const double* w, double* logq, double* grad_cores, int* status, void* workspace,
                         size_t workspace_bytes, bornvi_stream stream);

/* ---- natural gradient (no reference counterpart: the reference steps theta with Adam on the raw gradient).
 * bornvi_fisher_gram: the classical Fisher information matrix of the Born distribution from the stored parameter-shift
 * rows.  shifted dev [2 n_shift, 2^n] float64, rows (+p, -p) as bornvi_paramshift_probs lays them out; q dev [2^n]; both
 * 16-byte aligned.  F dev [n_shift, n_shift] row-major:
 *   F_ab = sum_z d_a(z) d_b(z) r_z,  d_a = 1/2 (row_{2a} - row_{2a+1}),  r_z = 1 / q_z where q_z >= q_floor, else 0
 * (the library's floor convention: a state under the floor contributes nothing).  A split-K SYRK on the fp64 matrix
 * cores; slab partials go to the workspace and a finishing launch adds them in a fixed order (no atomics: two calls are
 * bitwise equal); only tiles on or above the diagonal are computed and the lower triangle is the bitwise mirror
 * (F == F^T exactly).  No allocation or synchronisation (capturable).  1 <= n <= 30, 1 <= n_shift <= 1024, q_floor > 0.
 * Workspace: bornvi_fisher_workspace_bytes(h, n, n_shift). */
size_t bornvi_fisher_workspace_bytes(bornvi_handle h, int n, int n_shift);
int bornvi_fisher_gram(bornvi_handle h, int n, const double* shifted, int n_shift, const double* q,
                       double q_floor, double* F, void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* bornvi_spd_solve: (A + damping I) x = b by Cholesky, one launch of one workgroup, fixed operation order (bitwise
 * reproducible), no allocation or synchronisation (capturable).  A dev [P, P] symmetric: its upper triangle is read and A
 * is left untouched (the factor lives in the workspace); b, x dev [P]; info dev [1] int32: 0 on success.  If pivot k
 * (counted from 0) is non-positive or non-finite, info = k + 1; if b holds a non-finite entry, info = P + 1 (tested
 * first); if the solution is not finite, info = P + 2; in each of these cases x = b bit for bit, so that a caller which
 * steps along x falls back to the plain gradient: nothing non-finite is written into x on behalf of the factorisation.
 * 1 <= P <= 1024, damping >= 0.  Workspace: bornvi_spd_solve_workspace_bytes(h, P). */
size_t bornvi_spd_solve_workspace_bytes(bornvi_handle h, int P);
int bornvi_spd_solve(bornvi_handle h, int P, const double* A, double damping, const double* b, double* x, int* info,
                     void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* bornvi_spd_solve_batched: nb independent systems (A[j] + damping I) x[j] = b[j], one workgroup per system in one launch.
 * A dev [nb, P, P], b, x dev [nb, P], info dev [nb] int32.  System j has the operation order, the info codes and the
 * "x = b where info != 0" rule of bornvi_spd_solve: it equals that call on (A[j], b[j]) bit for bit.  1 <= P <= 1024,
 * 1 <= nb <= 65535 (else BORNVI_ERR_UNSUPPORTED before any launch), damping >= 0.  No allocation or synchronisation
 * (capturable).  Workspace: bornvi_spd_solve_batched_workspace_bytes(h, P, nb) (nb factors of P x P). */
size_t bornvi_spd_solve_batched_workspace_bytes(bornvi_handle h, int P, int nb);
int bornvi_spd_solve_batched(bornvi_handle h, int P, int nb, const double* A, double damping, const double* b, double* x,
                             int* info, void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* ---- natural gradient of the sampled MPS Born machine: the sampled Fisher estimate is a Gram of
 * per-sample score rows (stochastic reconfiguration).
 * bornvi_mps_score_rows, after bornvi_mps_environments on the same (n, D, B) workspace: for the sites k_begin ..
 * k_begin + k_count - 1 (counted from 0: site j uses cores[j]) and the samples idx dev [B],
 *   rows[j - k_begin][(s D + a) D + c][b] = 2 [z_b,j = s] l_b[a] r_b[c] / psi_b - mu[j][s][a][c],  mu = 2 (L A_j[s] E)[a][c] / Z
 * (l_b the left vector of sample b in front of site j, r_b the right vector behind it, L and E the environments there): the
 * centred score of sample b with respect to cores[j][s][a][c]; mu is the exact mean of the first term under q.
 * rows dev [k_count, 2 D^2, ld] float64, 16-byte aligned; ld a power of two, >= 64 and >= B (what bornvi_score_fisher_gram
 * takes); the columns B .. ld - 1 are written as 0.0.  A sample with psi = 0 or not finite gets an all-zero column and
 * status (dev [1] int32) becomes 2, else 0.  Sites outside the range are swept and not written, so the caller bounds
 * the buffer.  2 <= B <= 2^24, 1 <= n <= 63, 1 <= D <= 32, else BORNVI_ERR_UNSUPPORTED before any launch.  No atomics, no
 * allocation or synchronisation (capturable); two calls are bitwise equal, and a sub-range equals the same slice of a
 * whole call bit for bit.  mu lives in a region of its own at the end of the (n, D, B) workspace:
 * bornvi_mps_sample_workspace_bytes counts it (16 n D^2 bytes more than before, for every caller).
 * bornvi_score_fisher_gram: F[j] = (1 / B) X_j X_j^T for nblocks consecutive blocks X_j of R rows x ld columns of `rows`
 * (site blocks: R = 2 D^2, nblocks = sites; the whole matrix: R = 2 n D^2, nblocks = 1, over the same buffer).
 * F dev [nblocks, R, R] float64.  The split-K SYRK of bornvi_fisher_gram on the fp64 matrix cores with a plain row source;
 * slab partials go to the workspace, a finishing launch adds them in index order, divides by B once and writes F_ab and
 * F_ba from one value (F == F^T bitwise; no atomics: two calls are bitwise equal).  An entry's order of summation depends
 * on ld only: a site block equals the diagonal block of the whole matrix bit for bit.  1 <= R <= 1024, 1 <= nblocks <=
 * 65535, 2 <= B <= ld, else BORNVI_ERR_UNSUPPORTED before any launch.  Workspace:
 * bornvi_score_fisher_workspace_bytes(h, R, nblocks, ld). */
int bornvi_mps_score_rows(bornvi_handle h, int n, int D, long long B, const double* cores, const long long* idx,
                          int k_begin, int k_count, long long ld, double* rows, int* status, void* workspace,
                          size_t workspace_bytes, bornvi_stream stream);
size_t bornvi_score_fisher_workspace_bytes(bornvi_handle h, int R, int nblocks, long long ld);
int bornvi_score_fisher_gram(bornvi_handle h, int R, int nblocks, long long B, long long ld, const double* rows, double* F,
                             void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* ---- the same natural gradient solved in sample space.  With O the B x P matrix of the centred
 * score rows, (O^T O / B + damping I)^-1 O^T w = O^T u with (T + damping I) u = w, T = O O^T / B: a B x B system whatever P is.
 * bornvi_mps_score_sample_gram, after bornvi_mps_environments on env_workspace (the (n, D, B) workspace of
 * bornvi_mps_sample_workspace_bytes), writes T dev [B, B] float64 for the samples idx dev [B] without forming a row:
 *   B T_bb' = sum_k [z_bk = z_b'k] (x_bk . x_b'k)(r_bk . r_b'k) - m_b - m_b' + M,
 *   x_bk = (2 / psi_b) l_b,k-1,  m_b = sum_k x_bk^T mu_k[z_bk] r_bk,  M = sum_k,s ||mu_k[s]||_F^2,
 * the dot products on the fp64 matrix cores, the sites added in order.  T == T^T bitwise, two calls are bitwise equal, and
 * an entry's bits depend on (n, D, cores, the two samples) and B's one division only: not on the tile or the grid.  A sample
 * with psi = 0 or not finite gets a row and a column of exactly 0.0 and status (dev [1] int32) becomes 2, else 0.
 * 2 <= B <= 1024 (what bornvi_spd_solve factors), 1 <= n <= 63, 1 <= D <= 32; anything else, a short workspace included,
 * is BORNVI_ERR_UNSUPPORTED before any launch.  It rewrites the mu region of env_workspace (as bornvi_mps_score_rows does) and
 * keeps its vectors in `workspace`: bornvi_mps_score_sample_gram_workspace_bytes(h, n, D, B).  No atomics, no allocation
 * or synchronisation (capturable). */
size_t bornvi_mps_score_sample_gram_workspace_bytes(bornvi_handle h, int n, int D, long long B);
int bornvi_mps_score_sample_gram(bornvi_handle h, int n, int D, long long B, const double* cores, const long long* idx, double* T,
                                 int* status, void* env_workspace, size_t env_workspace_bytes, void* workspace,
                                 size_t workspace_bytes, bornvi_stream stream);

/* ---- the same natural gradient without any matrix: conjugate gradients on
 * (O^T O / B + damping I) delta = g, one product v -> O^T (O v) / B per iteration.  O^T w is bornvi_mps_score_vjp.
 * bornvi_mps_score_jvp, after bornvi_mps_environments on env_workspace (the (n, D, B) workspace of
 * bornvi_mps_sample_workspace_bytes), writes O v scaled: for the samples idx dev [B] and a direction v dev [n, 2, D, D]
 * float64 (the cores' layout),
 *   t_b = scale <grad log q(z_b), v> = scale (2 dpsi_b / psi_b - sum_k <mu_k, V_k>),  dpsi_b = sum_k l_b,k-1^T V_k[z_bk] r_b,k,
 * t dev [B] float64; mu as in bornvi_mps_score_rows.  One left-to-right sweep of (l, dl), dl <- dl A_k[z] + l V_k[z], both
 * rescaled by the same power of two after every site; <mu_k, V_k> is added in index order per site, then the sites in
 * order.  t_b's bits depend on (cores, v, scale, the sample) only: not on B, the grid or the tile; two calls are bitwise
 * equal.  A sample with psi = 0 or not finite gets t_b = 0.0 and status (dev [1] int32) becomes 2, else 0.  2 <= B <= 2^24,
 * 1 <= n <= 63, 1 <= D <= 32; anything else, a short workspace included, is BORNVI_ERR_UNSUPPORTED before any launch; scale
 * must be finite.  It rewrites the mu region of env_workspace (as bornvi_mps_score_rows does) and the per-workgroup weight
 * sums bornvi_mps_score_vjp keeps there between its own two launches.  No atomics, no allocation or synchronisation
 * (capturable). */
int bornvi_mps_score_jvp(bornvi_handle h, int n, int D, long long B, const double* cores, const long long* idx, const double* v,
                         double scale, double* t, int* status, void* env_workspace, size_t env_workspace_bytes,
                         bornvi_stream stream);

/* ---- exact posterior queries of the sampled MPS (kernels_mps_query.hip): what q says about parts
 * of z, from its environments in O(n D^3) per query; cores, n and D as in the sampled section above.
 * An evidence is a pair of int64 words (mask, value): a set mask bit clamps that site (tuple position p = bit n - 1 - p) to
 * the value's bit; value bits outside the mask are ignored; bits at or above n must be 0 in both words (the kernels never
 * look at them).  The clamped environments E^(j)_{k-1} = sum_{s allowed at k} A_k[s] E^(j)_k A_k[s]^T run the step of
 * bornvi_mps_environments (same fma chains, same power-of-two rescale and exponent), a disallowed s contributing no term.
 * bornvi_mps_log_marginals: Q evidences mask, value dev [Q] -> logm dev [Q] float64, the log probability of each partial
 * assignment.  One workgroup per query and one for the empty mask, the normaliser:
 *   logm_j = (log E^^(j)_0[0,0] - log E^_0[0,0]) + (e_j - e) ln 2,
 * so an empty evidence gives exactly 0.0 and one with all n sites clamped log q of that state.  Evidence of probability
 * zero gives -inf, an environment that is not finite NaN; either sets status (dev [1] int32) to 1, else 0.  1 <= Q <= 2^16.
 * bornvi_mps_sample_clamped: B exact draws from q(. | evidence), mask and value dev [1] (read by the kernels: capturable).
 * idx dev [B]; logq dev [B] = log q(z | evidence) (exactly 0.0 when all n sites are clamped: set, not computed); logm dev [1] = the evidence's log
 * marginal.  The sampler is bornvi_mps_sample's against the clamped environments: a free site decides as there, from the
 * same uniform (the Philox counter does not depend on the mask); a clamped site takes the evidence's bit.  A sample whose
 * chosen branch has a conditional mass that is not positive and finite is dead: status 1, logq NaN, its clamped positions
 * keep the evidence's bits and its free positions from there on are 0.  With an empty mask idx and logq are bitwise those
 * of bornvi_mps_environments + bornvi_mps_sample at the same (cores, seed, epoch).  Draws do not depend on B.
 * bornvi_mps_marginals: m1 dev [n], m1[i] = q(z_i = 1), and, where m2 is not NULL, m2 dev [n, n], m2[i][j] = q(z_i = 1,
 * z_j = 1).  It runs both unclamped sweeps itself, into its own workspace (no call of bornvi_mps_environments is needed
 * and none is disturbed), then one workgroup per site i:  m1[i] = <L_{i-1}, A_i[1] E_i A_i[1]^T> / Z, and
 * M = A_i[1]^T L_{i-1} A_i[1] carried through j = i + 1 .. n with m2[i][j] = <M, A_j[1] E_j A_j[1]^T> / Z, M rescaled by exact
 * powers of two.  The lower triangle is a copy of the upper and the diagonal is m1: m2 == m2^T bitwise.
 * All three: anything outside the ranges, a short workspace included, is BORNVI_ERR_UNSUPPORTED before any launch; no
 * atomics (two calls are bitwise equal), no allocation or synchronisation (capturable).  Workspace:
 * bornvi_mps_query_workspace_bytes(h, n, D, Q), with Q = 1 for the sampler and the marginals. */
size_t bornvi_mps_query_workspace_bytes(bornvi_handle h, int n, int D, int Q);
int bornvi_mps_log_marginals(bornvi_handle h, int n, int D, int Q, const double* cores, const long long* mask,
                             const long long* value, double* logm, int* status, void* workspace, size_t workspace_bytes,
                             bornvi_stream stream);
int bornvi_mps_sample_clamped(bornvi_handle h, int n, int D, long long B, const double* cores, const long long* mask,
                              const long long* value, unsigned long long seed, const long long* epoch_dev, long long* idx,
                              double* logq, double* logm, int* status, void* workspace, size_t workspace_bytes,
                              bornvi_stream stream);
int bornvi_mps_marginals(bornvi_handle h, int n, int D, const double* cores, double* m1, double* m2, void* workspace,
                         size_t workspace_bytes, bornvi_stream stream);

/* ---- canonical form, bond spectra and truncation (kernels_mps_canon.hip); cores, n and D as in the
 * sampled section above.  bornvi_mps_canonicalise brings the MPS to canonical form with two orthogonalising sweeps of one
 * workgroup and reads the Schmidt values at every bond on the way back:
 *   left, k = 1 .. n - 1:  [C A_k[0]; C A_k[1]] = Q (S V^T) (one-sided Jacobi), A_k <- the blocks of Q, C <- S V^T over its
 *     Frobenius norm, whose log is accumulated (C_0 = e0 e0^T);
 *   right, k = n .. 2:  [A_k[0] R, A_k[1] R] = U S W, the values of S (sorted descending, ties by index, over their norm) are
 *     the Schmidt values of bond k - 1; the D_out largest stay, then more go from the small end for as long as the dropped
 *     squares sum to <= cutoff, at least one stays; A_k <- the kept rows of W's blocks, R <- U S on the kept values over its
 *     Frobenius norm (R_n = e0 e0^T); at last R goes into site 1.
 * cores_out dev [n, 2, D_out, D_out]: psi_out = +psi_in / sqrt(Z) when nothing is cut, sites 2 .. n right-canonical (sum_s
 * A_k[s] A_k[s]^T = I on the kept block), its own Z is 1; rows >= 1 of the first core, columns >= 1 of the last and
 * everything outside the kept blocks are exactly 0.0.  schmidt dev [n - 1, D]: all D values of every bond, descending,
 * sum of squares 1, a value the rank rule found null exactly 0.0.  discarded dev [n - 1]: the sum of the dropped squares.
 * rank dev [n - 1] int32: the values kept.  log_norm dev [1] = log Z of the INPUT cores.  status dev [1] int32: 1 when
 * the input held a non-finite entry or Z is not positive and finite (cores_out and log_norm are NaN), 4 when a
 * factorisation used all 30 sweeps without converging (outputs as computed), else 0.  With n = 1 there are no bonds
 * (schmidt, discarded and rank may be NULL) and the one core is normalised.
 * The rank rule: a column pair is skipped when either squared norm is <= (D 2^-52)^2 times the largest squared column
 * norm of the matrix under factorisation, and such a column's singular value is exactly 0.0.
 * 1 <= n <= 63, 1 <= D <= 32, 1 <= D_out <= D, cutoff finite and >= 0: anything else, a short workspace included, is
 * BORNVI_ERR_UNSUPPORTED before any launch.  No atomics (two calls are bitwise equal), no allocation or synchronisation
 * (capturable).  The first int of the aligned workspace holds the largest sweep count of the call's factorisations. */
size_t bornvi_mps_canon_workspace_bytes(bornvi_handle h, int n, int D);
int bornvi_mps_canonicalise(bornvi_handle h, int n, int D, int D_out, double cutoff, const double* cores, double* cores_out,
                            double* schmidt, double* discarded, int* rank, double* log_norm, int* status, void* workspace,
                            size_t workspace_bytes, bornvi_stream stream);

/* ---- amortised inference: draws from the network, and the gradient of log-marginals.
 * bornvi_bn_sample: B exact ancestral draws from the network itself.  role[v] is the tuple position 0 .. n - 1 of node v in
 * the output word (each position taken once) or -3: such a node is drawn, because its children need it, and dropped.
 * Observed roles (-1, -2) and a node listed before one of its parents (a parent index not below the node's own) are
 * BORNVI_ERR_UNSUPPORTED: role, n_parents and parents are read back from the device for that, except while `stream` is being
 * captured, where the kernel writes NaN to logp and 1 to status instead.  Node v of sample b takes
 *   bit = U (t0 + t1) >= t0,  t_s = CPT_v[parents][s] as stored
 * (a value of probability 0 is never drawn), U the 53-bit uniform of Philox4x32-10 with counter (b, v >> 1, 0xfffffffe,
 * *epoch_dev) and key seed, even v the words (x, y), odd v (z, w): a sample depends on (network, seed, epoch, b) only, not on
 * B.  idx dev [B] int64: the kept nodes' bits, tuple position p at bit n - 1 - p.  logp dev [B] float64: the sum over all V
 * nodes, in descriptor order, of log of the chosen factor, unfloored; with no dropped node and every factor >= p_floor it is
 * bit for bit what bornvi_bn_logjoint_samples writes for idx.  status dev [1] int32: 0, or 1 when some sample met a row whose
 * t0 + t1 is not positive and finite (its logp is NaN, its remaining bits 0).  1 <= n <= 63, 1 <= B <= 2^24, else
 * BORNVI_ERR_UNSUPPORTED before any launch.  No allocation, no synchronisation outside the descriptor check: capturable. */
int bornvi_bn_sample(bornvi_handle h, const bornvi_bn_desc* bn, int n, long long B, unsigned long long seed,
                     const long long* epoch_dev, long long* idx, double* logp, int* status, bornvi_stream stream);
/* bornvi_mps_log_marginals_vjp: grad_cores dev [n, 2, D, D] = sum_j c_j grad log q(evidence_j), c dev [Q] float64, the
 * evidences as for bornvi_mps_log_marginals, and logm dev [Q]: bit for bit what that call returns for the same queries.
 *   log q(e_j) = log m_j - log Z,  d m_j / d A_k[s] = 2 L^(j)_{k-1} A_k[s] E^(j)_k for s allowed at site k, 0 otherwise,
 * L^(j) the clamped left environments; minus (sum_j c_j) times the same expression of the empty mask.  G workgroups (the
 * geometry call: a function of Q only) take the queries g, g + G, ... in order and add each query's term into their own
 * partial in the workspace; one more takes the empty mask; a finishing launch adds the G partials in order: no atomics,
 * two calls are bitwise equal, a query's logm depends neither on Q nor on its slot.  An evidence whose mass is 0 or not
 * finite contributes nothing (its weight stays out of sum_j c_j too), gets logm -inf or NaN and sets status (dev [1] int32)
 * to 1, else 0.  1 <= n <= 63, 1 <= D <= 32, 1 <= Q <= 2^16; anything else, a short workspace included, is
 * BORNVI_ERR_UNSUPPORTED before any launch.  No allocation or synchronisation (capturable). */
size_t bornvi_mps_log_marginals_vjp_workspace_bytes(bornvi_handle h, int n, int D, int Q);
int bornvi_mps_log_marginals_vjp_geometry(int Q, int* G);
int bornvi_mps_log_marginals_vjp(bornvi_handle h, int n, int D, int Q, const double* cores, const long long* mask,
                                 const long long* value, const double* c, double* grad_cores, double* logm, int* status,
                                 void* workspace, size_t workspace_bytes, bornvi_stream stream);

/* The conjugate-gradient recurrence for (F + damping I) x = g, the product F p left to the caller between the calls; every
 * vector dev [P] float64, state dev [8] float64 (rr = r^T r, rr0 = g^T g, iterations done, done flag, relres = sqrt(rr / rr0),
 * fallback flag, two spare words).  One workgroup each; every dot product is a fixed-order reduction, so two solves are
 * bitwise equal.
 * bornvi_cg_init: x = 0, r = p = g, the state.  g = 0 sets the done flag (x = 0 is the solution); a non-finite entry of g
 * sets the done and the fallback flag; info (dev [1] int32) becomes the fallback flag.
 * bornvi_cg_step, given Fp = F p (without the damping): writes nothing once the done flag is set.  Otherwise
 * q = Fp + damping p and alpha = rr / p^T q; where p^T q is not positive and finite the iteration freezes (done; x stays the
 * last iterate; at iteration 0 the fallback flag is set); else x += alpha p, r -= alpha q, rr' = r^T r, p = r + (rr' / rr) p,
 * one more iteration counted, and done once rr' <= rel_tol^2 rr0.
 * bornvi_cg_finish: where the fallback flag is set or x is not finite, x = g bit for bit and info = 1; else info = 0 (an
 * unconverged x too: every iterate from x_0 = 0 is a descent direction).  iters dev [1] int32, relres dev [1] float64.
 * 1 <= P <= 2^31 - 1, damping > 0 and finite, rel_tol >= 0 and finite, else BORNVI_ERR_INVALID.  No atomics, no allocation or
 * synchronisation (capturable): the launch sequence of a solve does not depend on the data. */
int bornvi_cg_init(bornvi_handle h, long long P, const double* g, double* x, double* r, double* p, double* state, int* info,
                   bornvi_stream stream);
int bornvi_cg_step(bornvi_handle h, long long P, double damping, double rel_tol, const double* Fp, double* x, double* r,
                   double* p, double* state, bornvi_stream stream);
int bornvi_cg_finish(bornvi_handle h, long long P, const double* g, double* x, const double* state, int* info, int* iters,
                     double* relres, bornvi_stream stream);

/* ---- quantum natural gradient: the Fubini-Study metric instead of the classical Fisher matrix (what PennyLane's
 * QNGOptimizer preconditions with; no reference counterpart).  Every parameter enters exactly one gate exp(-i theta s / 2),
 * so d_a psi = 1/2 psi(theta + pi e_a).
 * bornvi_paramshift_states: states dev [include_base + p_count, 2^n] complex128 (re, im interleaved), row 0 (if
 * include_base) U(theta)|0..0>, then U(theta + pi e_p)|0..0> for p = p_begin .. p_begin + p_count - 1; canonical order
 * (wire 0 the most significant bit), WITH the correct phase and with the gates that end the circuit applied: a row
 * agrees with bornvi_adjoint_state at the same parameters to rounding.  The batched engine runs a plan of its own with
 * raw fused matrices (the pivot-normalised records of the 8-amplitude kernel drop a phase per circuit, so that kernel is
 * not used here, whatever reg_wires says); a small kernel then applies the circuit-ending CNOTs and CZs on the way from
 * the engine's buffer into `states`.  Circuits are processed in chunks of as many as the workspace holds (at least one).
 * No allocation or synchronisation once the plan exists (capturable after one eager call).  Workspace:
 * bornvi_paramshift_states_workspace_bytes(h, ansatz, n, layers, rows) holds `rows` circuits at once. */
size_t bornvi_paramshift_states_workspace_bytes(bornvi_handle h, int ansatz, int n, int layers, int rows);
int bornvi_paramshift_states(bornvi_handle h, int ansatz, int n, int layers, const double* theta, int p_begin,
                             int p_count, int include_base, double* states, void* workspace, size_t workspace_bytes,
                             bornvi_stream stream);

/* bornvi_qfi_gram: the quantum Fisher information matrix (4 x the Fubini-Study metric, 4 x PennyLane's metric_tensor;
 * Q >= F, the classical Fisher matrix, in the Loewner order) from the pi-shifted states.  phi dev [P, 2^n] complex128,
 * psi dev [2^n] complex128, both 16-byte aligned; Q dev [P, P] float64 row-major:
 *   Q_ab = Re<phi_a|phi_b> - Re(conj(c_a) c_b),  c_a = <psi|phi_a>.
 * One real split-K SYRK on the fp64 matrix cores over the P + 2 rows (phi, psi, i psi) of 2^(n+1) doubles; slab partials
 * go to the workspace and a finishing launch adds them in a fixed order, subtracts the projection term and writes Q_ab
 * and Q_ba from the same value (no atomics: two calls are bitwise equal; Q == Q^T exactly).  No allocation or
 * synchronisation (capturable).  1 <= n <= 30, 1 <= P <= 1024.  Workspace: bornvi_qfi_workspace_bytes(h, n, P). */
size_t bornvi_qfi_workspace_bytes(bornvi_handle h, int n, int P);
int bornvi_qfi_gram(bornvi_handle h, int n, int P, const double* phi, const double* psi, double* Q, void* workspace,
                    size_t workspace_bytes, bornvi_stream stream);

/* Gradient hand-off to the optimiser (replaces the float cast of the parameter-shift VJP and
 * torch.nn.utils.clip_grad_norm_(params, gradient_clip_norm), ksd_vi_quantum.py:153): grad32 dev [P] float32 =
 * float32(grad64) * min(1, max_norm / (||float32(grad64)||_2 + 1e-6)); total_norm dev [1] float32 = that norm. */
int bornvi_clip_cast_grad(bornvi_handle h, int P, const double* grad64, double max_norm,
                          float* grad32, float* total_norm, bornvi_stream stream);
/* The same plus the reference's NaN/Inf guard on the loss (ksd_vi_quantum.py:147-148, "Skipping update") as a device
 * flag: found_inf dev [1] float32 = 1 if loss (dev [1] float64) is NaN or +-Inf, else 0 -- the form torch's fused
 * optimisers consume, so a step needs no host read-back of the loss. */
int bornvi_clip_cast_grad_guard(bornvi_handle h, int P, const double* grad64, double max_norm,
                                const double* loss, float* grad32, float* total_norm,
                                float* found_inf, bornvi_stream stream);

/* The whole optimiser hand-off of one epoch in one launch, for the latency-bound sizes (a HIP-graph replay of the step
 * spends most of its nodes in the optimiser otherwise): the clip and guard above, then the update of
 * optim.Adam(lr, betas) (ksd_vi_quantum.py:92-99; eps as given, no weight decay, no amsgrad) on the float32 theta:
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *   theta -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps),
 * moments and theta in float32, the products with the double hyper-parameters in double (as torch's fused kernel).
 * A NaN / +-Inf loss leaves theta, the moments and t untouched ("Skipping update", :147-148).
 *   theta dev [P] float32 (in/out); grad32 dev [P] float32 (out: the clipped gradient, what theta.grad holds);
 *   theta64 dev [P] float64 (out: the updated theta, the next epoch's circuit input);
 *   exp_avg, exp_avg_sq dev [P] float32 (in/out, zero before the first step);
 *   counters dev [2] int32 (in/out, zero before the first step): [0] = t, good steps so far; [1] = epochs so far;
 *   lr_table dev [n_lr] float64: the learning rate of epoch e at lr_table[min(e, n_lr - 1)] (the cosine schedule of
 *   :100-103 tabulated by the host; the epoch count advances on a skipped epoch too, like scheduler.step() at :158);
 *   loss_history dev [n_lr] float64, norm_history dev [n_lr] float32, or NULL: the same entry receives this epoch's
 *   loss and gradient norm (history['loss_ksd'] / ['grad_norm'], :163-166, without a copy per epoch). */
int bornvi_clip_adam_step(bornvi_handle h, int P, const double* grad64, double max_norm,
                          const double* loss, float* theta, float* grad32, double* theta64,
                          float* exp_avg, float* exp_avg_sq, int* counters, const double* lr_table,
                          int n_lr, double beta1, double beta2, double eps, float* total_norm,
                          double* loss_history, float* norm_history, bornvi_stream stream);

/* ---- adjoint differentiation: OPT-IN second gradient engine ---------------------------
 * The reference differentiates with diff_method="parameter-shift" (quantum_born_machine.py:58, :90, :114): 2P circuit
 * evaluations.  For L = f(q) the same gradient is  dL/dtheta_k = Im <lambda_k| P_k |phi_k>  (one forward and one
 * backward walk over the gates with two states, about three circuit evaluations).  Equal to the parameter-shift
 * gradient to rounding; never used unless the caller asks (it changes what "2P evaluations" means).
 *   bornvi_adjoint_state: theta dev [P] -> state dev [2^n] complex128 = U(theta)|0..0> (canonical order, wire 0 = MSB),
 *                         probs dev [2^n] = |state|^2 or NULL;
 *   bornvi_adjoint_vjp:   state (as returned above, left untouched), dLdq dev [2^n] -> grad dev [P]
 *                         = d/dtheta sum_z dLdq[z] q_z(theta).  Deterministic (fixed summation order).
 * workspace of both: 16-byte aligned (the walk's states are carved from the pointer as given), else
 * BORNVI_ERR_WORKSPACE. */
size_t bornvi_adjoint_workspace_bytes(bornvi_handle h, int ansatz, int n, int layers);
int bornvi_adjoint_state(bornvi_handle h, int ansatz, int n, int layers, const double* theta, double* state,
                         double* probs, void* workspace, size_t workspace_bytes, bornvi_stream stream);
int bornvi_adjoint_vjp(bornvi_handle h, int ansatz, int n, int layers, const double* theta, const double* state,
                       const double* dLdq, double* grad, void* workspace, size_t workspace_bytes,
                       bornvi_stream stream);

/* ---- introspection (host only, no GPU needed): serialised execution plan of a circuit ------
 * (passes / stages / fused gates) as uint32 words; used by the CPU tests to check the
 * planner against the oracle.  Returns the number of words (writes min(cap, words)). */
long long bornvi_plan_describe(int ansatz, int n, int layers, int tile_bits, uint32_t* out,
                               size_t cap_words);

/* Host-only: first pass of the plan whose matrices depend on parameter p (what the opt-in prefix sharing orders a
 * parameter-shift batch by); returns the number of parameters, or -1 for an unsupported configuration. */
int bornvi_plan_param_first_pass(int ansatz, int n, int layers, int tile_bits, int* out, int cap);

/* The tables the fast pass kernel reads (one entry per stage, tile and thread: LDS slots with the CNOT
 * index maps folded in, CZ sign bits), derived on the host from the plan above; pass_off_out[i] = word
 * offset of pass i's header.  Returns the number of words, 0 when the plan runs on the generic kernel
 * (tiles below 2^10 amplitudes), -1 when unsupported.  Host only; used by the CPU tests. */
long long bornvi_plan_fast_describe(int ansatz, int n, int layers, int tile_bits, uint32_t* out,
                                    size_t cap_words, uint32_t* pass_off_out, int cap_passes);

/* `tile_bits` of the three functions above: bits 0-7 tile size (0 = default), bit 8 the planner's read_map option, bit 9
 * (0x200) the plan with 3 register wires per stage (8 amplitudes per thread) that the high-occupancy pass kernel runs.
 *
 * The COMPACT tables of that plan (every per-(tile row, thread) word of the fast tables is GF(2)-affine in (tile row,
 * thread): one word per lane plus one per (tile row, wave)); same return convention.  Host only; CPU tests. */
long long bornvi_plan_compact_describe(int ansatz, int n, int layers, int tile_bits, uint32_t* out,
                                       size_t cap_words, uint32_t* pass_off_out, int cap_passes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BORNVI_H */
