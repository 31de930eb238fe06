"""Records tests/golden/abi_refusals_parent.json: what libbornvi_hip.so answers to calls it must refuse, per case the return
value and the text of bornvi_last_error.  For every entry-point family: each size one step outside each limit of bornvi.h,
below and above; one required pointer null; a misaligned pointer where alignment is asked for; a workspace one byte short of
what the family's *_workspace_bytes call returns; and the options: every name read back at its default, an unknown name, and
values outside the range of "tile_bits", "workgroups_per_cu", "grad_engine" and "reg_wires".

Every case is one the library refuses in its argument checks, before it selects a device or launches anything: no case depends
on a kernel, and the one 1-KiB device buffer behind every non-null pointer is never touched.  That leaves out what is checked
later: the network descriptor's contents (read back from the device), a short workspace of the circuit, adjoint and fused-dot
calls (their size needs a compiled plan on the device) and the fused dot's "needs a multi-pass plan" refusal.

bornvi_last_error keeps its text until the next failure, and a few refusals set none (a size query that returns 0, the
host-only geometry calls): before every case a read of the unknown option SENTINEL sets a known text, so such a case records
"unknown option <SENTINEL>".

tests/test_gpu_abi_refusals.py takes its cases and run_case() from here; only the C ABI is used, through the binding's loaded
library, so this file alone can be copied onto the commit whose answers are to be kept and run there.  The file in the
repository was recorded on the last commit before the binding, the limits and the option table were derived from bornvi.h.
Run from the repository root: python tests/golden/make_golden_abi_refusals.py [output.json]"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

SENTINEL = "?"
BUFFER_BYTES = 1024
OPTION_NAMES = ("workgroups_per_cu", "fast_workgroups_per_cu", "fast_path", "prefix_share", "batched_quadform", "grad_engine",
                "zero_support", "alternate_walk", "direct_stages", "tile_bits", "tile_bits_multi", "low_bits", "max_threads",
                "read_map", "reg_wires", "contig_out")
# the two options the recorded library sets but does not read back (the test's one allowance)
SET_ONLY_OPTIONS = {"workgroups_per_cu": 0, "max_threads": 1024}      # name: default

# Symbolic argument values, resolved by run_case: "p" the device buffer, "p8" the buffer + 8 bytes (not 16-byte aligned),
# None a null pointer, "bn" a well-formed network descriptor, ("bn", {...}) one with fields replaced, "short" one byte less
# than the family's size query returns for the call's own good arguments.
WS = dict(workspace="p", workspace_bytes=BUFFER_BYTES)
ST = dict(stream=None)
CIRC = dict(ansatz=0, n=2, layers=1)

# name: (good arguments in declaration order, without the handle; size query of its workspace and that query's argument names)
FUNCTIONS = {
    "bornvi_circuit_workspace_bytes": (dict(**CIRC, batch=1), None),
    "bornvi_circuit_probs": (dict(**CIRC, batch=1, thetas="p", probs="p", **WS, **ST), None),
    "bornvi_paramshift_probs": (dict(**CIRC, theta="p", p_begin=0, p_end=1, include_base=0, probs="p", **WS, **ST), None),
    "bornvi_paramshift_probs_strided": (dict(**CIRC, theta="p", p_begin=0, p_count=1, p_stride=1, include_base=0, probs="p", **WS, **ST), None),
    "bornvi_paramshift_grad_workspace_bytes": (dict(**CIRC, p_begin=0, p_end=1), None),
    "bornvi_paramshift_grad": (dict(**CIRC, theta="p", dLdq="p", p_begin=0, p_end=1, grad="p", **WS, **ST), None),
    "bornvi_paramshift_dot_workspace_bytes": (dict(**CIRC, p_count=1), None),
    "bornvi_paramshift_dot_begin": (dict(**CIRC, theta="p", p_begin=0, p_count=1, p_stride=1, q_out="p", **WS, **ST), None),
    "bornvi_paramshift_dot_finish": (dict(**CIRC, p_count=1, w="p", ksd2="p", grad="p", loss_out="p", **WS, **ST), None),
    "bornvi_paramshift_states_workspace_bytes": (dict(**CIRC, rows=1), None),
    "bornvi_paramshift_states": (dict(**CIRC, theta="p", p_begin=0, p_count=1, include_base=0, states="p", **WS, **ST), None),
    "bornvi_adjoint_workspace_bytes": (dict(**CIRC), None),
    "bornvi_adjoint_state": (dict(**CIRC, theta="p", state="p", probs="p", **WS, **ST), None),
    "bornvi_adjoint_vjp": (dict(**CIRC, theta="p", state="p", dLdq="p", grad="p", **WS, **ST), None),
    "bornvi_stein_matvec_kron_workspace_bytes": (dict(n=2), None),
    "bornvi_stein_matvec_kron": (dict(n=2, length_scale=1.0, S="p", q="p", y="p", ksd2="p", **WS, **ST), None),
    "bornvi_gate1q_apply": (dict(n=2, batch=1, state="p", wire=0, U="p", **ST), None),
    "bornvi_cnot_apply": (dict(n=2, batch=1, state="p", control=0, target=1, **ST), None),
    "bornvi_born_probs": (dict(n=2, batch=1, state="p", probs="p", **ST), None),
    "bornvi_score_from_cpts": (dict(bn="bn", n=2, S="p", pxz="p", **ST), None),
    "bornvi_bn_logjoint_samples": (dict(bn="bn", n=2, B=2, idx="p", p_floor=1e-12, logp="p", **ST), None),
    "bornvi_bn_score_samples": (dict(bn="bn", n=2, B=2, idx="p", p_floor=1e-12, S="p", logp="p", **ST), None),
    "bornvi_bn_sample": (dict(bn="bn", n=2, B=2, seed=1, epoch_dev="p", idx="p", logp="p", status="p", **ST), None),
    "bornvi_stein_pairs_workspace_bytes": (dict(n=2, B=2), None),
    "bornvi_stein_pairs_rowsum": (dict(n=2, B=2, length_scale=1.0, idx="p", S="p", r="p", total="p", **WS, **ST),
                                  ("bornvi_stein_pairs_workspace_bytes", ("n", "B"))),
    "bornvi_stein_gram_build": (dict(n=2, length_scale=1.0, S="p", K="p", **ST), None),
    "bornvi_stein_gram_build_rows": (dict(n=2, length_scale=1.0, S="p", row_begin=0, row_end=1, K_rows="p", **ST), None),
    "bornvi_stein_gram_build_rows_ld": (dict(n=2, length_scale=1.0, S="p", row_begin=0, row_end=1, K_rows="p", ld=4, **ST), None),
    "bornvi_stein_kp_pairs": (dict(n=2, length_scale=1.0, M=1, zi="p", zj="p", si="p", sj="p", out="p", **ST), None),
    "bornvi_stein_quadform_workspace_bytes": (dict(n=2, B=2), None),
    "bornvi_stein_quadform": (dict(n=2, K="p", Q="p", B=2, ksd2="p", Y="p", **WS, **ST),
                              ("bornvi_stein_quadform_workspace_bytes", ("n", "B"))),
    "bornvi_stein_quadform_ld": (dict(n=2, K="p", ld=4, Q="p", B=2, ksd2="p", Y="p", **WS, **ST),
                                 ("bornvi_stein_quadform_workspace_bytes", ("n", "B"))),
    "bornvi_stein_quadform_sym_workspace_bytes": (dict(n=2), None),
    "bornvi_stein_quadform_sym": (dict(n=2, K="p", q="p", ksd2="p", y="p", **WS, **ST),
                                  ("bornvi_stein_quadform_sym_workspace_bytes", ("n",))),
    "bornvi_stein_quadform_sym_ld": (dict(n=2, K="p", ld=4, q="p", ksd2="p", y="p", **WS, **ST),
                                     ("bornvi_stein_quadform_sym_workspace_bytes", ("n",))),
    "bornvi_stein_quadform_sym_pairs": (dict(n=2, K_lo="p", K_hi="p", pair_begin=0, pair_end=1, q="p", ksd2_partial="p",
                                             y_partial="p", **WS, **ST), None),
    "bornvi_stein_quadform_sym_pairs_ld": (dict(n=2, K_lo="p", K_hi="p", ld=4, pair_begin=0, pair_end=1, q="p", ksd2_partial="p",
                                                y_partial="p", **WS, **ST), None),
    "bornvi_stein_quadform_rows": (dict(n=2, K_rows="p", row_begin=0, row_end=1, q="p", y_rows="p", ksd2_partial="p", **WS, **ST),
                                   ("bornvi_stein_quadform_workspace_bytes", ("n", 1))),
    "bornvi_ksd_grad_finish": (dict(n=2, shifted="p", n_shift=1, y="p", ksd2="p", loss_out="p", dLdq_out="p", grad="p", **ST), None),
    "bornvi_shots_workspace_bytes": (dict(n=2, B=2), None),
    "bornvi_shots_histogram": (dict(n=2, B=2, probs="p", freq="p", shots=1, seed=1, epoch_dev="p", include_base=0, p_begin=0,
                                    p_stride=1, **WS, **ST), ("bornvi_shots_workspace_bytes", ("n", "B"))),
    "bornvi_born_table_workspace_bytes": (dict(n=2, rows=1), None),
    "bornvi_born_table_probs": (dict(n=2, rows=1, mode=0, w="p", q32="p", q64="p", entropy="p", **WS, **ST),
                                ("bornvi_born_table_workspace_bytes", ("n", "rows"))),
    "bornvi_born_table_vjp": (dict(n=2, rows=1, mode=0, w="p", q64="p", y="p", ksd2="p", entropy_weight=0.0, grad="p",
                                   loss_out="p", **WS, **ST), ("bornvi_born_table_workspace_bytes", ("n", "rows"))),
    "bornvi_reinforce_workspace_bytes": (dict(n=2, B=2), None),
    "bornvi_reinforce_step": (dict(n=2, B=2, idx="p", logit="p", log_p="p", q32="p", baseline="p", first=1, baseline_decay=0.9,
                                   entropy_coef=0.0, q_floor=1e-10, dLdq="p", loss="p", found_inf="p", **WS, **ST),
                              ("bornvi_reinforce_workspace_bytes", ("n", "B"))),
    "bornvi_elbo_workspace_bytes": (dict(n=2, rows=1), None),
    "bornvi_elbo_weights": (dict(n=2, rows=1, q="p", log_p="p", q_floor=1e-10, w="p", neg_elbo="p", entropy="p", **WS, **ST),
                            ("bornvi_elbo_workspace_bytes", ("n", "rows"))),
    "bornvi_mps_workspace_bytes": (dict(n=2, D=2), None),
    "bornvi_mps_probs": (dict(n=2, D=2, cores="p", q64="p", q32="p", psi="p", Z_out="p", **WS, **ST),
                         ("bornvi_mps_workspace_bytes", ("n", "D"))),
    "bornvi_mps_vjp": (dict(n=2, D=2, cores="p", g="p", grad_cores="p", **WS, **ST), ("bornvi_mps_workspace_bytes", ("n", "D"))),
    "bornvi_mps_sample_workspace_bytes": (dict(n=2, D=2, B=2), None),
    "bornvi_mps_environments": (dict(n=2, D=2, B=2, cores="p", log_Z_out="p", **WS, **ST),
                                ("bornvi_mps_sample_workspace_bytes", ("n", "D", "B"))),
    "bornvi_mps_sample": (dict(n=2, D=2, B=2, cores="p", seed=1, epoch_dev="p", idx="p", logq="p", status="p", **WS, **ST),
                          ("bornvi_mps_sample_workspace_bytes", ("n", "D", "B"))),
    "bornvi_mps_score_vjp": (dict(n=2, D=2, B=2, cores="p", idx="p", w="p", logq="p", grad_cores="p", status="p", **WS, **ST),
                             ("bornvi_mps_sample_workspace_bytes", ("n", "D", "B"))),
    "bornvi_mps_score_rows": (dict(n=2, D=2, B=2, cores="p", idx="p", k_begin=0, k_count=1, ld=64, rows="p", status="p", **WS, **ST),
                              ("bornvi_mps_sample_workspace_bytes", ("n", "D", "B"))),
    "bornvi_score_fisher_workspace_bytes": (dict(R=2, nblocks=1, ld=64), None),
    "bornvi_score_fisher_gram": (dict(R=2, nblocks=1, B=2, ld=64, rows="p", F="p", **WS, **ST),
                                 ("bornvi_score_fisher_workspace_bytes", ("R", "nblocks", "ld"))),
    "bornvi_mps_score_sample_gram_workspace_bytes": (dict(n=2, D=2, B=2), None),
    "bornvi_mps_score_sample_gram": (dict(n=2, D=2, B=2, cores="p", idx="p", T="p", status="p", env_workspace="p",
                                          env_workspace_bytes=1 << 40, **WS, **ST),
                                     ("bornvi_mps_score_sample_gram_workspace_bytes", ("n", "D", "B"))),
    "bornvi_mps_score_jvp": (dict(n=2, D=2, B=2, cores="p", idx="p", v="p", scale=1.0, t="p", status="p", env_workspace="p",
                                  env_workspace_bytes=BUFFER_BYTES, **ST), None),
    "bornvi_mps_query_workspace_bytes": (dict(n=2, D=2, Q=1), None),
    "bornvi_mps_log_marginals": (dict(n=2, D=2, Q=1, cores="p", mask="p", value="p", logm="p", status="p", **WS, **ST),
                                 ("bornvi_mps_query_workspace_bytes", ("n", "D", "Q"))),
    "bornvi_mps_sample_clamped": (dict(n=2, D=2, B=2, cores="p", mask="p", value="p", seed=1, epoch_dev="p", idx="p", logq="p",
                                       logm="p", status="p", **WS, **ST), ("bornvi_mps_query_workspace_bytes", ("n", "D", 1))),
    "bornvi_mps_marginals": (dict(n=2, D=2, cores="p", m1="p", m2="p", **WS, **ST), ("bornvi_mps_query_workspace_bytes", ("n", "D", 1))),
    "bornvi_mps_log_marginals_vjp_workspace_bytes": (dict(n=2, D=2, Q=1), None),
    "bornvi_mps_log_marginals_vjp": (dict(n=2, D=2, Q=1, cores="p", mask="p", value="p", c="p", grad_cores="p", logm="p",
                                          status="p", **WS, **ST), ("bornvi_mps_log_marginals_vjp_workspace_bytes", ("n", "D", "Q"))),
    "bornvi_mps_canon_workspace_bytes": (dict(n=2, D=2), None),
    "bornvi_mps_canonicalise": (dict(n=2, D=2, D_out=2, cutoff=0.0, cores="p", cores_out="p", schmidt="p", discarded="p", rank="p",
                                     log_norm="p", status="p", **WS, **ST), ("bornvi_mps_canon_workspace_bytes", ("n", "D"))),
    "bornvi_cg_init": (dict(P=2, g="p", x="p", r="p", p="p", state="p", info="p", **ST), None),
    "bornvi_cg_step": (dict(P=2, damping=1.0, rel_tol=0.0, Fp="p", x="p", r="p", p="p", state="p", **ST), None),
    "bornvi_cg_finish": (dict(P=2, g="p", x="p", state="p", info="p", iters="p", relres="p", **ST), None),
    "bornvi_fisher_workspace_bytes": (dict(n=2, n_shift=2), None),
    "bornvi_fisher_gram": (dict(n=2, shifted="p", n_shift=2, q="p", q_floor=1e-10, F="p", **WS, **ST),
                           ("bornvi_fisher_workspace_bytes", ("n", "n_shift"))),
    "bornvi_spd_solve_workspace_bytes": (dict(P=2), None),
    "bornvi_spd_solve": (dict(P=2, A="p", damping=0.0, b="p", x="p", info="p", **WS, **ST), ("bornvi_spd_solve_workspace_bytes", ("P",))),
    "bornvi_spd_solve_batched_workspace_bytes": (dict(P=2, nb=1), None),
    "bornvi_spd_solve_batched": (dict(P=2, nb=1, A="p", damping=0.0, b="p", x="p", info="p", **WS, **ST),
                                 ("bornvi_spd_solve_batched_workspace_bytes", ("P", "nb"))),
    "bornvi_qfi_workspace_bytes": (dict(n=2, P=2), None),
    "bornvi_qfi_gram": (dict(n=2, P=2, phi="p", psi="p", Q="p", **WS, **ST), ("bornvi_qfi_workspace_bytes", ("n", "P"))),
    "bornvi_clip_cast_grad": (dict(P=2, grad64="p", max_norm=1.0, grad32="p", total_norm="p", **ST), None),
    "bornvi_clip_cast_grad_guard": (dict(P=2, grad64="p", max_norm=1.0, loss="p", grad32="p", total_norm="p", found_inf="p", **ST), None),
    "bornvi_clip_adam_step": (dict(P=2, grad64="p", max_norm=1.0, loss="p", theta="p", grad32="p", theta64="p", exp_avg="p",
                                   exp_avg_sq="p", counters="p", lr_table="p", n_lr=1, beta1=0.9, beta2=0.999, eps=1e-8,
                                   total_norm="p", loss_history="p", norm_history="p", **ST), None),
}
HANDLE_FREE = {"bornvi_stein_gram_ld": dict(n=2), "bornvi_stein_pairs_geometry": dict(B=2, tiles_per_range="host", num_ranges="host"),
               "bornvi_mps_log_marginals_vjp_geometry": dict(Q=1, G="host")}

INF = float("inf")
M24, M17, M16, M31 = 1 << 24, 1 << 17, 1 << 16, 1 << 31
CIRCUIT_N = (0, 30)                 # outside 1 .. 29
TABLE_N = (0, 31)                   # outside 1 .. 30
DENSE_N = (-1, 0, 18, 41)           # outside 1 .. 17, and outside what the calls without `ld` shift by
SAMPLED = dict(n=(0, 64), D=(0, 33))
# name: {argument: values outside its range}; every (argument, value) is one case, the other arguments good
OUTSIDE = {
    "bornvi_circuit_workspace_bytes": dict(n=CIRCUIT_N, batch=(-1,)),
    "bornvi_circuit_probs": dict(n=CIRCUIT_N, batch=(-1,)),
    "bornvi_paramshift_probs": dict(n=CIRCUIT_N, p_end=(-1, 99)),
    "bornvi_paramshift_probs_strided": dict(n=CIRCUIT_N, p_begin=(-1, 99), p_count=(-1, 99), p_stride=(0,)),
    "bornvi_paramshift_grad_workspace_bytes": dict(n=CIRCUIT_N, p_end=(-1,)),
    "bornvi_paramshift_dot_workspace_bytes": dict(n=CIRCUIT_N, p_count=(-1,)),
    "bornvi_paramshift_dot_begin": dict(n=CIRCUIT_N, p_begin=(-1, 99), p_count=(-1, 99), p_stride=(0,)),
    "bornvi_paramshift_dot_finish": dict(n=CIRCUIT_N, p_count=(-1,)),
    "bornvi_paramshift_states_workspace_bytes": dict(n=CIRCUIT_N, rows=(-1,)),
    "bornvi_paramshift_states": dict(n=CIRCUIT_N, p_begin=(-1, 99), p_count=(-1, 99)),
    "bornvi_adjoint_workspace_bytes": dict(n=CIRCUIT_N),
    "bornvi_adjoint_state": dict(n=CIRCUIT_N),
    "bornvi_adjoint_vjp": dict(n=CIRCUIT_N),
    "bornvi_stein_matvec_kron_workspace_bytes": dict(n=CIRCUIT_N),
    "bornvi_stein_matvec_kron": dict(n=CIRCUIT_N, length_scale=(0.0,)),
    "bornvi_gate1q_apply": dict(n=(0, 41), wire=(-1, 2), batch=(-1,)),
    "bornvi_cnot_apply": dict(n=(1, 41), control=(-1, 2), target=(0, 2), batch=(-1,)),
    "bornvi_born_probs": dict(n=(-1, 41), batch=(-1,)),
    "bornvi_score_from_cpts": dict(n=TABLE_N, bn=(("bn", dict(num_nodes=0)), ("bn", dict(num_nodes=65)), ("bn", dict(max_parents=0)))),
    "bornvi_bn_logjoint_samples": dict(n=(0, 64), B=(0, M24 + 1), p_floor=(0.0, INF)),
    "bornvi_bn_score_samples": dict(n=(0, 64), B=(0, M24 + 1), p_floor=(0.0, INF)),
    "bornvi_bn_sample": dict(n=(0, 64), B=(0, M24 + 1)),
    "bornvi_stein_pairs_workspace_bytes": dict(n=(0, 64), B=(1, M17 + 1)),
    "bornvi_stein_pairs_rowsum": dict(n=(0, 64), B=(1, M17 + 1), length_scale=(0.25, INF)),
    "bornvi_stein_pairs_geometry": dict(B=(1, M17 + 1)),
    "bornvi_stein_gram_ld": dict(n=(0, 18)),
    "bornvi_stein_gram_build": dict(n=DENSE_N, length_scale=(0.0,)),
    "bornvi_stein_gram_build_rows": dict(n=DENSE_N, row_begin=(-1,), row_end=(5,)),
    "bornvi_stein_gram_build_rows_ld": dict(n=(0, 18), ld=(2, 5, 4 + 4098), row_end=(5,), length_scale=(0.0,)),
    "bornvi_stein_kp_pairs": dict(n=TABLE_N, M=(-1,), length_scale=(0.0,)),
    "bornvi_stein_quadform_workspace_bytes": dict(n=TABLE_N),
    "bornvi_stein_quadform": dict(n=DENSE_N, B=(-1,)),
    "bornvi_stein_quadform_ld": dict(n=(0, 18), ld=(2, 5, 4 + 4098), B=(-1,)),
    "bornvi_stein_quadform_sym_workspace_bytes": dict(n=(0, 18)),
    "bornvi_stein_quadform_sym": dict(n=DENSE_N),
    "bornvi_stein_quadform_sym_ld": dict(n=(0, 18), ld=(2, 5, 6, 4 + 4098)),     # 6: a padded K below two bands of rows
    "bornvi_stein_quadform_sym_pairs": dict(n=DENSE_N + (2,)),                     # 2: fewer than two bands of rows
    "bornvi_stein_quadform_sym_pairs_ld": dict(n=(0, 18), ld=(2, 5, 4 + 4098)),
    "bornvi_stein_quadform_rows": dict(n=(0, 18), row_begin=(-1,), row_end=(5,)),
    "bornvi_ksd_grad_finish": dict(n=TABLE_N, n_shift=(-1,)),
    "bornvi_shots_workspace_bytes": dict(n=TABLE_N, B=(-1,)),
    "bornvi_shots_histogram": dict(n=TABLE_N, B=(-1,), shots=(0, M31), p_begin=(-1,), p_stride=(0,)),
    "bornvi_born_table_workspace_bytes": dict(n=(-1, 31), rows=(0, M16)),
    "bornvi_born_table_probs": dict(n=(-1, 31), rows=(0, M16), mode=(-1, 2)),
    "bornvi_born_table_vjp": dict(n=(-1, 31), rows=(0, M16), mode=(-1, 2), entropy_weight=(INF,)),
    "bornvi_reinforce_workspace_bytes": dict(n=TABLE_N, B=(0, M24 + 1)),
    "bornvi_reinforce_step": dict(n=TABLE_N, B=(0, M24 + 1), q_floor=(-1.0,), baseline_decay=(INF,)),
    "bornvi_elbo_workspace_bytes": dict(n=TABLE_N, rows=(0, M16)),
    "bornvi_elbo_weights": dict(n=TABLE_N, rows=(0, M16), q_floor=(0.0, INF)),
    "bornvi_mps_workspace_bytes": dict(n=(0, 27), D=(0, 33)),
    "bornvi_mps_probs": dict(n=(0, 27), D=(0, 33)),
    "bornvi_mps_vjp": dict(n=(0, 27), D=(0, 33)),
    "bornvi_mps_sample_workspace_bytes": dict(**SAMPLED, B=(0, M24 + 1)),
    "bornvi_mps_environments": dict(**SAMPLED, B=(0, M24 + 1)),
    "bornvi_mps_sample": dict(**SAMPLED, B=(0, M24 + 1)),
    "bornvi_mps_score_vjp": dict(**SAMPLED, B=(0, M24 + 1)),
    "bornvi_mps_score_rows": dict(**SAMPLED, B=(1, M24 + 1), ld=(32, 96, 2 * M24), k_begin=(-1,), k_count=(0, 3)),
    "bornvi_score_fisher_workspace_bytes": dict(R=(0, 1025), nblocks=(0, M16), ld=(32, 96, 2 * M24)),
    "bornvi_score_fisher_gram": dict(R=(0, 1025), nblocks=(0, M16), B=(1, 65, M24 + 1), ld=(32, 96, 2 * M24)),   # B = 65 > ld
    "bornvi_mps_score_sample_gram_workspace_bytes": dict(**SAMPLED, B=(1, 1025)),
    "bornvi_mps_score_sample_gram": dict(**SAMPLED, B=(1, 1025), env_workspace_bytes=(0,)),
    "bornvi_mps_score_jvp": dict(**SAMPLED, B=(1, M24 + 1), scale=(INF,), env_workspace_bytes=(0,)),
    "bornvi_mps_query_workspace_bytes": dict(**SAMPLED, Q=(0, M16 + 1)),
    "bornvi_mps_log_marginals": dict(**SAMPLED, Q=(0, M16 + 1)),
    "bornvi_mps_sample_clamped": dict(**SAMPLED, B=(0, M24 + 1)),
    "bornvi_mps_marginals": dict(**SAMPLED),
    "bornvi_mps_log_marginals_vjp_workspace_bytes": dict(**SAMPLED, Q=(0, M16 + 1)),
    "bornvi_mps_log_marginals_vjp_geometry": dict(Q=(0, M16 + 1)),
    "bornvi_mps_log_marginals_vjp": dict(**SAMPLED, Q=(0, M16 + 1)),
    "bornvi_mps_canon_workspace_bytes": dict(**SAMPLED),
    "bornvi_mps_canonicalise": dict(**SAMPLED, D_out=(0, 3), cutoff=(-1.0, INF)),
    "bornvi_cg_init": dict(P=(0, M31)),
    "bornvi_cg_step": dict(P=(0, M31), damping=(0.0, INF), rel_tol=(-1.0, INF)),
    "bornvi_cg_finish": dict(P=(0, M31)),
    "bornvi_fisher_workspace_bytes": dict(n=TABLE_N, n_shift=(0, 1025)),
    "bornvi_fisher_gram": dict(n=TABLE_N, n_shift=(0, 1025), q_floor=(0.0, INF)),
    "bornvi_spd_solve_workspace_bytes": dict(P=(0, 1025)),
    "bornvi_spd_solve": dict(P=(0, 1025), damping=(-1.0, INF)),
    "bornvi_spd_solve_batched_workspace_bytes": dict(P=(0, 1025), nb=(0, M16)),
    "bornvi_spd_solve_batched": dict(P=(0, 1025), nb=(0, M16), damping=(-1.0, INF)),
    "bornvi_qfi_workspace_bytes": dict(n=TABLE_N, P=(0, 1025)),
    "bornvi_qfi_gram": dict(n=TABLE_N, P=(0, 1025)),
    "bornvi_clip_cast_grad": dict(P=(-1,), max_norm=(-1.0,)),
    "bornvi_clip_cast_grad_guard": dict(P=(-1,), max_norm=(-1.0,)),
    "bornvi_clip_adam_step": dict(P=(0,), n_lr=(0,), beta1=(1.0,), eps=(-1.0,)),
}
# name: pointer arguments the call requires, each null in a case of its own; then those that must be 16-byte aligned
REQUIRED = {
    "bornvi_circuit_probs": ("thetas", "probs"), "bornvi_paramshift_probs": ("theta", "probs"),
    "bornvi_paramshift_grad": ("theta", "dLdq", "grad"), "bornvi_paramshift_dot_begin": ("theta", "q_out"),
    "bornvi_paramshift_dot_finish": ("w", "grad"), "bornvi_paramshift_states": ("theta", "states"),
    "bornvi_stein_matvec_kron": ("S", "q", "ksd2"), "bornvi_gate1q_apply": ("state", "U"), "bornvi_cnot_apply": ("state",),
    "bornvi_born_probs": ("state", "probs"), "bornvi_score_from_cpts": ("bn", "S"),
    "bornvi_bn_logjoint_samples": ("bn", "idx", "logp"), "bornvi_bn_score_samples": ("bn", "idx", "S"),
    "bornvi_bn_sample": ("bn", "epoch_dev", "idx", "logp", "status"), "bornvi_stein_pairs_rowsum": ("idx", "S", "r", "total", "workspace"),
    "bornvi_stein_pairs_geometry": ("tiles_per_range", "num_ranges"), "bornvi_stein_gram_build": ("S", "K"),
    "bornvi_stein_gram_build_rows_ld": ("S", "K_rows"), "bornvi_stein_kp_pairs": ("zi", "out"),
    "bornvi_stein_quadform": ("K", "Q", "ksd2", "workspace"), "bornvi_stein_quadform_sym": ("K", "q", "ksd2", "workspace"),
    "bornvi_stein_quadform_sym_pairs_ld": ("K_lo", "q", "ksd2_partial", "y_partial"),
    "bornvi_stein_quadform_rows": ("K_rows", "q", "ksd2_partial", "workspace"), "bornvi_ksd_grad_finish": ("shifted", "y", "ksd2", "grad"),
    "bornvi_shots_histogram": ("probs", "freq", "epoch_dev", "workspace"), "bornvi_born_table_probs": ("w", "q32", "q64", "workspace"),
    "bornvi_born_table_vjp": ("w", "q64", "grad", "ksd2", "workspace"),
    "bornvi_reinforce_step": ("idx", "logit", "log_p", "q32", "baseline", "dLdq", "loss", "found_inf", "workspace"),
    "bornvi_elbo_weights": ("q", "log_p", "neg_elbo", "workspace"), "bornvi_mps_probs": ("cores", "q64", "Z_out", "workspace"),
    "bornvi_mps_vjp": ("cores", "g", "grad_cores", "workspace"), "bornvi_mps_environments": ("cores", "workspace"),
    "bornvi_mps_sample": ("cores", "epoch_dev", "idx", "logq", "status", "workspace"),
    "bornvi_mps_score_vjp": ("cores", "idx", "w", "logq", "grad_cores", "status", "workspace"),
    "bornvi_mps_score_rows": ("cores", "idx", "rows", "status", "workspace"), "bornvi_score_fisher_gram": ("rows", "F", "workspace"),
    "bornvi_mps_score_sample_gram": ("cores", "idx", "T", "status", "env_workspace", "workspace"),
    "bornvi_mps_score_jvp": ("cores", "idx", "v", "t", "status", "env_workspace"),
    "bornvi_mps_log_marginals": ("cores", "mask", "value", "logm", "status", "workspace"),
    "bornvi_mps_sample_clamped": ("cores", "mask", "value", "epoch_dev", "idx", "logq", "logm", "status", "workspace"),
    "bornvi_mps_marginals": ("cores", "m1", "workspace"), "bornvi_mps_log_marginals_vjp_geometry": ("G",),
    "bornvi_mps_log_marginals_vjp": ("cores", "mask", "value", "c", "grad_cores", "logm", "status", "workspace"),
    "bornvi_mps_canonicalise": ("cores", "cores_out", "schmidt", "discarded", "rank", "log_norm", "status", "workspace"),
    "bornvi_cg_init": ("g", "x", "r", "p", "state", "info"), "bornvi_cg_step": ("Fp", "x", "r", "p", "state"),
    "bornvi_cg_finish": ("g", "x", "state", "info", "iters", "relres"), "bornvi_fisher_gram": ("shifted", "q", "F", "workspace"),
    "bornvi_spd_solve": ("A", "b", "x", "info", "workspace"), "bornvi_spd_solve_batched": ("A", "b", "x", "info", "workspace"),
    "bornvi_qfi_gram": ("phi", "psi", "Q", "workspace"), "bornvi_clip_cast_grad": ("grad64", "grad32", "total_norm"),
    "bornvi_clip_cast_grad_guard": ("grad64", "grad32", "total_norm", "loss", "found_inf"),
    "bornvi_clip_adam_step": ("grad64", "loss", "theta", "grad32", "theta64", "exp_avg", "exp_avg_sq", "counters", "lr_table", "total_norm"),
}
ALIGNED = {
    "bornvi_paramshift_states": ("states",), "bornvi_stein_quadform_sym": ("K", "workspace"),
    "bornvi_stein_quadform_sym_pairs_ld": ("K_lo", "K_hi"), "bornvi_mps_score_rows": ("rows",), "bornvi_score_fisher_gram": ("rows",),
    "bornvi_fisher_gram": ("shifted", "q"), "bornvi_qfi_gram": ("phi", "psi"),
}
# option cases: (id, "get" or "set", name, value)
OPTION_CASES = [(f"get:{name}", "get", name, 0) for name in OPTION_NAMES + ("no_such_option",)] + \
               [("set:no_such_option", "set", "no_such_option", 1)] + \
               [(f"set:{name}={v}", "set", name, v) for name, v in (("tile_bits", 3), ("tile_bits", 14), ("workgroups_per_cu", -1),
                                                                    ("workgroups_per_cu", 17), ("grad_engine", -1), ("grad_engine", 2),
                                                                    ("reg_wires", 2), ("reg_wires", 5))]


def _cases():
    out = []
    for name, good in list((k, v[0]) for k, v in FUNCTIONS.items()) + list(HANDLE_FREE.items()):
        for arg, values in OUTSIDE.get(name, {}).items():
            out += [(f"{name}:{arg}={v[1] if isinstance(v, tuple) else v}", name, {arg: v}) for v in values]
        out += [(f"{name}:{arg}=null", name, {arg: None}) for arg in REQUIRED.get(name, ())]
        out += [(f"{name}:{arg}=misaligned", name, {arg: "p8"}) for arg in ALIGNED.get(name, ())]
        if name in FUNCTIONS and FUNCTIONS[name][1]:
            out.append((f"{name}:workspace_bytes=short", name, {"workspace_bytes": "short"}))
    return out


CASES = _cases()        # (id, function, {argument: value replacing the good one})


class Session:
    """A handle of its own (so that nothing a case sets outlives it) and the one device buffer."""

    def __init__(self):
        import torch
        from tensornetworks_amd import _ext
        assert torch.cuda.is_available(), "needs an MI355X"
        self.lib = _ext.lib()
        self.handle = _ext.Handle(torch.cuda.current_device())
        self.buffer = torch.zeros(BUFFER_BYTES, dtype=torch.uint8, device="cuda")
        self.host = (C.c_int * 4)()
        self.descriptors = []
        self.BnDesc = _ext.BnDesc

    def close(self):
        self.handle.close()

    def _value(self, v):
        p = self.buffer.data_ptr()
        if v == "p":
            return p
        if v == "p8":
            return p + 8
        if v == "host":
            return C.addressof(self.host)
        if v == "bn" or (isinstance(v, tuple) and v[0] == "bn"):
            fields = dict(num_nodes=2, max_parents=8, role=p, n_parents=p, parents=p, cpt_off=p, cpt=p)
            fields.update(v[1] if isinstance(v, tuple) else {})
            self.descriptors.append(self.BnDesc(**fields))
            return C.byref(self.descriptors[-1])
        return v

    def _call(self, name, values):
        fn = getattr(self.lib, name)
        # (where a binding declares a host pointer as POINTER(T), an address is cast to that type)
        return fn(*(C.cast(C.c_void_p(v), t) if isinstance(v, int) and issubclass(t, C._Pointer) else v
                    for v, t in zip(values, fn.argtypes)))

    def _sentinel(self):
        rc = self.lib.bornvi_get_option(self.handle.h, SENTINEL.encode(), C.byref(C.c_longlong()))
        assert rc != 0

    def error(self):
        return self.lib.bornvi_last_error(self.handle.h).decode()

    def run_case(self, case):
        """[return value, text of bornvi_last_error] of one case."""
        _, name, replaced = case
        if name in HANDLE_FREE:
            args = dict(HANDLE_FREE[name], **replaced)
            self._sentinel()
            return [int(self._call(name, [self._value(v) for v in args.values()])), self.error()]
        good, size_query = FUNCTIONS[name]
        args = dict(good, **replaced)
        if args.get("workspace_bytes") == "short":
            query, names = size_query
            need = getattr(self.lib, query)(self.handle.h, *(good[a] if isinstance(a, str) else a for a in names))
            assert need > 0, (name, query, self.error())
            args["workspace_bytes"] = need - 1
        self._sentinel()
        return [int(self._call(name, [self.handle.h] + [self._value(v) for v in args.values()])), self.error()]

    def run_option_case(self, case):
        """[return value, text, value read or None] of one option case."""
        _, kind, name, value = case
        self._sentinel()
        if kind == "set":
            return [int(self.lib.bornvi_set_option(self.handle.h, name.encode(), value)), self.error(), None]
        out = C.c_longlong(-12345)
        rc = int(self.lib.bornvi_get_option(self.handle.h, name.encode(), C.byref(out)))
        return [rc, self.error(), int(out.value) if rc == 0 else None]


if __name__ == "__main__":
    s = Session()
    out = {}
    for case in CASES:
        got = s.run_case(case)
        refused = got[0] == 0 if case[1].endswith("_workspace_bytes") or case[1] == "bornvi_stein_gram_ld" else got[0] < 0
        assert refused, (case, got)
        assert case[0] not in out, case[0]
        out[case[0]] = got
    for case in OPTION_CASES:
        assert case[0] not in out, case[0]
        out[case[0]] = s.run_option_case(case)
    s.close()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "abi_refusals_parent.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")
