"""CPU-side checks: the C-ABI library loads and exports every symbol include/bornvi.h declares,
the circuit planner (C++ host code) is correct against the oracle via the NumPy plan emulator,
host helpers mirror the reference, and the product refuses to run without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import circuit as oc, stein as os_
import plan_emulator as pe
from conftest import REPO, golden


def test_library_exports_every_declared_symbol():
    from tensornetworks_amd import _ext
    lib = _ext.lib()
    hdr = open(os.path.join(REPO, "include", "bornvi.h")).read()
    declared = set(re.findall(r"\b(bornvi_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} declared in bornvi.h but not exported"
    assert declared == set(_ext.EXPORTED_SYMBOLS), declared ^ set(_ext.EXPORTED_SYMBOLS)
    assert lib.bornvi_version() == 100
    for ansatz, aid in _ext.ANSATZ_IDS.items():
        for n, L in [(3, 4), (8, 4), (16, 6), (20, 8)]:
            assert lib.bornvi_num_params(aid, n, L) == oc.num_params(ansatz, n, L)
            assert lib.bornvi_num_gates(aid, n, L) == len(oc.gate_list(ansatz, n, L))
    assert lib.bornvi_num_params(7, 3, 1) == -1 and lib.bornvi_num_gates(7, 3, 1) == -1


# What the binding's hand-written table said before it was derived from the header, per symbol "return <- arguments" with
# i32 = int, i64 = long long, u64 = unsigned long long / size_t, f64 = double, ptr = any pointer or handle, str = const char*.
# A signature changed on purpose changes its line here.
ABI_KINDS = {
    "bornvi_version": "i32 <-",
    "bornvi_create": "i32 <- i32 ptr",
    "bornvi_destroy": "void <- ptr",
    "bornvi_last_error": "str <- ptr",
    "bornvi_set_option": "i32 <- ptr str i64",
    "bornvi_get_option": "i32 <- ptr str ptr",
    "bornvi_num_params": "i32 <- i32 i32 i32",
    "bornvi_num_gates": "i32 <- i32 i32 i32",
    "bornvi_circuit_workspace_bytes": "u64 <- ptr i32 i32 i32 i32",
    "bornvi_circuit_probs": "i32 <- ptr i32 i32 i32 i32 ptr ptr ptr u64 ptr",
    "bornvi_paramshift_probs": "i32 <- ptr i32 i32 i32 ptr i32 i32 i32 ptr ptr u64 ptr",
    "bornvi_paramshift_probs_strided": "i32 <- ptr i32 i32 i32 ptr i32 i32 i32 i32 ptr ptr u64 ptr",
    "bornvi_paramshift_grad_workspace_bytes": "u64 <- ptr i32 i32 i32 i32 i32",
    "bornvi_paramshift_grad": "i32 <- ptr i32 i32 i32 ptr ptr i32 i32 ptr ptr u64 ptr",
    "bornvi_paramshift_dot_workspace_bytes": "u64 <- ptr i32 i32 i32 i32",
    "bornvi_paramshift_dot_begin": "i32 <- ptr i32 i32 i32 ptr i32 i32 i32 ptr ptr u64 ptr",
    "bornvi_paramshift_dot_finish": "i32 <- ptr i32 i32 i32 i32 ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_gate1q_apply": "i32 <- ptr i32 i64 ptr i32 ptr ptr",
    "bornvi_cnot_apply": "i32 <- ptr i32 i64 ptr i32 i32 ptr",
    "bornvi_born_probs": "i32 <- ptr i32 i64 ptr ptr ptr",
    "bornvi_score_from_cpts": "i32 <- ptr ptr i32 ptr ptr ptr",
    "bornvi_bn_logjoint_samples": "i32 <- ptr ptr i32 i64 ptr f64 ptr ptr",
    "bornvi_bn_score_samples": "i32 <- ptr ptr i32 i64 ptr f64 ptr ptr ptr",
    "bornvi_stein_pairs_workspace_bytes": "u64 <- ptr i32 i64",
    "bornvi_stein_pairs_rowsum": "i32 <- ptr i32 i64 f64 ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_stein_pairs_geometry": "i32 <- i64 ptr ptr",
    "bornvi_stein_gram_build": "i32 <- ptr i32 f64 ptr ptr ptr",
    "bornvi_stein_gram_build_rows": "i32 <- ptr i32 f64 ptr i64 i64 ptr ptr",
    "bornvi_stein_gram_ld": "i64 <- i32",
    "bornvi_stein_gram_build_rows_ld": "i32 <- ptr i32 f64 ptr i64 i64 ptr i64 ptr",
    "bornvi_stein_kp_pairs": "i32 <- ptr i32 f64 i64 ptr ptr ptr ptr ptr ptr",
    "bornvi_stein_quadform_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_stein_quadform": "i32 <- ptr i32 ptr ptr i32 ptr ptr ptr u64 ptr",
    "bornvi_stein_quadform_ld": "i32 <- ptr i32 ptr i64 ptr i32 ptr ptr ptr u64 ptr",
    "bornvi_stein_quadform_sym_workspace_bytes": "u64 <- ptr i32",
    "bornvi_stein_quadform_sym": "i32 <- ptr i32 ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_stein_quadform_sym_ld": "i32 <- ptr i32 ptr i64 ptr ptr ptr ptr u64 ptr",
    "bornvi_stein_sym_strip_rows": "i32 <-",
    "bornvi_stein_quadform_sym_pairs": "i32 <- ptr i32 ptr ptr i64 i64 ptr ptr ptr ptr u64 ptr",
    "bornvi_stein_quadform_sym_pairs_ld": "i32 <- ptr i32 ptr ptr i64 i64 i64 ptr ptr ptr ptr u64 ptr",
    "bornvi_stein_quadform_rows": "i32 <- ptr i32 ptr i64 i64 ptr ptr ptr ptr u64 ptr",
    "bornvi_stein_matvec_kron_workspace_bytes": "u64 <- ptr i32",
    "bornvi_stein_matvec_kron": "i32 <- ptr i32 f64 ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_ksd_grad_finish": "i32 <- ptr i32 ptr i32 ptr ptr ptr ptr ptr ptr",
    "bornvi_shots_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_shots_histogram": "i32 <- ptr i32 i32 ptr ptr i64 u64 ptr i32 i32 i32 ptr u64 ptr",
    "bornvi_born_table_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_born_table_probs": "i32 <- ptr i32 i32 i32 ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_born_table_vjp": "i32 <- ptr i32 i32 i32 ptr ptr ptr ptr f64 ptr ptr ptr u64 ptr",
    "bornvi_reinforce_workspace_bytes": "u64 <- ptr i32 i64",
    "bornvi_reinforce_step": "i32 <- ptr i32 i64 ptr ptr ptr ptr ptr i32 f64 f64 f64 ptr ptr ptr ptr u64 ptr",
    "bornvi_elbo_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_elbo_weights": "i32 <- ptr i32 i32 ptr ptr f64 ptr ptr ptr ptr u64 ptr",
    "bornvi_mps_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_mps_probs": "i32 <- ptr i32 i32 ptr ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_mps_vjp": "i32 <- ptr i32 i32 ptr ptr ptr ptr u64 ptr",
    "bornvi_mps_sample_workspace_bytes": "u64 <- ptr i32 i32 i64",
    "bornvi_mps_environments": "i32 <- ptr i32 i32 i64 ptr ptr ptr u64 ptr",
    "bornvi_mps_sample": "i32 <- ptr i32 i32 i64 ptr u64 ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_mps_score_vjp": "i32 <- ptr i32 i32 i64 ptr ptr ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_fisher_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_fisher_gram": "i32 <- ptr i32 ptr i32 ptr f64 ptr ptr u64 ptr",
    "bornvi_spd_solve_workspace_bytes": "u64 <- ptr i32",
    "bornvi_spd_solve": "i32 <- ptr i32 ptr f64 ptr ptr ptr ptr u64 ptr",
    "bornvi_spd_solve_batched_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_spd_solve_batched": "i32 <- ptr i32 i32 ptr f64 ptr ptr ptr ptr u64 ptr",
    "bornvi_mps_score_rows": "i32 <- ptr i32 i32 i64 ptr ptr i32 i32 i64 ptr ptr ptr u64 ptr",
    "bornvi_score_fisher_workspace_bytes": "u64 <- ptr i32 i32 i64",
    "bornvi_score_fisher_gram": "i32 <- ptr i32 i32 i64 i64 ptr ptr ptr u64 ptr",
    "bornvi_mps_score_sample_gram_workspace_bytes": "u64 <- ptr i32 i32 i64",
    "bornvi_mps_score_sample_gram": "i32 <- ptr i32 i32 i64 ptr ptr ptr ptr ptr u64 ptr u64 ptr",
    "bornvi_mps_score_jvp": "i32 <- ptr i32 i32 i64 ptr ptr ptr f64 ptr ptr ptr u64 ptr",
    "bornvi_mps_query_workspace_bytes": "u64 <- ptr i32 i32 i32",
    "bornvi_mps_log_marginals": "i32 <- ptr i32 i32 i32 ptr ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_mps_sample_clamped": "i32 <- ptr i32 i32 i64 ptr ptr ptr u64 ptr ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_mps_marginals": "i32 <- ptr i32 i32 ptr ptr ptr ptr u64 ptr",
    "bornvi_mps_canon_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_mps_canonicalise": "i32 <- ptr i32 i32 i32 f64 ptr ptr ptr ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_bn_sample": "i32 <- ptr ptr i32 i64 u64 ptr ptr ptr ptr ptr",
    "bornvi_mps_log_marginals_vjp_workspace_bytes": "u64 <- ptr i32 i32 i32",
    "bornvi_mps_log_marginals_vjp_geometry": "i32 <- i32 ptr",
    "bornvi_mps_log_marginals_vjp": "i32 <- ptr i32 i32 i32 ptr ptr ptr ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_cg_init": "i32 <- ptr i64 ptr ptr ptr ptr ptr ptr ptr",
    "bornvi_cg_step": "i32 <- ptr i64 f64 f64 ptr ptr ptr ptr ptr ptr",
    "bornvi_cg_finish": "i32 <- ptr i64 ptr ptr ptr ptr ptr ptr ptr",
    "bornvi_paramshift_states_workspace_bytes": "u64 <- ptr i32 i32 i32 i32",
    "bornvi_paramshift_states": "i32 <- ptr i32 i32 i32 ptr i32 i32 i32 ptr ptr u64 ptr",
    "bornvi_qfi_workspace_bytes": "u64 <- ptr i32 i32",
    "bornvi_qfi_gram": "i32 <- ptr i32 i32 ptr ptr ptr ptr u64 ptr",
    "bornvi_clip_cast_grad": "i32 <- ptr i32 ptr f64 ptr ptr ptr",
    "bornvi_clip_cast_grad_guard": "i32 <- ptr i32 ptr f64 ptr ptr ptr ptr ptr",
    "bornvi_clip_adam_step": "i32 <- ptr i32 ptr f64 ptr ptr ptr ptr ptr ptr ptr ptr i32 f64 f64 f64 ptr ptr ptr ptr",
    "bornvi_adjoint_workspace_bytes": "u64 <- ptr i32 i32 i32",
    "bornvi_adjoint_state": "i32 <- ptr i32 i32 i32 ptr ptr ptr ptr u64 ptr",
    "bornvi_adjoint_vjp": "i32 <- ptr i32 i32 i32 ptr ptr ptr ptr ptr u64 ptr",
    "bornvi_plan_describe": "i64 <- i32 i32 i32 i32 ptr u64",
    "bornvi_plan_param_first_pass": "i32 <- i32 i32 i32 i32 ptr i32",
    "bornvi_plan_fast_describe": "i64 <- i32 i32 i32 i32 ptr u64 ptr i32",
    "bornvi_plan_compact_describe": "i64 <- i32 i32 i32 i32 ptr u64 ptr i32",
}

# Every limit of the header with the literal the Python backend carried before it read them from there, and the backend
# constant that now takes its value from it (None: used by the library only).
ABI_LIMITS = {
    "BORNVI_CIRCUIT_MAX_N": (29, "CIRCUIT_MAX_N"),
    "BORNVI_DENSE_MAX_N": (17, None),
    "BORNVI_DENSE_MAX_LD_PAD": (4096, None),
    "BORNVI_TABLE_MAX_N": (30, None),
    "BORNVI_GATE_MAX_N": (40, None),
    "BORNVI_BN_MAX_NODES": (64, None),
    "BORNVI_BORN_TABLE_MAX_ROWS": (65535, "BORN_TABLE_MAX_ROWS"),
    "BORNVI_ELBO_MAX_ROWS": (65535, "ELBO_MAX_ROWS"),
    "BORNVI_REINFORCE_MAX_BATCH": (1 << 24, "REINFORCE_MAX_BATCH"),
    "BORNVI_SHOTS_MAX": ((1 << 31) - 1, "SHOTS_MAX"),
    "BORNVI_MPS_MAX_N": (26, "MPS_MAX_N"),
    "BORNVI_MPS_MAX_BOND": (32, "MPS_MAX_BOND"),
    "BORNVI_MPS_SAMPLED_MAX_N": (63, "MPS_SAMPLED_MAX_N"),
    "BORNVI_MPS_SAMPLED_MAX_BATCH": (1 << 24, "MPS_SAMPLED_MAX_BATCH"),
    "BORNVI_SCORE_MIN_LD": (64, None),
    "BORNVI_MPS_QUERY_MAX_QUERIES": (1 << 16, "MPS_QUERY_MAX_QUERIES"),
    "BORNVI_STEIN_PAIRS_MAX_B": (1 << 17, "STEIN_PAIRS_MAX_BATCH"),
    "BORNVI_FISHER_MAX_PARAMS": (1024, "FISHER_MAX_PARAMS"),
    "BORNVI_SAMPLE_GRAM_MAX_BATCH": (1024, "SAMPLE_GRAM_MAX_BATCH"),
    "BORNVI_SPD_BATCHED_MAX_SYSTEMS": (65535, None),
    "BORNVI_SCORE_FISHER_MAX_BLOCKS": (65535, None),
    "BORNVI_CG_MAX_PARAMS": ((1 << 31) - 1, "CG_MAX_PARAMS"),
    "BORNVI_CG_STATE_DOUBLES": (8, "CG_STATE_DOUBLES"),
}


def _abi_kind(t):
    import ctypes as C
    if t is None:
        return "void"
    if t is C.c_char_p:
        return "str"
    if t is C.c_void_p or issubclass(t, C._Pointer):
        return "ptr"
    return {C.c_int: "i32", C.c_longlong: "i64", C.c_ulonglong: "u64", C.c_size_t: "u64", C.c_double: "f64"}[t]


def test_prototypes_parsed_from_the_header_are_the_hand_written_ones():
    from tensornetworks_amd import _ext
    parsed = {name: f"{_abi_kind(res)} <- {' '.join(_abi_kind(a) for a in args)}".rstrip()
              for name, (res, args) in _ext.PROTOTYPES.items()}
    assert len(ABI_KINDS) == 99
    assert parsed == ABI_KINDS, {k: (parsed.get(k), ABI_KINDS.get(k)) for k in set(parsed) | set(ABI_KINDS) if parsed.get(k) != ABI_KINDS.get(k)}
    assert _ext.EXPORTED_SYMBOLS == tuple(_ext.PROTOTYPES)
    lib = _ext.lib()
    for name, (res, args) in _ext.PROTOTYPES.items():        # what the loaded functions carry is the parsed table
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args), name
    assert (_ext.BORNVI_OK, _ext.ANSATZ_IDS) == (0, {"hardware_efficient": 0, "all_to_all": 1, "basic": 2})


def test_limits_parsed_from_the_header_are_the_backends_literals():
    from tensornetworks_amd import _ext, backend, born_machine_base
    from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference
    assert _ext.LIMITS == dict({name: value for name, (value, _) in ABI_LIMITS.items()}, BORNVI_VERSION=100)
    for name, (value, constant) in ABI_LIMITS.items():
        if constant is not None:
            assert getattr(backend, constant) == value == _ext.LIMITS[name], (name, constant)
    assert born_machine_base.MAX_EVIDENCE_QUERIES == 1 << 16 and AmortisedMPSInference.MAX_ENUMERATED_OBSERVED == 16


def test_bn_descriptor_fields_are_the_headers():
    from tensornetworks_amd import _ext
    hdr = open(os.path.join(REPO, "include", "bornvi.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} bornvi_bn_desc;", hdr, re.S).group(1)
    members = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert members == [name for name, _ in _ext.BnDesc._fields_] and len(members) == 7


def test_header_parser_refuses_what_it_cannot_map():
    from tensornetworks_amd import _ext
    ok = "#define BORNVI_X 7\nint bornvi_f(bornvi_handle h, const float* w, long long* out);\n"
    assert _ext.parse_header(ok)[0] == {"BORNVI_X": 7} and list(_ext.parse_header(ok)[2]) == ["bornvi_f"]
    with pytest.raises(_ext.BornviError, match=r"float.*int bornvi_f\(bornvi_handle h, float w\);"):
        _ext.parse_header("#define BORNVI_X 7\nint bornvi_f(bornvi_handle h, float w);\n")
    with pytest.raises(_ext.BornviError, match="cannot read"):
        _ext.parse_header("int bornvi_f(int (*callback)(int));\n")


def test_host_only_calls_take_byref_and_arrays():
    """The parser maps every `T*` to c_void_p where the hand-written table had POINTER(T) for a few host-only calls: byref()
    and ctypes arrays still pass."""
    import ctypes as C
    from tensornetworks_amd import _ext
    lib = _ext.lib()
    tiles, ranges, groups = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.bornvi_stein_pairs_geometry(4096, C.byref(tiles), C.byref(ranges)) == 0 and tiles.value > 0 and ranges.value > 0
    assert lib.bornvi_mps_log_marginals_vjp_geometry(300, C.byref(groups)) == 0 and groups.value > 0
    words = _ext.plan_words(0, 5, 2)
    first = (C.c_int * 64)()
    assert lib.bornvi_plan_param_first_pass(0, 5, 2, 0, first, 64) == 30
    assert list(first[:30]) == list(_ext.plan_param_first_pass(words))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_product_fails_loudly_without_gpu():
    from tensornetworks_amd import _ext, backend
    from tensornetworks_amd.quantum_born_machine import QuantumBornMachine
    with pytest.raises(_ext.BornviError):
        _ext.Handle(0)
    with pytest.raises(_ext.BornviError):
        backend.compute_device("cpu")
    bm = QuantumBornMachine(3, 1)
    with pytest.raises(_ext.BornviError, match="no CPU fallback"):
        bm.get_probabilities()


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb", [(1, 1, 0), (2, 3, 0), (3, 4, 0), (5, 2, 0), (6, 3, 4), (7, 2, 5), (9, 2, 6),
                                    (10, 2, 7), (11, 1, 13), (12, 1, 8)])
def test_planner_against_oracle(ansatz, n, L, kb):
    """The pass / stage / micro-op program emitted by the C++ planner, interpreted on NumPy exactly
    as the HIP kernel interprets it, reproduces the oracle's q_theta."""
    from tensornetworks_amd import _ext
    W = _ext.plan_words(_ext.ANSATZ_IDS[ansatz], n, L, kb)
    rng = np.random.default_rng(n * 31 + L)
    th = rng.uniform(-np.pi, np.pi, oc.num_params(ansatz, n, L))
    q = pe.run_plan(W, pe.fused_matrices(W, th))
    np.testing.assert_allclose(q, oc.probs(ansatz, n, L, th), rtol=0, atol=1e-13)
    st = pe.plan_stats(W)
    assert st["gates"] == len(oc.gate_list(ansatz, n, L)) and st["k"] == min(n, kb or 13)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb", [(10, 1, 0), (11, 1, 0), (12, 3, 0), (13, 2, 11), (13, 1, 13), (14, 2, 12), (14, 3, 11)])
def test_fast_tables_against_oracle(ansatz, n, L, kb):
    """The per-(stage, tile, thread) tables the fast pass kernel reads (LDS slots with the CNOT index maps
    folded in, CZ sign bits, slot-offset bases, stage kinds), interpreted as that kernel interprets them."""
    from tensornetworks_amd import _ext
    aid = _ext.ANSATZ_IDS[ansatz]
    W = _ext.plan_words(aid, n, L, kb)
    F, offs = _ext.plan_fast_words(aid, n, L, kb)
    assert F is not None, "plan should be eligible for the fast kernel"
    th = np.random.default_rng(n * 7 + L).uniform(-np.pi, np.pi, oc.num_params(ansatz, n, L))
    q = pe.run_plan(W, pe.fused_matrices(W, th), fast=(F, offs))
    np.testing.assert_allclose(q, oc.probs(ansatz, n, L, th), rtol=0, atol=1e-13)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb,read_map", [(6, 3, 0, 0), (7, 2, 0, 0), (8, 4, 0, 0), (9, 3, 6, 0), (10, 2, 7, 0), (9, 1, 0, 0), (11, 2, 9, 0),
                                             (12, 3, 0, 1), (13, 2, 11, 0), (14, 2, 12, 1), (14, 3, 11, 1), (15, 3, 12, 0)])
def test_r3_plan_and_compact_tables_against_oracle(ansatz, n, L, kb, read_map):
    """The plan with 3 register wires per stage (8 amplitudes per thread, circuit_pass_r3_kernel): (i) its stage headers
    interpreted as the generic kernel does, (ii) its per-(tile row, thread) fast tables, (iii) its COMPACT tables -- every
    word = LANE[row][lane] ^ UNI[tile row][row][wave], sign rows with the bilinear lane x (wave, tile row) term -- run exactly
    as the kernel runs them (direct first / last stages on and off, support of |0..0> on and off) reproduce the oracle."""
    from tensornetworks_amd import _ext
    aid = _ext.ANSATZ_IDS[ansatz]
    flags = kb | _ext.R3 | (0x100 if read_map else 0)
    W = _ext.plan_words(aid, n, L, flags)
    assert int(W[pe.PH_R]) == 3 and int(W[pe.PH_THREADS]) == max(64, 1 << (int(W[pe.PH_K]) - 3))    # (tiles below 2^9: part of one wave)
    th = np.random.default_rng(n * 13 + L).uniform(-np.pi, np.pi, oc.num_params(ansatz, n, L))
    ref = oc.probs(ansatz, n, L, th)
    mats = pe.fused_matrices(W, th)
    np.testing.assert_allclose(pe.run_plan(W, mats), ref, rtol=0, atol=1e-13)
    F, offs = _ext.plan_fast_words(aid, n, L, flags)
    if F is not None:         # (the full tables keep the 16-amplitude kernel's rule "one matrix piece per thread"; the compact ones do not)
        np.testing.assert_allclose(pe.run_plan(W, mats, fast=(F, offs)), ref, rtol=0, atol=1e-13)
    Cw, coffs = _ext.plan_compact_words(aid, n, L, kb | (0x100 if read_map else 0))
    assert Cw is not None and len(coffs) == int(W[pe.PH_NPASSES])
    for direct, zs in ((3, True), (3, False), (0, False)):
        if read_map:
            continue          # (the compact emulator asserts stages without cross reads; those plans are covered on the GPU)
        np.testing.assert_allclose(pe.run_plan_compact(W, (Cw, coffs), mats, direct=direct, zero_support=zs), ref, rtol=0, atol=1e-13)


def test_r3_benchmark_sizes_are_eligible():
    """BASELINE configs 3 and 4 under the 8-amplitude kernel: 2^13 tiles (1024 threads), compact tables within the CU's LDS
    beside the tile; the planner's read map brings the stage count close to the bound of 3 gates per stage."""
    from tensornetworks_amd import _ext
    for n, L, gates in ((16, 6, 96), (20, 8, 160)):
        for rm, max_stages in ((0, 10 ** 6), (0x100, gates // 3 + 8)):
            W = _ext.plan_words(0, n, L, _ext.R3 | rm)
            st = pe.plan_stats(W)
            assert st["k"] == 13 and int(W[pe.PH_THREADS]) == 1024 and sum(st["stages"]) <= max_stages, st
        Cw, coffs = _ext.plan_compact_words(0, n, L, 0)
        assert Cw is not None and len(Cw) * 4 < 4 << 20


def test_zero_support_masks_leave_out_only_zeros():
    """Support of |0..0> (fast tables, FH_ZINFO): the INIT pass leaves out tiles nobody reads, the pass behind it does
    not load slots known to be zero.  The emulator writes NaN where a left-out tile would have gone and computes with 0
    where a slot is not loaded (asserting that only zeros or that poison lie there): the plan still reproduces the
    oracle -- and the masks are really in use at the sizes that matter."""
    from tensornetworks_amd import _ext
    used = 0
    for ansatz, n, L, kb in [("all_to_all", 13, 2, 10), ("hardware_efficient", 14, 3, 10), ("basic", 14, 3, 11),
                             ("hardware_efficient", 13, 3, 10), ("all_to_all", 14, 2, 11)]:
        aid = _ext.ANSATZ_IDS[ansatz]
        W = _ext.plan_words(aid, n, L, kb)
        F, offs = _ext.plan_fast_words(aid, n, L, kb)
        if F is None:                                     # (not eligible for the persistent kernel at this tile size)
            continue
        gmask, zslots = int(F[offs[0] + pe.FH_ZINFO]), int(F[offs[1] + pe.FH_ZINFO])
        assert (gmask == 0) == (zslots == 0)
        used += gmask != 0
        th = np.random.default_rng(n + L).uniform(-np.pi, np.pi, oc.num_params(ansatz, n, L))
        q = pe.run_plan(W, pe.fused_matrices(W, th), fast=(F, offs))
        np.testing.assert_allclose(q, oc.probs(ansatz, n, L, th), rtol=0, atol=1e-13)
    assert used >= 2
    for n, L in ((16, 6), (20, 8)):                      # the benchmark sizes: one resp. 8 of 2^(n-13) tiles written, 2 resp. 1 of 16 slots loaded
        F, offs = _ext.plan_fast_words(0, n, L, 0)
        gmask, zslots = int(F[offs[0] + pe.FH_ZINFO]), int(F[offs[1] + pe.FH_ZINFO])
        assert bin(gmask).count("1") == min(n - 13, 4) and bin(zslots).count("1") == 16 - (16 >> min(n - 13, 4))


def test_fast_tables_eligibility_and_kron():
    from tensornetworks_amd import _ext
    # the first / last stages of multi-pass plans go straight between HBM and registers (coalescing checked by
    # the table builder; the emulator checks the offsets against the ordinary tile fill / drain)
    Wd = _ext.plan_words(0, 14, 3, 11)
    Fd, od = _ext.plan_fast_words(0, 14, 3, 11)
    n_in = sum(int(Fd[int(o) + pe.FH_IN_TAB]) != 0 for o in od)
    n_out = sum(int(Fd[int(o) + pe.FH_OUT_TAB]) != 0 for o in od)
    assert n_in >= 1, (n_in, n_out, len(od))
    assert _ext.plan_fast_words(0, 8, 4, 0) == (None, None)          # tiles below 2^10: generic kernel
    assert _ext.plan_fast_words(0, 10, 2, 0) == (None, None)         # 6 stages x 16 matrix pieces > 64 threads
    assert _ext.plan_fast_words(0, 12, 2, 8) == (None, None)
    for n, L in [(16, 6), (20, 8)]:
        F, offs = _ext.plan_fast_words(0, n, L, 0)
        W = _ext.plan_words(0, n, L, 0)
        assert F is not None and len(offs) == int(W[3]) and len(F) * 4 < 64 << 20
    n, kb = 12, 10
    W = _ext.plan_words(-1, n, 0, kb)
    F, offs = _ext.plan_fast_words(-1, n, 0, kb)
    assert F is not None
    a = np.exp(-1.0 / n)
    M = np.array([[1, a], [a, 1]], dtype=np.complex128)
    rng = np.random.default_rng(n)
    v = rng.normal(size=2 ** n) + 1j * rng.normal(size=2 ** n)
    out = pe.run_plan(W, [M], state_in=v, fast=(F, offs))
    ref = os_.kbase_apply(v.real, n, a) + 1j * os_.kbase_apply(v.imag, n, a)
    np.testing.assert_allclose(out, ref, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("n,kb", [(1, 0), (3, 0), (6, 4), (9, 5), (10, 7), (12, 13)])
def test_kron_plan_against_oracle(n, kb):
    """State-in / state-out program for K_base = M^{(x) n} (matrix-free Stein mat-vec)."""
    from tensornetworks_amd import _ext
    W = _ext.plan_words(-1, n, 0, kb)
    a = np.exp(-1.0 / n)
    M = np.array([[1, a], [a, 1]], dtype=np.complex128)
    rng = np.random.default_rng(n)
    v = rng.normal(size=2 ** n) + 1j * rng.normal(size=2 ** n)
    out = pe.run_plan(W, [M], state_in=v)
    ref = os_.kbase_apply(v.real, n, a) + 1j * os_.kbase_apply(v.imag, n, a)
    np.testing.assert_allclose(out, ref, rtol=1e-13, atol=1e-13)


def test_full_size_plans_are_well_formed():
    from tensornetworks_amd import _ext
    for ansatz_id in (0, 1, 2):
        for n, L in [(16, 6), (20, 8)]:
            W = _ext.plan_words(ansatz_id, n, L, 0)
            st = pe.plan_stats(W)
            # tile size of a multi-tile state: 2^13 wherever the fast kernel can run it (make_plan)
            # (all_to_all at n = 20 carries CZ sign tables in every stage: tile + table rows exceed 160 KiB of LDS -> 2^11)
            assert st["k"] == (11 if (ansatz_id, n) == (1, 20) else 13)
            assert _ext.plan_fast_words(ansatz_id, n, L, 0)[0] is not None
            p11 = pe.plan_stats(_ext.plan_words(ansatz_id, n, L, 11))["passes"]
            p13 = pe.plan_stats(_ext.plan_words(ansatz_id, n, L, 13))["passes"]
            assert st["passes"] == (p13 if st["k"] == 13 else p11) and p13 <= p11
            assert 2 <= st["passes"] <= 3 * L + 2
            assert int(W[8]) == len(W)
    assert _ext.lib().bornvi_plan_describe(0, 31, 1, 0, None, 0) == -1       # n out of range
    assert _ext.lib().bornvi_plan_describe(9, 4, 1, 0, None, 0) == -1        # unknown ansatz


def test_utils_and_network_helpers():
    from tensornetworks_amd import utils as u
    from tensornetworks_amd.bayesian_network import (BayesianNetwork, get_sprinkler_network, pack_network,
                                                      synthetic_network, joint_table)
    assert u.generate_all_binary_outcomes(0) == [()]
    assert u.generate_all_binary_outcomes(1) == [(0,), (1,)]
    assert u.generate_all_binary_outcomes(3) == os_.generate_all_binary_outcomes(3)
    assert all(u.outcome_index(z) == i for i, z in enumerate(u.generate_all_binary_outcomes(5)))
    p1 = {'00': 0.25, '01': 0.25, '10': 0.25, '11': 0.25}
    p2 = {'00': 0.5, '01': 0.1, '10': 0.1, '11': 0.3}
    assert abs(u.calculate_tvd(p1, p2) - 0.3) < 1e-15                                  # utils.py:96-102
    assert abs(u.calculate_tvd(np.array([.25] * 4), np.array([.5, .1, .1, .3])) - 0.3) < 1e-15
    with pytest.raises(ValueError):
        u.calculate_tvd(np.zeros(3), np.zeros(4))
    with pytest.raises(TypeError):
        u.calculate_tvd(p1, np.zeros(4))
    bn = get_sprinkler_network(False)
    assert bn.nodes == ['C', 'S', 'R', 'W'] and bn.parents['W'] == ['S', 'R']
    assert abs(bn.get_joint_probability((1, 0, 1, 1)) - 0.5 * 0.9 * 0.8 * 0.9) < 1e-16
    with pytest.raises(ValueError):
        bn.add_node('C', cpt={})
    with pytest.raises(ValueError):
        BayesianNetwork().add_node('X', cpt={}, parent_names=['nope'])
    with pytest.raises(ValueError):
        bn.get_joint_probability((1, 0))
    g = golden("sprinkler_w1.npz")
    np.testing.assert_array_equal(joint_table(bn, ['C', 'S', 'R'], {'W': 1}), g["pxz"])
    pk = pack_network(bn, ['C', 'S', 'R'], {'W': 1})
    for k in pk:
        np.testing.assert_array_equal(pk[k], g["pack_" + k])
    sb, lat, obs, x = synthetic_network(6, 0)
    assert lat == [f"Z{i}" for i in range(6)] and obs == ["X"] and x == {"X": 1}
    assert sb.parents["Z4"] == ["Z3", "Z2"] and sb.parents["Z5"] == ["Z4"] and sb.parents["X"] == ["Z4", "Z5"]
    sb2, *_ = synthetic_network(6, 0)
    assert sb.cpts == sb2.cpts                                                          # seeded
    hidden = pack_network(bn, ['C', 'R'], {'W': 0})
    assert hidden["role"].tolist() == [0, -3, 1, -1]


def test_shard_ranges_cover_all_parameters():
    from tensornetworks_amd.paramshift_shard import shard_range
    for P in (0, 1, 7, 36, 96, 288, 480):
        for W in (1, 2, 3, 4, 8):
            got = []
            for r in range(W):
                lo, hi = shard_range(P, r, W)
                assert 0 <= lo <= hi <= P
                got += list(range(lo, hi))
            assert got == list(range(P))
    assert shard_range(288, 3, 8) == (108, 144) and shard_range(480, 7, 8) == (420, 480)


def test_interleaved_parameter_deal_and_gather_order():
    """shard_params deals the parameters rank, rank + W, ...; all_gather_grad's re-ordering (rank-major gathered
    buffer -> parameter order) is its exact inverse."""
    import torch
    from tensornetworks_amd.paramshift_shard import shard_params
    for P in (0, 1, 7, 36, 96, 288, 480):
        for W in (1, 2, 3, 4, 8):
            chunk = -(-P // W) if P else 0
            owned = [list(range(*shard_params(P, r, W))) for r in range(W)]
            assert sorted(sum(owned, [])) == list(range(P))
            assert all(len(o) <= chunk for o in owned) and max(map(len, owned)) - min(map(len, owned)) <= 1
            if P == 0:
                continue
            gathered = torch.full((W * chunk,), -1.0, dtype=torch.float64)       # what all_gather_into_tensor delivers
            for r in range(W):
                gathered[r * chunk: r * chunk + len(owned[r])] = torch.tensor(owned[r], dtype=torch.float64)
            full = gathered.view(W, chunk).t().reshape(-1)[:P]
            assert full.tolist() == [float(p) for p in range(P)]



def test_planner_property_random_configurations():
    """Property test: for random (ansatz, n, layers, tile size) the emitted plan reproduces the oracle."""
    from hypothesis import given, settings, strategies as st
    from tensornetworks_amd import _ext

    @settings(max_examples=30, deadline=None, derandomize=True)
    @given(st.sampled_from(oc.ANSATZ_TYPES), st.integers(1, 9), st.integers(0, 3), st.integers(4, 13), st.integers(0, 10 ** 6),
           st.booleans())
    def check(ansatz, n, L, kb, seed, read_map):
        # (bit 8 of the tile-size argument: the planner's `read_map` option -- phase-0 CNOTs on thread-held wires, stages
        # flagged STAGE_CROSS_READ; off in the product, kept correct)
        W = _ext.plan_words(_ext.ANSATZ_IDS[ansatz], n, L, kb | (0x100 if read_map else 0))
        th = np.random.default_rng(seed).uniform(-np.pi, np.pi, oc.num_params(ansatz, n, L))
        q = pe.run_plan(W, pe.fused_matrices(W, th))
        np.testing.assert_allclose(q, oc.probs(ansatz, n, L, th), rtol=0, atol=1e-13)
        assert abs(q.sum() - 1) < 1e-13
    check()


def test_c_port_matches_numpy_oracle():
    from oracle import cpu_port as cp
    if not cp.available():
        pytest.skip("oracle/_build/libcpu_port.so not built (run __graft_entry__.build())")
    rng = np.random.default_rng(1)
    for ansatz in oc.ANSATZ_TYPES:
        th = rng.uniform(-3, 3, (2, oc.num_params(ansatz, 7, 2)))
        q = cp.circuit_probs(ansatz, 7, 2, th)
        for b in range(2):
            np.testing.assert_allclose(q[b], oc.probs(ansatz, 7, 2, th[b]), rtol=0, atol=1e-15)
    g = golden("synthetic_n6_s0.npz")
    K = cp.gram_rows(g["S"], 6, 1.0, 0, 64)
    np.testing.assert_allclose(K, g["K"], rtol=0, atol=3e-15 * np.abs(g["K"]).max())
    q = rng.random(64); q /= q.sum()
    y, part = cp.gemv_rows(K[8:24], 6, 8, 24, q)
    np.testing.assert_allclose(y, K[8:24] @ q, rtol=1e-14)
    assert abs(part - q[8:24] @ (K[8:24] @ q)) < 1e-12 * abs(part)
    pr, used = cp.paramshift_probs("basic", 5, 2, th[0][:20], 2, 4, True)
    tp = th[0][:20].copy(); tp[3] -= np.pi / 2
    np.testing.assert_allclose(pr[4], oc.probs("basic", 5, 2, tp), atol=1e-15)
    assert pr.shape == (5, 32) and used >= 1
    # matrix-free K_p q (the CPU baseline's contraction at n = 20) == dense closed form == NumPy Kronecker oracle
    from oracle import stein as os_
    yk, k2 = cp.kron_matvec(g["S"], q, 6, 1.0)
    np.testing.assert_allclose(yk, g["K"] @ q, rtol=0, atol=1e-13 * np.abs(g["K"] @ q).max())
    np.testing.assert_allclose(yk, os_.stein_matvec_kron(g["S"], q, 6, 1.0), rtol=0, atol=1e-13 * np.abs(yk).max())
    assert abs(k2 - q @ g["K"] @ q) <= 1e-12 * abs(k2)


def test_param_first_pass_from_plan_words():
    """Every parameter is touched by some pass, single-pass plans share nothing, and with several passes the early
    layers' parameters come first (parameters are numbered layer by layer): the ordering prefix sharing relies on."""
    from tensornetworks_amd import _ext
    W = _ext.plan_words(_ext.ANSATZ_IDS["hardware_efficient"], 10, 3)
    assert int(W[3]) == 1 and not _ext.plan_param_first_pass(W).any()
    for ansatz, n, L in (("hardware_efficient", 16, 6), ("basic", 15, 3), ("all_to_all", 14, 2)):
        W = _ext.plan_words(_ext.ANSATZ_IDS[ansatz], n, L)
        fp = _ext.plan_param_first_pass(W)
        npass = int(W[3])
        assert fp.shape == (int(W[5]),) and fp.min() == 0 and fp.max() <= npass - 1
        assert len(set(fp.tolist())) > 1
        per_layer = fp.reshape(L, -1) if ansatz != "all_to_all" else None
        if per_layer is not None:       # the mean first pass grows with the layer
            m = per_layer.mean(axis=1)
            assert all(m[i] <= m[i + 1] for i in range(L - 1))


def test_first_pass_rule_is_the_librarys():
    """The parser bench.py uses for its byte accounting (_ext.plan_param_first_pass on the serialised plan) and the
    planner's own Plan::param_first_pass (what prefix sharing orders the batch by) are the same numbers."""
    import ctypes as C
    from tensornetworks_amd import _ext
    L_ = _ext.lib()
    for ansatz, n, L in (("hardware_efficient", 16, 6), ("hardware_efficient", 20, 8), ("basic", 15, 3), ("all_to_all", 14, 2),
                         ("hardware_efficient", 10, 3)):
        aid = _ext.ANSATZ_IDS[ansatz]
        P = L_.bornvi_plan_param_first_pass(aid, n, L, 0, None, 0)
        assert P == len(_ext.plan_param_first_pass(_ext.plan_words(aid, n, L)))
        buf = (C.c_int * P)()
        assert L_.bornvi_plan_param_first_pass(aid, n, L, 0, buf, P) == P
        assert list(buf) == _ext.plan_param_first_pass(_ext.plan_words(aid, n, L)).tolist()
    assert L_.bornvi_plan_param_first_pass(99, 8, 2, 0, None, 0) == -1


def test_trainer_rejects_mismatched_latent_count():
    """qbm_num_latent_vars != len(latent_vars_names) would make the device kernels read S [2^m, m] as [2^n, n]
    (an out-of-bounds read): refused in the constructor, before anything touches a device."""
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    with pytest.raises(ValueError, match="must equal len"):
        KSDVariationalInference(get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], qbm_num_latent_vars=4)


def test_overlap_modes_are_retired():
    """The overlap stream modes are gone: what the benchmark record still reads stays (overlap_streams is False and
    takes False / None, overlap_choice is None), every other mode is refused, and there is no choose_overlap."""
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    vi = KSDVariationalInference(get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], qbm_num_latent_vars=3)
    assert vi.overlap_streams is False
    for mode in (False, None):
        vi.overlap_streams = mode
        assert vi.overlap_streams is False
    for mode in (True, "partition"):
        with pytest.raises(ValueError, match="retired"):
            vi.overlap_streams = mode
        assert vi.overlap_streams is False
    assert vi.overlap_choice is None
    assert not hasattr(vi, "choose_overlap")


@pytest.mark.parametrize("mode,n,dense", [("auto", 1, True), ("auto", 12, True), ("auto", 16, True), ("auto", 17, False),
                                          ("auto", 29, False), ("dense", 12, True), ("dense", 17, True), ("kron", 3, False),
                                          ("kron", 16, False)])
def test_gram_layout_from_plain_values(mode, n, dense):
    """The form of K_p that _prepare_stein settles and the contraction follows, for every rank of 1 ... 8: "auto" is dense
    up to n = 16, "dense" / "kron" override; one rank: symmetric or full; several ranks: strip pairs exactly where
    backend.sym_pair_shard cuts 2^n into whole pairs (symmetric contraction only), else row blocks."""
    from tensornetworks_amd import backend
    from tensornetworks_amd.stein_operator import gram_layout
    for symmetric in (True, False):
        for W in (1, 2, 3, 4, 8):
            for rank in range(W):
                if not dense:
                    want = "kron"
                elif W == 1:
                    want = "sym" if symmetric else "full"
                elif symmetric and backend.sym_pair_shard(n, rank, W) is not None:
                    want = "pairs"
                else:
                    want = "rows"
                assert gram_layout(mode, n, symmetric, rank, W) == want, (symmetric, rank, W)


def test_stein_state_is_set_by_the_constructors():
    """Every attribute the Stein path reads exists right after construction, without a GPU: on a SteinOperator of its
    own, on the quantum trainer (which derives from it) and on the classical trainer's operator."""
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    from tensornetworks_amd.ksd_vi import KSDVariationalInference as ClassicalKSD
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference as QuantumKSD
    from tensornetworks_amd.stein_operator import SteinOperator
    bn, lat, obs = get_sprinkler_network(False), ['C', 'S', 'R'], ['W']
    classical = ClassicalKSD(bn, lat, obs, born_machine_config={'use_logits': True, 'conditioning_dim': 0})
    quantum = QuantumKSD(bn, lat, obs, qbm_num_latent_vars=3)
    assert isinstance(quantum, SteinOperator) and type(classical._stein) is SteinOperator
    for op in (SteinOperator(bn, lat, 1.0, "cpu"), quantum, classical._stein):
        state = vars(op)
        for name in ("_S", "_K", "_K_rows", "_K_pairs", "_K_sig", "_stein_key", "gram_placement", "timers"):
            assert name in state and state[name] is None, name
        assert state["gram_placement_tries"] == 4 and state["symmetric_contraction"] is True
        assert state["_score_function_cache"] == {} and state["num_latent_vars"] == 3
        assert op.gram_mode == "auto" and op.base_kernel_length_scale == 1.0 and op.latent_vars_names == lat
    with pytest.raises(ValueError, match="gram_mode must be 'auto', 'dense' or 'kron'"):
        SteinOperator(bn, lat, 1.0, "cpu", gram_mode="sparse")
    with pytest.raises(ValueError, match="gram_mode must be 'auto', 'dense' or 'kron'"):
        QuantumKSD(bn, lat, obs, qbm_num_latent_vars=3, gram_mode="sparse")


def test_bench_refuses_a_world_size_that_is_not_gpus(monkeypatch):
    """bench.py --gpus N under a launcher that started a different number of ranks exits non-zero (before any GPU call)
    instead of measuring the wrong job with a note on stderr."""
    import bench
    monkeypatch.setenv("WORLD_SIZE", "3")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "2"])
    assert "WORLD_SIZE=3" in str(e.value)


def test_reinforce_step_against_the_reference_trace():
    """The Born-machine (REINFORCE) step of the adversarial trainer against a trace captured from the reference's own
    train() (adversarial_vi.py:184-231; tests/golden/make_golden.py: reinforce_trace -- sample indices, classifier logits,
    log p(x|z), log q, running baseline and loss_q of 4 epochs): the build's reward / baseline / loss arithmetic, fed the
    reference's per-step inputs, reproduces the reference's baseline and loss_q; log q comes from the build's own
    expression log(clamp(q, 1e-9))[index] on the reference's q (quantum_born_machine.py:180-201)."""
    import torch
    from tensornetworks_amd.adversarial_vi import AdversarialVariationalInference as A
    g = golden("reinforce_trace.npz")
    decay = float(g["baseline_decay"])
    baseline = torch.zeros(())
    for e in range(len(g["loss_q"])):
        logits, log_p = torch.tensor(g["logits"][e]), torch.tensor(g["log_p"][e])
        idx = torch.tensor(g["idx"][e], dtype=torch.long)
        log_q = torch.log(torch.tensor(g["q"][e]).clamp(min=1e-9))[idx]
        np.testing.assert_allclose(log_q.numpy(), g["log_q"][e], rtol=1e-6, atol=1e-7)
        rr = A._reinforce_reward(logits, log_p, baseline, e == 0, decay)
        loss_q = A._reinforce_loss(log_q, rr)
        assert abs(baseline.item() - g["baseline"][e]) <= 1e-6 * abs(g["baseline"][e])
        assert abs(loss_q.item() - g["loss_q"][e]) <= 1e-6 * max(1.0, abs(g["loss_q"][e])), (e, loss_q.item(), g["loss_q"][e])


def test_cosine_schedule_table_follows_torch():
    """DeviceAdam tabulates CosineAnnealingLR by its closed form: equal to the scheduler's own (recursive) values to
    rounding, beyond T_max as well (the bench replays more steps than T_max)."""
    import torch
    from tensornetworks_amd.ksd_vi_quantum import cosine_annealing_lr
    for lr0, T, eta in ((0.05, 7, 0.005), (0.005, 1285, 0.0005), (0.1, 1, 0.0)):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=lr0)
        sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T, eta_min=eta)
        want = [lr0]
        for _ in range(min(3 * T + 5, 4000)):
            opt.step()
            sch.step()
            want.append(sch.get_last_lr()[0])
        got = cosine_annealing_lr(np.arange(len(want)), lr0, T, eta)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-15)
        assert cosine_annealing_lr(0, lr0, T, eta) == lr0


@pytest.mark.parametrize("aid", [-1, 0, 1, 2])
def test_every_accepted_n_has_a_plan(aid):
    """The route get_plan takes yields a plan for every n the backend accepts for circuits and the kron mat-vec, and
    none above: the 8-amplitude plan (compact tables) up to n = 27, the 4-wire plan (fast or generic kernel) beyond.
    2^11 tiles leave a 17-bit workgroup index at n = 28, so the 4-wire fallback must keep 2^13 tiles there."""
    from tensornetworks_amd import _ext, backend
    lib = _ext.lib()
    assert backend.CIRCUIT_MAX_N == 29

    def compact(n, L):
        return lib.bornvi_plan_compact_describe(aid, n, L, _ext.R3, None, 0, None, 0)

    for n in range(17, 31):
        for L in ((0,) if aid == -1 else (0, 1, 2)):
            if n <= 27:
                st = pe.plan_stats(_ext.plan_words(aid, n, L, _ext.R3))
                assert st["k"] <= 13 and n - st["k"] <= 16, (aid, n, L, st["k"])
                # (the compact tables take seconds per plan at n >= 24: built at both ends of their range only)
                if n in (17, 27) and L <= 1:
                    assert compact(n, L) > 0, (aid, n, L)
            elif n <= backend.CIRCUIT_MAX_N:
                W = _ext.plan_words(aid, n, L, 0)
                st = pe.plan_stats(W)
                assert st["k"] <= 13 and n - st["k"] <= 16 and int(W[1]) == n, (aid, n, L, st["k"])
                if aid >= 0:
                    assert st["k"] == 13 and st["gates"] == lib.bornvi_num_gates(aid, n, L)
                assert compact(n, L) == 0        # (the 8-amplitude route refuses it: get_plan takes this plan)
            else:
                with pytest.raises(_ext.BornviError):
                    _ext.plan_words(aid, n, L, 0)
                assert compact(n, L) == -1


def test_circuit_entry_points_refuse_n_above_the_planner_range():
    """n = 30 is refused by the argument checks, before a handle or a GPU is needed."""
    import torch
    from tensornetworks_amd import _ext, backend
    t = torch.zeros(1, dtype=torch.float64)
    calls = [lambda: backend.circuit_probs("basic", 30, 1, t.reshape(1, 1)),
             lambda: backend.paramshift_probs("basic", 30, 1, t, 0, 1),
             lambda: backend.paramshift_dot_begin("basic", 30, 1, t, 0, 1),
             lambda: backend.paramshift_grad("basic", 30, 1, t, t, 0, 1),
             lambda: backend.adjoint_state("basic", 30, 1, t),
             lambda: backend.adjoint_vjp("basic", 30, 1, t, t, t),
             lambda: backend.stein_matvec_kron(t, t, 30)]
    for f in calls:
        with pytest.raises(_ext.BornviError, match="out of range"):
            f()
