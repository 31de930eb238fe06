"""The plans that change when diagonal gates commute in the planner (csrc/plan.cpp, "Commutation rule"), on the GPU:
hardware_efficient n = 14, L = 3 and n = 15, L = 2 with the default tiles, the smallest multi-tile plans that change (stages
7 7 3 -> 8 6 3 and 7 4 -> 8 3 with three register wires).  Each case runs under both pass kernels (reg_wires 3 and 4) in a
FRESH process whose first GPU work it is (tests/plan_commute_worker.py: a stage that reads across thread groups without its
barrier was wrong only on a cold GPU):

  * the base row and six shifted rows per entry, under the bound of test_gpu_circuit_precision.py (ratio of 1 against the
    long-double reference of circuit_hp.py, constants of the plan that ran), and against the oracle's C port within that bound
    plus the port's own (circuit_hp.oracle_constants: the difference of two fp64 results may use both);
  * every row of the batch sums to 1;
  * prefix sharing on and off: the whole batch bit for bit;
  * the fused dot (8-amplitude kernel only) against the gradient of the stored rows: q and loss bitwise, gradient to 1e-12
    of its largest entry, the tolerance of that pair in test_gpu_fused_dot_pass.py and test_gpu_r3_spread.py."""
import numpy as np
import pytest

import circuit_hp as ch
import plan_commute_worker
import plan_emulator as pe
from conftest import golden, run_ranks
from oracle import circuit as oc, cpu_port as cp

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ch.unavailable() is not None, reason=str(ch.unavailable()))]
ANSATZ = "hardware_efficient"
CASES = [(14, 3, [8, 6, 3]), (15, 2, [8, 3])]


def test_the_cases_are_plans_that_changed():
    """No GPU work: the stage counts this file was written for (the parent's are in tests/golden/plan_shapes_parent.npz)."""
    from tensornetworks_amd import _ext
    parent = golden("plan_shapes_parent.npz")["stages"]
    for n, L, want in CASES:
        st = pe.plan_stats(_ext.plan_words(0, n, L, _ext.R3 | 0x100))["stages"]
        was = [int(s) for s in parent[0, n - 8, L - 1, 0, 1] if s >= 0]
        assert st == want and was != st and len(was) == len(st) and sum(was) >= sum(st), (n, L, was, st)


@pytest.mark.parametrize("reg_wires", [3, 4])
@pytest.mark.parametrize("n,L,stages", CASES)
def test_cold_process_rows_dot_and_prefix_sharing(tmp_path, n, L, stages, reg_wires):
    from tensornetworks_amd import _ext
    codes = run_ranks(plan_commute_worker.cold_rows, 1, (n, L, reg_wires, str(tmp_path)), timeout=300)
    errs = [p.read_text() for p in tmp_path.glob("*.err")]
    assert codes == [0], (codes, errs)
    res = np.load(tmp_path / f"cold_{n}_{L}_{reg_wires}.npz")
    flags = 0x100 if reg_wires == 3 else 0                     # the read map is on with three register wires (PlanOptions)
    r3 = reg_wires == 3 and _ext.plan_compact_words(0, n, L, flags)[0] is not None
    assert r3 == (reg_wires == 3)
    C = ch.plan_constants(ANSATZ, n, L, "r3" if r3 else "r4", flags)
    O = ch.oracle_constants(ANSATZ, n, L)
    theta = res["theta"]
    thetas = [theta] + [ch.shifted(theta, int(p_), s) for p_ in res["picks"] for s in (np.pi / 2, -np.pi / 2)]
    rows = res["rows"]
    assert np.isfinite(rows).all() and float(res["worst_sum"]) < 1e-12
    port = cp.circuit_probs(ANSATZ, n, L, np.stack(thetas)) if cp.available() else None
    worst, worst_port = 0.0, 0.0
    for b, t in enumerate(thetas):
        ref = ch.cached_reference(ANSATZ, n, L, t)
        worst = ch.fold(worst, ch.worst_ratio(ch.q_ratio(rows[b], ref, C["C_psi"], C["C_q"])), ch.sum_ratio(rows[b], ref, C["C_psi"], C["C_q"]))
        if port is not None:
            both = ch.q_allowed(ref, C["C_psi"], C["C_q"]) + ch.q_allowed(ref, O["C_psi"], O["C_q"])
            worst_port = ch.fold(worst_port, ch.worst_ratio(ch.allowed_ratio(rows[b], port[b], both)))
    print(f"n={n} L={L} reg_wires={reg_wires} [{C['n_passes']} passes, {C['n_fused']} fused gates, C_psi {C['C_psi']:.0f}, C_q {C['C_q']:.0f}]"
          f" worst ratio of 1: long double {worst:.3g}, C port {worst_port:.3g}")
    assert worst <= 1.0 and worst_port <= 1.0
    assert str(res["digest"]) == str(res["digest_shared"])     # prefix sharing: the same bits, all 2 P + 1 rows
    assert bool(res["fused"]) == r3
    if r3:
        gf, gu = res["grad_fused"], res["grad_stored"]
        print(f"   fused dot vs stored rows: largest |dg| {np.abs(gf - gu).max():.3g}, largest |g| {np.abs(gu).max():.3g}")
        assert bool(res["q_equal"]) and bool(res["loss_equal"])
        assert np.abs(gf - gu).max() <= 1e-12 * np.abs(gu).max()
