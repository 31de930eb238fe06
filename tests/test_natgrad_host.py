"""Host checks of the natural-gradient feature: the float64 mirror (natgrad_mirror.py) against known answers and Gram
identities through oracle/circuit.py, the recorded Sprinkler run, and the trainers' argument refusals (no GPU)."""
import numpy as np
import pytest

import elbo_mirror as em
import natgrad_mirror as nm
from conftest import golden
from oracle import circuit as oc
from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network


def basic_fisher(n):
    theta = np.random.default_rng(n).uniform(0.3, 1.2, 2 * n)       # (RY_i, RZ_i) per qubit: sin(theta_RY) != 0
    q = oc.probs("basic", n, 1, theta)
    return nm.fisher(nm.shifted_rows("basic", n, 1, theta), q), q


@pytest.mark.parametrize("n", [1, 3])
def test_basic_ansatz_has_the_known_fisher_matrix(n):
    """RY on |0> has classical Fisher information exactly 1; the closing RZ and the CNOT ring only permute |psi|^2."""
    F, _ = basic_fisher(n)
    np.testing.assert_allclose(F, np.diag([1.0, 0.0] * n), rtol=0, atol=1e-12)


@pytest.mark.parametrize("n", [1, 3])
def test_singular_fisher_is_solvable_with_damping_only(n):
    F, _ = basic_fisher(n)
    g = np.random.default_rng(7).standard_normal(2 * n)
    lam = 1e-3
    x, info = nm.spd_solve(F, g, lam)
    assert info == 0
    np.testing.assert_allclose(x[0::2], g[0::2] / (1 + lam), rtol=1e-9)
    np.testing.assert_allclose(x[1::2], g[1::2] / lam, rtol=1e-9)
    F0 = np.diag([1.0, 0.0] * n)                                    # exactly singular: pivot 1 is 0
    x, info = nm.spd_solve(F0, g, 0.0)
    assert info == 2 and np.array_equal(x, g)


def test_mirror_solve_status_rule():
    A = np.array([[4.0, 2.0], [999.0, 3.0]])                        # the lower triangle is not read
    x, info = nm.spd_solve(A, np.array([2.0, 1.0]))
    assert info == 0
    np.testing.assert_allclose(np.array([[4.0, 2.0], [2.0, 3.0]]) @ x, [2.0, 1.0], rtol=1e-14)
    b = np.array([1.0, -2.0])
    x, info = nm.spd_solve(np.diag([1.0, -1.0]), b)
    assert info == 2 and np.array_equal(x, b)
    x, info = nm.spd_solve(np.array([[np.nan, 0.0], [0.0, 1.0]]), b)
    assert info == 1 and np.array_equal(x, b)
    bad = np.array([1.0, np.inf])
    x, info = nm.spd_solve(np.eye(2), bad)
    assert info == 3 and np.array_equal(x, bad)


def test_gram_identities():
    """hardware_efficient, n = 4, L = 2: the explicit sum, symmetry, positive semi-definiteness."""
    ansatz, n, L = "hardware_efficient", 4, 2
    theta = np.random.default_rng(2).standard_normal(oc.num_params(ansatz, n, L))
    q = oc.probs(ansatz, n, L, theta)
    rows = nm.shifted_rows(ansatz, n, L, theta)
    F = nm.fisher(rows, q)
    P = theta.size
    ref = np.zeros((P, P))
    for a in range(P):
        for b in range(P):
            ref[a, b] = sum(0.25 * (rows[2 * a, z] - rows[2 * a + 1, z]) * (rows[2 * b, z] - rows[2 * b + 1, z]) / q[z]
                            for z in range(1 << n) if q[z] >= nm.Q_FLOOR)
    np.testing.assert_allclose(F, ref, rtol=0, atol=1e-13 * np.abs(ref).max())
    np.testing.assert_allclose(F, F.T, rtol=0, atol=1e-15 * np.abs(F).max())
    assert np.linalg.eigvalsh(0.5 * (F + F.T)).min() >= -1e-12 * np.trace(F)
    # the floor: a state under it contributes nothing
    q2 = q.copy()
    q2[5] = 1e-30
    rows2 = rows.copy()
    rows2[:, 5] = 0.0
    np.testing.assert_array_equal(nm.fisher(rows, q2), nm.fisher(rows2, q2))


def test_sprinkler_mirror_run_is_the_recorded_trace_and_has_its_margin():
    h, th0 = nm.sprinkler_run()
    g = golden("natgrad_sprinkler_trace.npz")
    np.testing.assert_array_equal(g["theta0"], th0)
    np.testing.assert_allclose(h["loss_elbo"], g["loss_elbo"], rtol=1e-7)
    np.testing.assert_allclose(h["theta"][-1], g["theta_final"], rtol=0, atol=1e-6)
    assert max(h["natgrad_info"]) == 0
    assert h["kl"][-1] * nm.KL_MARGIN < nm.KL_THRESHOLD and min(h["kl"]) >= -1e-12


def trainers():
    from tensornetworks_amd.elbo_vi_quantum import ELBOVariationalInference
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    return KSDVariationalInference, ELBOVariationalInference


@pytest.mark.parametrize("which", [0, 1])
def test_trainer_argument_refusals(which):
    from tensornetworks_amd.natural_gradient import FisherPreconditioner
    cls = trainers()[which]
    bn, lat, obs = get_sprinkler_network(False), ['C', 'S', 'R'], ['W']
    vi = cls(bn, lat, obs, 3, 2, natural_gradient=True)
    assert isinstance(vi.natural_gradient, FisherPreconditioner) and vi.natural_gradient.damping == 1e-3
    assert vi._extra_keys[-1] == 'natgrad_info'
    with pytest.raises(ValueError, match="adjoint"):
        vi.grad_engine = "adjoint"
    assert vi.grad_engine == "paramshift"
    assert cls(bn, lat, obs, 3, 2, natural_gradient=0.5).natural_gradient.damping == 0.5
    own = FisherPreconditioner(damping=0.0, q_floor=1e-12)
    assert cls(bn, lat, obs, 3, 2, natural_gradient=own).natural_gradient is own
    if which == 0:
        with pytest.raises(ValueError, match="histograms"):
            cls(bn, lat, obs, 3, 2, qbm_shots=100, shot_seed=1, natural_gradient=True)
    bn4, lat4, obs4, _ = synthetic_network(4, 0)
    with pytest.raises(ValueError, match="1024"):
        cls(bn4, lat4, obs4, 4, 100, natural_gradient=True)          # P = 1200
    for bad in ("yes", -1.0, float("nan")):
        with pytest.raises(ValueError):
            cls(bn, lat, obs, 3, 2, natural_gradient=bad)
    with pytest.raises(ValueError):
        FisherPreconditioner(q_floor=0.0)


@pytest.mark.parametrize("which", [0, 1])
def test_default_path_builds_no_preconditioner(which):
    cls = trainers()[which]
    bn, lat, obs = get_sprinkler_network(False), ['C', 'S', 'R'], ['W']
    for vi in (cls(bn, lat, obs, 3, 2), cls(bn, lat, obs, 3, 2, natural_gradient=None)):
        assert vi.natural_gradient is None and vi._natgrad_extras() == ()
        assert 'natgrad_info' not in vi._extra_keys and vi._extra_keys == type(vi)._extra_keys
        vi.grad_engine = "adjoint"                                   # still allowed
        assert vi.grad_engine == "adjoint"
