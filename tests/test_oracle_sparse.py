"""The sparse exact circuit oracle (oracle/sparse_circuit.py) against the dense one (oracle/circuit.py).  CPU only."""
import numpy as np
import pytest

from oracle import circuit as oc, sparse_circuit as sc


def _dense_from_sparse(n, idx, p):
    q = np.zeros(1 << n)
    q[idx] = p
    return q


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L", [(1, 1), (2, 2), (3, 3), (5, 2), (7, 1), (8, 2)])
def test_dense_random_theta(ansatz, n, L):
    """Fully random angles: the support is all of 2^n, so every split and merge path runs."""
    rng = np.random.default_rng(100 * n + L)
    th = rng.uniform(-np.pi, np.pi, oc.num_params(ansatz, n, L))
    idx, p = sc.probs_sparse(ansatz, n, L, th)
    assert np.all(np.diff(idx) > 0)
    np.testing.assert_allclose(_dense_from_sparse(n, idx, p), oc.probs(ansatz, n, L, th), rtol=0, atol=1e-14)
    idx_s, amp = sc.state_sparse(ansatz, n, L, th)
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[idx_s] = amp
    np.testing.assert_allclose(psi, oc.simulate(oc.gate_list(ansatz, n, L), n, th), rtol=0, atol=1e-14)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("L", [0, 1, 2, 3])
@pytest.mark.parametrize("n,g", [(4, 3), (9, 5), (12, 6)])
def test_sparse_families(ansatz, n, L, g):
    rng = np.random.default_rng(1000 * n + 10 * L + g)
    th, generic = sc.sparse_theta(ansatz, n, L, rng, g=g)
    assert len(generic) == (min(g, n) if L else 0) and len(set(generic)) == len(generic)
    idx, p = sc.probs_sparse(ansatz, n, L, th)
    # (L = 0 of hardware_efficient / all_to_all is H on every wire: the uniform state, no rotation to make it sparse)
    assert idx.size <= (1 << n if L == 0 and ansatz != "basic" else 1 << len(generic))
    q = oc.probs(ansatz, n, L, th)
    np.testing.assert_allclose(_dense_from_sparse(n, idx, p), q, rtol=0, atol=1e-14)
    assert abs(p.sum() - 1.0) < 1e-13
    # nothing off the support: the dense oracle's mass there is rounding only
    off = np.ones(1 << n, dtype=bool)
    off[idx] = False
    assert q[off].max(initial=0.0) <= 1e-28


def test_support_bound_at_large_n():
    """The support stays at most 2^g however large n is (no 2^n array is ever formed)."""
    rng = np.random.default_rng(7)
    for ansatz in oc.ANSATZ_TYPES:
        for n, L, g in [(29, 2, 10), (40, 1, 8), (60, 3, 12)]:
            th, generic = sc.sparse_theta(ansatz, n, L, rng, g=g)
            idx, p = sc.probs_sparse(ansatz, n, L, th)
            assert idx.size <= 1 << g and len(generic) == g
            assert idx.min() >= 0 and idx.max() < (1 << n)
            assert abs(p.sum() - 1.0) < 1e-12
    # the generic rotations reach both ends of the index: high and low bits both vary over the support
    th, _ = sc.sparse_theta("hardware_efficient", 29, 2, np.random.default_rng(3), g=8)
    idx, _ = sc.probs_sparse("hardware_efficient", 29, 2, th)
    varying = np.bitwise_or.reduce(idx ^ idx[0])
    assert varying >> 27 and varying & 0x3


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
def test_shifted_rows_match_dense(ansatz):
    """+-pi/2 shifts of monomial and generic gates: the sparse oracle gives the dense oracle's shifted rows and gradient."""
    n, L = 7, 2
    rng = np.random.default_rng(11)
    th, generic = sc.sparse_theta(ansatz, n, L, rng, g=3)
    monomial = [p for p in range(th.size) if p not in generic]
    params = generic[:2] + list(rng.choice(monomial, 4, replace=False))
    w = rng.standard_normal(1 << n)
    for p, ((ip, qp), (im, qm)) in zip(params, sc.paramshift_sparse(ansatz, n, L, th, params)):
        (tp, tm), = sc.shifted_thetas(th, [p])
        dp, dm = oc.probs(ansatz, n, L, tp), oc.probs(ansatz, n, L, tm)
        np.testing.assert_allclose(_dense_from_sparse(n, ip, qp), dp, rtol=0, atol=1e-14)
        np.testing.assert_allclose(_dense_from_sparse(n, im, qm), dm, rtol=0, atol=1e-14)
        g_sparse = 0.5 * (w[ip] @ qp - w[im] @ qm)
        assert abs(g_sparse - 0.5 * w @ (dp - dm)) <= 1e-13 * np.abs(w).max()


def test_rejects_wrong_theta_length():
    with pytest.raises(ValueError):
        sc.state_sparse("basic", 4, 1, np.zeros(3))
