"""The sampled KSD estimator on the host: the mirror (ksd_sampled_mirror.py) against the fp64 oracle, the Gram arrangement the
row-sum kernel evaluates and its amplification factor, the weights' zero sum, the estimator's unbiasedness by exact
enumeration of every sample tuple, and the trainer's constructor."""
import itertools
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import ksd_sampled_mirror as km
from oracle import stein as os_
from tensornetworks_amd import backend
from tensornetworks_amd.backend import bn_score_samples, stein_pairs_rowsum  # noqa: F401  (fails at import without the feature)


def _networks():
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
    yield "sprinkler", get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], {'W': 1}
    for n in (1, 2, 4, 5):
        bn, lat, obs, x = synthetic_network(n, 0)
        yield f"synthetic{n}", bn, lat, obs, x


def test_mirror_equals_the_oracle():
    """kappa and the scores of the mirror at sampled indices (with repeats) equal oracle.stein's gram_closed_form[idx][:, idx]
    and score_matrix[idx]; the oracle is fp64, so to its own error: gram_constant x EPS64 x B~ per entry, and
    (2 V + 2) EPS64 (1 + |ratio|) for a score."""
    from tensornetworks_amd.bayesian_network import pack_network
    rng = np.random.default_rng(0)
    for name, bn, lat, obs, x in _networks():
        n = len(lat)
        packed = pack_network(bn, lat, x)
        idx = np.concatenate([rng.integers(0, 1 << n, 9), [0, (1 << n) - 1, 0]])
        S_o = os_.score_matrix(bn, x, lat, obs)
        assert np.all(os_.joint_vector(bn, x, lat) >= 1e-12)          # (no zeroed row: the two conventions agree)
        S, R, k = km.scores(packed, idx, n)
        V = len(packed["role"])
        assert np.all(np.abs(hp.to_f64(S - hp.arithmetic().arr(S_o[idx]))) <= (2 * V + 2) * hp.EPS64 * hp.to_f64(1 + R)), name
        assert np.all(k >= 1) and np.all(k <= V)
        for ls in (1.0, 0.37):
            K, Bt, d = km.kappa_bound(idx, S_o[idx], n, ls)
            K_o = os_.gram_closed_form(S_o, n, ls)[idx][:, idx]
            r = hp.ratio(K_o, K, Bt * hp.gram_constant(n, d))
            assert hp.worst(r)[0] <= 1.0, (name, ls, hp.worst(r))
            K4, _ = km.kappa(idx, S_o[idx], n, ls)
            assert hp.worst(hp.ratio(hp.to_f64(K4), K, Bt))[0] <= 2.0, (name, ls)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 16, 40, 63])
def test_gemm_identity_and_amplification(n):
    """The arrangement of kernels_ksd_sampled.hip equals the closed form in extended precision, and the sum of the absolute
    values of its terms is at most 4 x the closed form's (B~) wherever n l >= 1: l in {1, 1/n, 0.37 if n >= 3}, score scales
    0.01, 1, 30 and a row-wise mix of them."""
    X = hp.arithmetic()
    eps_x = float(np.finfo(np.longdouble).eps) if X.name == "longdouble" else 1e-38
    rng = np.random.default_rng(n)
    B = 24 if X.name == "longdouble" else 6          # (mpmath on object arrays is slow: fewer samples, every n all the same)
    idx = rng.integers(0, 1 << n, B, dtype=np.int64)
    idx[:3] = [0, (1 << n) - 1, 0]
    worst_amp = 0.0
    for ls in [1.0, 1.0 / n] + ([0.37] if n >= 3 else []):
        assert n * ls >= 1.0
        for scale in (0.01, 1.0, 30.0, None):
            sc = rng.choice([0.01, 1.0, 30.0], size=(B, 1)) if scale is None else scale
            S = rng.standard_normal((B, n)) * sc
            K, Bt, _ = km.kappa_bound(idx, S, n, ls, X)
            Kg, A = km.gemm_form(idx, S, n, ls, X)
            assert np.all(np.abs(Kg - K) <= 64 * n * eps_x * A), (n, ls, scale)
            amp = float(np.max(hp.to_f64(A / Bt)))
            worst_amp = max(worst_amp, amp)
    print(f"n={n}: worst A / B~ = {worst_amp:.3f} (bound {km.AMPLIFICATION})")
    assert worst_amp <= km.AMPLIFICATION


def test_weights_sum_to_zero():
    rng = np.random.default_rng(2)
    for B in (3, 4, 65, 1024):
        K = rng.standard_normal((B, B))
        K = K + K.T
        r, T = km.rowsums(K)
        U, m, w = km.weights(r, T, B)
        assert abs(w.sum()) <= 8 * hp.EPS64 * np.abs(w).sum() * math.log2(B + 1)
        assert abs(U - (K.sum() - np.trace(K)) / (B * (B - 1))) <= 1e-13 * np.abs(K).sum() / (B * (B - 1))


def test_unbiased_by_exact_enumeration():
    """Softmax table over the 4 states of n = 2, B = 3: over all 4^3 sample tuples, E[U] = q^T K_p q and
    E[sum_b w_b grad log q(z_b)] = grad (q^T K_p q), to 1e-13 -- with the diagonal of K_p in, pairs dropped by index."""
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(2, 0)
    S_all = os_.score_matrix(bn, x, lat, obs)
    K = os_.gram_closed_form(S_all, 2, 1.0)
    theta = np.array([0.3, -0.7, 0.1, 0.9])
    q = np.exp(theta) / np.exp(theta).sum()
    J = np.diag(q) - np.outer(q, q)                     # d q / d theta
    exact, exact_grad = q @ K @ q, J.T @ (2 * K @ q)
    B = 3
    EU, Eg, EU_by_distance = 0.0, np.zeros(4), 0.0
    for tup in itertools.product(range(4), repeat=B):
        idx = np.array(tup)
        p = np.prod(q[idx])
        Kb = km.kappa_bound(idx, S_all[idx], 2, 1.0, X=km.F64)[0]
        r, T = km.rowsums(Kb)
        U, m, w = km.weights(r, T, B)
        EU += p * U
        Eg += p * sum(w[b] * (np.eye(4)[idx[b]] - q) for b in range(B))
        off = Kb * (idx[:, None] != idx[None, :])       # the biased variant: pairs dropped by Hamming distance 0
        EU_by_distance += p * off.sum() / (B * (B - 1))
    assert abs(EU - exact) <= 1e-13 * abs(exact) + 1e-15
    assert np.all(np.abs(Eg - exact_grad) <= 1e-13 * np.abs(exact_grad).max() + 1e-15)
    assert abs(EU_by_distance - exact) > 1e-3 * abs(exact)


def test_geometry_restatement():
    """ksd_sampled_mirror.pairs_geometry is the library's (bornvi_stein_pairs_geometry): the error constants depend on it."""
    for B in (2, 3, 31, 32, 33, 64, 65, 257, 513, 1024, 4096, 16384, 65536, 1 << 17):
        assert backend.stein_pairs_geometry(B) == km.pairs_geometry(B), B
    from tensornetworks_amd._ext import BornviError
    for B in (1, (1 << 17) + 1):
        with pytest.raises(BornviError):
            backend.stein_pairs_geometry(B)


def test_backend_argument_checks():
    """Every argument error is raised on the host, before any GPU call."""
    from tensornetworks_amd._ext import BornviError
    assert backend.STEIN_PAIRS_MAX_BATCH == 1 << 17
    i3 = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(BornviError, match="accepted: 1 ... 63"):
        backend.bn_score_samples(None, 64, i3)
    with pytest.raises(BornviError, match="p_floor"):
        backend.bn_score_samples(None, 4, i3, p_floor=0.0)
    with pytest.raises(BornviError, match="idx"):
        backend.bn_score_samples(None, 4, torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(BornviError, match="accepted: 1 ... 63"):
        backend.stein_pairs_rowsum(i3, torch.zeros(3, 64, dtype=torch.float64), 64)
    with pytest.raises(BornviError, match="n \\* length_scale >= 1"):
        backend.stein_pairs_rowsum(i3, torch.zeros(3, 4, dtype=torch.float64), 4, length_scale=0.2)
    with pytest.raises(BornviError, match="length_scale"):
        backend.stein_pairs_rowsum(i3, torch.zeros(3, 4, dtype=torch.float64), 4, length_scale=0.0)
    with pytest.raises(BornviError, match="2 <= B <= 2\\^17"):
        backend.stein_pairs_rowsum(torch.zeros(1, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.float64), 4)


def test_trainer_construction():
    from tensornetworks_amd import SampledKSDVariationalInference, SampledELBOVariationalInference
    from tensornetworks_amd.sampled_trainer import SampledTrainer
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(40, 0)
    vi = SampledKSDVariationalInference(bn, lat, obs, {'bond_dim': 4, 'num_samples': 64, 'seed': 3}, base_kernel_length_scale=0.5)
    assert vi.born_machine.cores.shape == (40, 2, 4, 4) and vi.num_samples == 64 and vi.seed == 3 and vi.objective == 'ksd2'
    assert isinstance(vi, SampledTrainer) and issubclass(SampledELBOVariationalInference, SampledTrainer)
    for bad in (2, 0, (1 << 17) + 1, 2.5, True):
        with pytest.raises(ValueError, match="num_samples must be an integer in 3 ... 2\\^17"):
            SampledKSDVariationalInference(bn, lat, obs, {'num_samples': bad})
    with pytest.raises(ValueError, match="unknown keys"):
        SampledKSDVariationalInference(bn, lat, obs, {'family': 'mps'})
    with pytest.raises(ValueError, match="base_kernel_length_scale >= 1"):
        SampledKSDVariationalInference(bn, lat, obs, {}, base_kernel_length_scale=0.02)
    with pytest.raises(ValueError, match="objective"):
        SampledKSDVariationalInference(bn, lat, obs, {}, objective='kl')
    with pytest.raises(ValueError, match="p_floor"):
        SampledKSDVariationalInference(bn, lat, obs, {}, p_floor=0.0)
    # the ELBO trainer's own range and wording are untouched
    with pytest.raises(ValueError, match="num_samples must be an integer in 1 ... 2\\^24"):
        SampledELBOVariationalInference(bn, lat, obs, {'num_samples': 0})
    assert SampledELBOVariationalInference(bn, lat, obs, {'num_samples': 1}).num_samples == 1
