"""Host checks of the exact-ELBO feature: the float64 mirror (elbo_mirror.py) on the two networks the feature was argued
with, the log-joint table's floor, and the argument validation that needs no GPU."""
import math
import os

import numpy as np
import pytest
import torch

import elbo_mirror as em
import hp_reference as hp
from conftest import GOLDEN, golden
from tensornetworks_amd import backend
from tensornetworks_amd.bayesian_network import get_sprinkler_network, joint_table, synthetic_network

SPRINKLER = ("hardware_efficient", 3, 4)
SYNTHETIC = ("hardware_efficient", 5, 3)


def sprinkler():
    return get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], {'W': 1}


def run(case, bn, lat, x, epochs=200):
    ansatz, n, L = case
    log_p, log_ev = em.log_joint(bn, lat, x)
    th0 = em.theta0(backend.num_params(ansatz, n, L))
    return em.train(ansatz, n, L, log_p, log_ev, th0, 0.05, epochs, posterior=np.exp(log_p - log_ev)), th0


@pytest.fixture(scope="module")
def sprinkler_run():
    bn, lat, _, x = sprinkler()
    return run(SPRINKLER, bn, lat, x)


@pytest.mark.parametrize("which", ["sprinkler", "synthetic"])
def test_loss_plus_evidence_is_a_kl(which):
    """L + log p(x) = KL(q || p(.|x)) >= 0 at random parameters."""
    if which == "sprinkler":
        (bn, lat, _, x), (ansatz, n, L) = sprinkler(), SPRINKLER
    else:
        (bn, lat, _, x), (ansatz, n, L) = synthetic_network(5, 0), SYNTHETIC
    log_p, log_ev = em.log_joint(bn, lat, x)
    rng = np.random.default_rng(4)
    for scale in (0.0, 0.1, 1.0, 3.0):
        theta = scale * rng.standard_normal(backend.num_params(ansatz, n, L))
        loss, ent, _, q = em.loss_and_grad(ansatz, n, L, theta, log_p)
        assert loss + log_ev >= -1e-12, (which, scale, loss + log_ev)
        assert 0.0 <= ent <= n * math.log(2) + 1e-12 and abs(q.sum() - 1) < 1e-12


def test_mirror_gradient_is_the_derivative_of_the_mirror_loss():
    """paramshift_vjp with w is d loss / d theta: central differences at a generic point."""
    bn, lat, _, x = synthetic_network(5, 0)
    ansatz, n, L = SYNTHETIC
    log_p, _ = em.log_joint(bn, lat, x)
    theta = np.random.default_rng(1).standard_normal(backend.num_params(ansatz, n, L))
    _, _, g, _ = em.loss_and_grad(ansatz, n, L, theta, log_p)
    for p in (0, 7, len(theta) - 1):
        e = np.zeros_like(theta)
        e[p] = 1e-5
        fd = (em.loss_and_grad(ansatz, n, L, theta + e, log_p)[0] - em.loss_and_grad(ansatz, n, L, theta - e, log_p)[0]) / 2e-5
        assert abs(fd - g[p]) <= 1e-8 * max(1.0, abs(g[p])), (p, fd, g[p])


def test_sprinkler_mirror_run_converges(sprinkler_run):
    """200 epochs, Adam, lr 0.05, cosine to lr / 10, clip 10, theta0 = 0.1 N(0, 1) from default_rng(0): the KL to the exact
    posterior falls from 1.095 to below 1e-6 (measured: 5.4e-11) and the TVD below 1e-4 (measured: 2.9e-6)."""
    h, _ = sprinkler_run
    assert h["kl"][-1] < h["kl"][0]
    assert h["kl"][-1] < 1e-6 and h["tvd"][-1] < 1e-4, (h["kl"][-1], h["tvd"][-1])
    assert min(h["kl"]) >= -1e-12


def test_sprinkler_mirror_run_is_the_recorded_trace(sprinkler_run):
    """tests/golden/elbo_sprinkler_trace.npz (what the GPU trainer test compares train() with) is this run."""
    h, th0 = sprinkler_run
    g = golden("elbo_sprinkler_trace.npz")
    np.testing.assert_array_equal(g["theta0"], th0)
    np.testing.assert_allclose(h["loss_elbo"], g["loss_elbo"], rtol=1e-7)
    np.testing.assert_allclose(h["theta"][-1], g["theta_final"], rtol=0, atol=1e-6)


def test_synthetic_mirror_run_improves():
    bn, lat, _, x = synthetic_network(5, 0)
    h, _ = run(SYNTHETIC, bn, lat, x)
    assert h["kl"][-1] < h["kl"][0] and h["tvd"][-1] < h["tvd"][0]
    assert min(h["kl"]) >= -1e-12


def test_p_floor_keeps_the_table_finite():
    """cut_network(): joint probabilities down to 1e-12; with a CPT row made deterministic, exact zeros: the table is
    log max(p, p_floor), finite either way, and equal to log p wherever p is above the floor."""
    from tensornetworks_amd.elbo_objective import ElboObjective
    bn, lat, _, x = hp.cut_network()
    for deterministic in (False, True):
        if deterministic:
            bn.cpts["Z1"][()] = {0: 1.0, 1: 0.0}
        pxz = torch.from_numpy(joint_table(bn, lat, x))
        assert bool((pxz == 0).any()) == deterministic
        table = ElboObjective.log_table(pxz, 1e-30)
        assert torch.isfinite(table).all()
        above = pxz > 1e-30
        assert torch.equal(table[above], torch.log(pxz[above]))
        assert (table[~above] == math.log(1e-30)).all()
        np.testing.assert_array_equal(table.numpy(), em.log_joint(bn, lat, x)[0])
    assert not torch.isfinite(torch.log(pxz)).all()           # what the floor is for


def test_argument_validation():
    from tensornetworks_amd.elbo_objective import ElboObjective
    from tensornetworks_amd.elbo_vi import ELBOVariationalInference as ClassicalELBO
    from tensornetworks_amd.elbo_vi_quantum import ELBOVariationalInference
    bn, lat, obs, x = sprinkler()
    for bad in (0.0, -1e-30, float("nan"), float("inf"), "1e-30", True):
        with pytest.raises(ValueError, match="p_floor"):
            ElboObjective(bn, lat, "cpu", p_floor=bad)
        with pytest.raises(ValueError, match="p_floor"):
            ELBOVariationalInference(bn, lat, obs, 3, p_floor=bad)
        with pytest.raises(ValueError, match="p_floor"):
            ClassicalELBO(bn, lat, obs, {"use_logits": True}, p_floor=bad)
    with pytest.raises(ValueError, match="latent"):
        ElboObjective(bn, [], "cpu")
    with pytest.raises(ValueError, match="qbm_num_latent_vars"):
        ELBOVariationalInference(bn, lat, obs, 4)
    with pytest.raises(ValueError, match="prepare"):
        ElboObjective(bn, lat, "cpu").weights(torch.zeros(8, dtype=torch.float64))
    vi = ELBOVariationalInference(bn, lat, obs, 3)
    with pytest.raises(ValueError, match="prepare"):
        vi.elbo_and_grad_local(torch.zeros(vi.born_machine.num_ansatz_params, dtype=torch.float64), 0, 1, 1)
    with pytest.raises(ValueError, match="Keys in x_observation_dict"):
        vi.train({'Q': 1}, 1, 0.01, verbose=False)
    # the wrapper's own checks come before any GPU call
    q, log_p = torch.full((8,), 0.125, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    for kw in ({"q_floor": 0.0}, {"q_floor": -1.0}, {"q_floor": float("nan")}, {"want_w": False, "out": q.clone()}):
        with pytest.raises(backend.BornviError):
            backend.elbo_weights(q, log_p, **kw)
    for a, b in ((q[:6], log_p[:6]), (q, log_p[:4]), (q.reshape(2, 2, 2), log_p), (q[:1], log_p[:1])):
        with pytest.raises(backend.BornviError):
            backend.elbo_weights(a, b)


def test_exports():
    import tensornetworks_amd as t
    from tensornetworks_amd import _ext
    assert t.ELBOVariationalInference.__module__.endswith("elbo_vi_quantum")
    assert t.ClassicalELBOVariationalInference.__module__.endswith("elbo_vi")
    assert {"bornvi_elbo_workspace_bytes", "bornvi_elbo_weights"} <= set(_ext.EXPORTED_SYMBOLS)
    lib = _ext.lib()
    assert lib.bornvi_elbo_weights is not None and lib.bornvi_elbo_workspace_bytes is not None
    assert os.path.exists(os.path.join(GOLDEN, "elbo_sprinkler_trace.npz"))
