"""The sampled MPS Born machine's mathematics on the CPU (mps_sampled_mirror.py) and the host surface: no GPU needed."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_mirror as mm
import mps_sampled_mirror as sm
from tensornetworks_amd import backend
from tensornetworks_amd.backend import mps_environments, mps_sample, mps_score_vjp, bn_logjoint_samples  # noqa: F401


def rand_cores(n, D, seed=0, spread=0.3):
    rng = np.random.default_rng([n, D, seed])
    return (np.eye(D)[None, None] + spread * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0)


@pytest.mark.parametrize("n,D", [(1, 1), (1, 3), (2, 2), (3, 3), (5, 2), (8, 1), (8, 3), (6, 2)])
def test_conditionals_multiply_to_q(n, D):
    """The product over the sites of the mirror's conditionals is mps_mirror's q(z), for every z; so is exp(logq); and the
    left and right environments give the same Z."""
    cores = rand_cores(n, D)
    ref = mm.reference(cores)
    bits = mm.bits_of(n)
    c = sm.conditionals(cores, bits)
    prod = np.prod(np.where(bits == 1, c["p1"], 1 - c["p1"]), axis=1)
    assert np.allclose(hp.to_f64(prod), hp.to_f64(ref["q"]), rtol=1e-12, atol=1e-300)
    assert np.allclose(hp.to_f64(np.exp(c["logq"])), hp.to_f64(ref["q"]), rtol=1e-12, atol=1e-300)
    env = sm.environments(cores)
    assert abs(float(env["Z"] / ref["Z"]) - 1.0) < 1e-13
    assert abs(float(env["L"][n][0, 0] / ref["Z"]) - 1.0) < 1e-13
    assert np.array_equal(sm.idx_of_bits(bits), np.arange(1 << n))
    assert np.array_equal(sm.bits_of_idx(np.arange(1 << n), n), bits)


@pytest.mark.parametrize("n,D", [(1, 2), (3, 1), (4, 3), (7, 2)])
def test_score_has_mean_zero(n, D):
    """sum_z q_z grad log q_z = 0: against the absolute-value gradient, to rounding."""
    cores = rand_cores(n, D, 1)
    bits = mm.bits_of(n)
    q = hp.to_f64(mm.reference(cores)["q"])
    g = sm.score_gradient(cores, bits, q)
    r, at = hp.worst(hp.ratio(hp.to_f64(g["grad"]), 0.0, g["grad_abs"], X=hp._LongDouble))
    assert r <= 8, (r, at)


@pytest.mark.parametrize("n,D,B", [(1, 1, 3), (2, 3, 7), (5, 2, 40), (8, 3, 33)])
def test_score_gradient_agrees_with_autograd(n, D, B):
    """The mirror's sum_b w_b grad log q(z_b) (left and right vectors, extended precision) against torch autograd on a float64
    restatement: to 64 n D units of EPS64 of the absolute-value gradient; unused entries of the boundary cores are exactly 0."""
    cores = rand_cores(n, D, 2)
    rng = np.random.default_rng([n, D, B])
    bits = rng.integers(0, 2, size=(B, n))
    bits[0] = 0
    bits[-1] = 1
    w = rng.standard_normal(B)
    g = sm.score_gradient(cores, bits, w)
    auto = sm.autograd_score(cores, bits, w)
    r, at = hp.worst(hp.ratio(auto, g["grad"], g["grad_abs"], X=hp._LongDouble))
    assert r <= 64 * n * D, (r, at)
    if D > 1:
        g64 = hp.to_f64(g["grad"])
        assert np.all(g64[0][:, 1:, :] == 0.0) and np.all(g64[n - 1][:, :, 1:] == 0.0)
    assert np.allclose(hp.to_f64(g["logq"]), sm.logq_torch(torch.as_tensor(cores), bits).numpy(), rtol=1e-12, atol=1e-12)


def test_uniforms_and_sampler():
    """The uniforms are a function of (seed, epoch, b, k) only; the mirror's sampler follows q (chi-square-free check: with
    2^14 samples at n = 3 every frequency is within 6 standard errors)."""
    U = sm.uniforms(7, 3, np.arange(10), 5)
    assert U.shape == (10, 5) and np.all((U >= 0) & (U < 1))
    assert np.array_equal(U[4:6], sm.uniforms(7, 3, np.array([4, 5]), 5))
    assert np.array_equal(U[:, :3], sm.uniforms(7, 3, np.arange(10), 3))           # odd n: the pair's second word unused
    assert not np.array_equal(U, sm.uniforms(7, 4, np.arange(10), 5)) and not np.array_equal(U, sm.uniforms(8, 3, np.arange(10), 5))
    cores = rand_cores(3, 2, 5)
    q = hp.to_f64(mm.reference(cores)["q"])
    B = 1 << 14
    s = sm.sample(cores, 11, 0, B)
    freq = np.bincount(s["idx"], minlength=8) / B
    assert np.all(np.abs(freq - q) <= 6 * np.sqrt(q * (1 - q) / B))
    c = sm.conditionals(cores, s["bits"])
    assert np.allclose(hp.to_f64(s["logq"]), hp.to_f64(c["logq"]), rtol=0, atol=1e-14)


def test_log_joint_mirror_against_the_network():
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    bn = get_sprinkler_network(False)
    lat = ['C', 'S', 'R']
    for wv in (0, 1):
        packed = pack_network(bn, lat, {'W': wv})
        bits = mm.bits_of(3)
        lp = sm.log_joint(packed, bits)
        for z in range(8):
            a = dict(zip(lat, bits[z].tolist()))
            a['W'] = wv
            assert abs(lp[z] - np.log(bn.get_joint_probability(tuple(a[nm] for nm in bn.nodes)))) < 1e-14
    packed = pack_network(bn, ['C', 'S'], {'W': 1})
    with pytest.raises(ValueError):
        sm.log_joint(packed, mm.bits_of(2))


def test_module_construction_and_messages():
    from tensornetworks_amd import MPSBornMachine, SampledMPSBornMachine
    torch.manual_seed(5)
    a = SampledMPSBornMachine(4, bond_dim=3)
    torch.manual_seed(5)
    b = MPSBornMachine(4, bond_dim=3)
    assert torch.equal(a.cores, b.cores) and a.cores.dtype == torch.float64 and a.num_parameters == 4 * 2 * 9
    big = SampledMPSBornMachine(27, bond_dim=2)
    assert big.cores.shape == (27, 2, 2, 2)
    SampledMPSBornMachine(63, bond_dim=1)
    with pytest.raises(ValueError, match="1 ... 26"):
        MPSBornMachine(27)
    with pytest.raises(ValueError, match="1 ... 63"):
        SampledMPSBornMachine(64)
    with pytest.raises(ValueError, match="1 ... 63"):
        SampledMPSBornMachine(0)
    with pytest.raises(ValueError, match="bond_dim must be an integer in 1 ... 32"):
        SampledMPSBornMachine(4, bond_dim=33)
    with pytest.raises(ValueError, match="init_method"):
        SampledMPSBornMachine(4, init_method='ones')
    with pytest.raises(ValueError, match="not conditional"):
        SampledMPSBornMachine(4, conditioning_dim=1)
    for call in (big.get_probabilities, big.probabilities64):
        with pytest.raises(ValueError, match="sample_indices and log_prob"):
            call()
    with pytest.raises(ValueError, match="not a valid outcome"):
        a.indices_of(torch.tensor([[0., 1., 2., 0.]]))
    assert a.indices_of(torch.tensor([[1., 0., 1., 1.]])).tolist() == [11]
    assert torch.equal(a.bits_of(torch.tensor([11])), torch.tensor([[1., 0., 1., 1.]]))
    i62 = big.indices_of(torch.ones(1, 27))
    assert i62.tolist() == [(1 << 27) - 1]


def test_backend_argument_checks():
    """Every argument error is raised on the host, before any GPU call (none of these reaches the library)."""
    from tensornetworks_amd._ext import BornviError
    assert backend.MPS_SAMPLED_MAX_N == 63
    with pytest.raises(BornviError, match="accepted: 1 ... 63"):
        backend.mps_environments(torch.zeros(64, 2, 2, 2, dtype=torch.float64), 8)
    with pytest.raises(BornviError, match="bond dimension"):
        backend.mps_environments(torch.zeros(4, 2, 33, 33, dtype=torch.float64), 8)
    with pytest.raises(BornviError, match="n, 2, D, D"):
        backend.mps_environments(torch.zeros(4, 2, 3, 2, dtype=torch.float64), 8)
    for bad in (0, (1 << 24) + 1, 2.5, True):
        with pytest.raises(BornviError, match="number of samples"):
            backend.mps_environments(torch.zeros(4, 2, 2, 2, dtype=torch.float64), bad)
    with pytest.raises(BornviError, match="idx"):
        backend.mps_score_vjp(torch.zeros(4, 2, 2, 2, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.int64), None)
    with pytest.raises(BornviError, match="p_floor"):
        backend.bn_logjoint_samples(None, 4, torch.zeros(3, dtype=torch.int64), p_floor=0.0)
    with pytest.raises(BornviError, match="accepted: 1 ... 63"):
        backend.bn_logjoint_samples(None, 64, torch.zeros(3, dtype=torch.int64))


def test_trainer_construction():
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network, get_sprinkler_network
    bn, lat, obs, x = synthetic_network(40, 0)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 4, 'num_samples': 64, 'seed': 3})
    assert vi.born_machine.cores.shape == (40, 2, 4, 4) and vi.num_samples == 64 and vi.seed == 3
    with pytest.raises(ValueError, match="num_samples"):
        SampledELBOVariationalInference(bn, lat, obs, {'num_samples': 0})
    with pytest.raises(ValueError, match="unknown keys"):
        SampledELBOVariationalInference(bn, lat, obs, {'family': 'mps'})
    with pytest.raises(ValueError, match="p_floor"):
        SampledELBOVariationalInference(bn, lat, obs, {}, p_floor=-1.0)
    sp = SampledELBOVariationalInference(get_sprinkler_network(False), ['C', 'S'], ['W'], {'bond_dim': 2, 'num_samples': 8})
    with pytest.raises(ValueError, match="summed-out"):
        sp._prepare_observation({'W': 1})
