"""Host side of amortised inference: the mirror's sampler and log-marginal gradient against what they
mirror, pack_network_for_sampling, and every argument error of AmortisedMPSInference, raised before any GPU call."""
import itertools

import numpy as np
import pytest
import torch

import amortised_mirror as am
import mps_sampled_mirror as sm
from tensornetworks_amd import _ext
from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference
from tensornetworks_amd.bayesian_network import (BayesianNetwork, check_sampling_pack, get_sprinkler_network, pack_network,
                                                pack_network_for_sampling, synthetic_network)


def test_mirror_sampler_frequencies_on_sprinkler():
    """B = 65 536, seed 0, epoch 0: every one of the 16 joint frequencies within 5 sqrt(p (1 - p) / B) of the exact joint."""
    bn = get_sprinkler_network(False)
    sites = ['C', 'S', 'R', 'W']
    B = 65536
    s = am.bn_sample(pack_network_for_sampling(bn, sites), 4, 0, 0, B)
    assert not s["dead"].any()
    freq = np.bincount(s["idx"].astype(np.int64), minlength=16) / B
    for state, z in enumerate(itertools.product((0, 1), repeat=4)):
        p = bn.get_joint_probability(z)
        assert abs(freq[state] - p) <= 5 * np.sqrt(p * (1 - p) / B), (z, freq[state], p)
    # logp is the log joint of the draw
    want = np.log([bn.get_joint_probability(tuple(b)) for b in s["bits"][:64]])
    assert np.allclose(np.asarray(s["logp"][:64], dtype=np.float64), want, rtol=0, atol=1e-14)
    # a sample depends on (seed, epoch, b), not on B
    small = am.bn_sample(pack_network_for_sampling(bn, sites), 4, 0, 0, 65)
    assert np.array_equal(small["idx"], s["idx"][:65])
    assert not np.array_equal(am.bn_sample(pack_network_for_sampling(bn, sites), 4, 0, 1, 65)["idx"], small["idx"])


def _cores(n, D, seed=0):
    rng = np.random.default_rng([n, D, seed])
    return (np.eye(D)[None, None] + 0.4 * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0)


@pytest.mark.parametrize("n,D", [(1, 1), (1, 3), (2, 2), (4, 3), (6, 2), (5, 1)])
def test_mirror_log_marginal_gradient_against_autograd(n, D):
    cores = _cores(n, D)
    rng = np.random.default_rng([n, D, 5])
    evs = [{}, {p: int(rng.integers(0, 2)) for p in range(n)}, {0: 1}, {n - 1: 0},
           {p: int(rng.integers(0, 2)) for p in range(0, n, 2)}]
    c = rng.standard_normal(len(evs))
    ref = am.log_marginal_gradient(cores, evs, c)
    want = am.autograd_logm(cores, evs, c)
    got = np.asarray(ref["grad"], dtype=np.float64)
    scale = np.asarray(ref["grad_abs"], dtype=np.float64)
    assert np.all(np.abs(got - want) <= 1e-12 * (scale + 1e-300)), float(np.abs(got - want).max())
    for j, ev in enumerate(evs):
        assert abs(float(ref["logm"][j]) - float(am.logm_torch(torch.as_tensor(cores), ev))) <= 1e-12
    assert float(ref["logm"][0]) == 0.0
    # all-empty evidences: the gradient vanishes; an all-clamped one is the score gradient
    zero = am.log_marginal_gradient(cores, [{}, {}], [0.7, -0.2])
    assert np.all(np.abs(np.asarray(zero["grad"], dtype=np.float64)) <= 1e-15 * np.asarray(zero["grad_abs"], dtype=np.float64))
    bits = np.array([[evs[1][p] for p in range(n)]])
    score = sm.score_gradient(cores, bits, [1.5])
    full = am.log_marginal_gradient(cores, [evs[1]], [1.5])
    assert np.allclose(np.asarray(full["grad"], dtype=np.float64), np.asarray(score["grad"], dtype=np.float64), rtol=0,
                       atol=1e-13 * float(np.asarray(score["grad_abs"], dtype=np.float64).max()))
    # the batched environments of the replay are the same function
    mask = np.array([[1 if p in ev else 0 for p in range(n)] for ev in evs])
    value = np.array([[ev.get(p, 0) for p in range(n)] for ev in evs])
    env = am.logm_env_torch(torch.as_tensor(cores), mask, value).numpy()
    assert np.allclose(env, np.asarray(ref["logm"], dtype=np.float64), rtol=0, atol=1e-12)


def test_mirror_gradient_drops_impossible_evidence():
    cores = _cores(4, 2)
    cores[2, 1] = 0.0
    evs = [{2: 1}, {0: 1}, {2: 0, 3: 1}]
    both = am.log_marginal_gradient(cores, evs, [0.3, -0.8, 0.5])
    rest = am.log_marginal_gradient(cores, evs[1:], [-0.8, 0.5])
    assert both["logm"][0] == -np.inf and np.array_equal(both["grad"], rest["grad"])


def test_pack_network_for_sampling():
    bn = get_sprinkler_network(False)
    packed = pack_network_for_sampling(bn, ['W', 'C', 'S'])
    assert packed["role"].tolist() == [1, 2, -3, 0]                 # C, S, R (drawn and dropped), W
    ref = pack_network(bn, ['W', 'C', 'S'], {})
    for k in ref:
        assert np.array_equal(packed[k], ref[k])
    with pytest.raises(ValueError, match="repeated"):
        pack_network_for_sampling(bn, ['C', 'C'])
    with pytest.raises(ValueError, match="not a node"):
        pack_network_for_sampling(bn, ['C', 'Q'])
    # a child listed before its parent
    wrong = BayesianNetwork()
    wrong.add_node('A', cpt={(): {0: 0.5, 1: 0.5}})
    wrong.add_node('B', cpt={(0,): {0: 0.5, 1: 0.5}, (1,): {0: 0.1, 1: 0.9}}, parent_names=['A'])
    wrong.nodes = ['B', 'A']
    wrong.node_to_index = {'B': 0, 'A': 1}
    with pytest.raises(ValueError, match="before its parent"):
        pack_network_for_sampling(wrong, ['A', 'B'])
    # the same two rules on packed arrays: an observed role, a parent index not below the node's own
    observed = pack_network(bn, ['C', 'S', 'R'], {'W': 1})
    with pytest.raises(ValueError, match="observed"):
        check_sampling_pack(observed, 3)
    bad = {k: v.copy() for k, v in packed.items()}
    bad["parents"][1, 0] = 2
    with pytest.raises(ValueError, match="parent index"):
        check_sampling_pack(bad, 3)
    bad = {k: v.copy() for k, v in packed.items()}
    bad["role"][0] = 0
    with pytest.raises(ValueError, match="each once"):
        check_sampling_pack(bad, 3)


def test_trainer_arguments_raise_before_any_gpu_call():
    bn = get_sprinkler_network(False)
    lat, obs = ['C', 'S', 'R'], ['W']
    with pytest.raises(ValueError, match="unknown keys"):
        AmortisedMPSInference(bn, lat, obs, {'bond_dim': 2, 'length_scale': 1.0})
    with pytest.raises(ValueError, match="site_order"):
        AmortisedMPSInference(bn, lat, obs, {'site_order': ['C', 'S', 'R']})                      # W is missing
    with pytest.raises(ValueError, match="site_order"):
        AmortisedMPSInference(bn, lat, obs, {'site_order': ['C', 'S', 'R', 'W', 'C']})            # repeated
    with pytest.raises(ValueError, match="site_order"):
        AmortisedMPSInference(bn, lat, obs, {'site_order': ['C', 'S', 'R', 'Q']})                 # unknown
    with pytest.raises(ValueError, match="num_samples"):
        AmortisedMPSInference(bn, lat, obs, {'num_samples': 0})
    big, zs, xs, _ = synthetic_network(64)
    with pytest.raises(ValueError, match="63"):
        AmortisedMPSInference(big, zs, xs, {'bond_dim': 2})                                       # 65 sites
    net, zs, xs, _ = synthetic_network(20)
    vi = AmortisedMPSInference(net, zs[:3], zs[3:] + xs, {'bond_dim': 2, 'num_samples': (1 << 16) + 1})     # 18 observed sites
    with pytest.raises(ValueError, match="2\\^16"):
        vi.train(1, 0.01, objective='conditional', verbose=False)
    with pytest.raises(ValueError, match="objective"):
        vi.train(1, 0.01, objective='reverse', verbose=False)
    vi = AmortisedMPSInference(bn, lat, obs, {'bond_dim': 2, 'site_order': ['W', 'R', 'S', 'C']})
    assert vi.site_names == ['W', 'R', 'S', 'C'] and vi._packed["role"].tolist() == [3, 2, 1, 0]
    assert AmortisedMPSInference(bn, ['S'], ['W'], {}).site_names == ['S', 'W']                   # network order; C, R dropped
    for call in (vi.posterior_marginals, vi.log_evidence, lambda x: vi.posterior_sample(x, 4),
                 lambda x: vi.posterior_log_prob(x, np.zeros((1, 3), np.int64))):
        with pytest.raises(ValueError, match="neither"):
            call({'Q': 1})
        with pytest.raises(ValueError, match="0 or 1"):
            call({'W': 2})
    import tensornetworks_amd
    assert tensornetworks_amd.AmortisedMPSInference is AmortisedMPSInference and "AmortisedMPSInference" in tensornetworks_amd.__all__
    assert {"bornvi_bn_sample", "bornvi_mps_log_marginals_vjp", "bornvi_mps_log_marginals_vjp_geometry",
            "bornvi_mps_log_marginals_vjp_workspace_bytes"} <= set(_ext.EXPORTED_SYMBOLS)


def test_site_joint_is_the_marginal_of_the_network():
    bn = get_sprinkler_network(False)
    vi = AmortisedMPSInference(bn, ['S'], ['W'], {})
    p = vi.site_joint_table().numpy()
    assert np.allclose(p, am.site_joint(bn, ['S', 'W']), rtol=0, atol=1e-16) and abs(p.sum() - 1) < 1e-15
    post, pw = bn.get_true_posterior(['S'], {'W': 1})
    assert abs(p[0b01] + p[0b11] - pw) < 1e-15 and abs(p[0b11] / pw - post[(1,)]) < 1e-15
