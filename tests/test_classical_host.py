"""Classical Born machine, host side: the torch mirror of the reference's epoch reproduces the captured classical
traces on the CPU, the drop-in draws the reference's initial parameters, and argument errors are raised before any GPU
call."""
import numpy as np
import pytest
import torch

import classical_mirror as mirror
from conftest import golden
from oracle import stein as os_
from tensornetworks_amd import backend
from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
from tensornetworks_amd.born_machine_classical_sim import ClassicalBornMachine
from tensornetworks_amd.ksd_vi import KSDVariationalInference
from tensornetworks_amd.utils import generate_all_binary_outcomes

CASES = ["classical_sprinkler_logits", "classical_sprinkler_abs", "classical_sprinkler_sgd", "classical_synthetic_n6",
         "classical_sprinkler_mlp"]


def case_setup(g):
    """(bn, latents, observed, evidence, posterior dict) of a golden trace."""
    n = int(g["n"])
    if n == 3:
        bn, lat, obs, x = get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], {'W': int(g["x_value"][0])}
    else:
        bn, lat, obs, x = synthetic_network(n, 0)
    post = dict(zip(generate_all_binary_outcomes(n), (float(v) for v in g["posterior"])))
    return bn, lat, obs, x, post


def config(g):
    return {'use_logits': bool(g["use_logits"]), 'conditioning_dim': int(g["conditioning_dim"])}


@pytest.mark.parametrize("name", CASES)
def test_mirror_reproduces_reference_trace(name):
    g = golden(name + ".npz")
    bn, lat, obs, x, post = case_setup(g)
    n = len(lat)
    K = torch.from_numpy(os_.gram_closed_form(os_.score_matrix(bn, x, lat, obs), n))
    torch.manual_seed(int(g["seed"]))
    bm = mirror.MirrorBornMachine(n, **config(g))
    xc = None
    if int(g["conditioning_dim"]) > 0:
        bm.param_generator_net.eval()
        xc = torch.tensor([float(v) for v in g["x_value"]])
    flat = lambda: torch.cat([p.detach().reshape(-1) for p in bm.parameters()]).numpy()
    np.testing.assert_array_equal(flat(), g["params"][0])          # same draws in the same order
    snaps = {}
    E = len(g["loss_ksd"])
    hist, qs, fixed = mirror.train(bm, K, post, xc, num_epochs=E, lr=float(g["lr"]), clip=float(g["clip"]),
                                   optimizer_type="sgd" if bool(g["sgd"]) else "adam",
                                   entropy_weight=float(g["entropy_weight"]))
    snaps[E] = flat()
    # CPU against CPU, same float32 operations except the order of the K_p contraction: agreement to a few float32 ulps
    np.testing.assert_allclose(qs, g["q"], rtol=1e-5, atol=1e-7)
    for key in ("loss_ksd", "entropy", "grad_norm", "tvd"):
        np.testing.assert_allclose(hist[key], g[key], rtol=1e-5, atol=1e-7, err_msg=key)
    np.testing.assert_allclose(snaps[E], g["params"][-1], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(fixed, g["fixed_probs"], rtol=1e-5, atol=1e-7)


def test_initialisation_matches_reference_draws():
    g = golden("classical_sprinkler_logits.npz")
    torch.manual_seed(int(g["seed"]))
    bm = ClassicalBornMachine(3, use_logits=True)
    np.testing.assert_array_equal(bm.params.detach().numpy(), g["params"][0])
    gm = golden("classical_sprinkler_mlp.npz")
    torch.manual_seed(int(gm["seed"]))
    bm = ClassicalBornMachine(3, conditioning_dim=1)
    np.testing.assert_array_equal(torch.cat([p.detach().reshape(-1) for p in bm.parameters()]).numpy(), gm["params"][0])


def test_trainer_forces_small_random():
    g = golden("classical_sprinkler_logits.npz")
    torch.manual_seed(int(g["seed"]))
    vi = KSDVariationalInference(get_sprinkler_network(False), ['C', 'S', 'R'], ['W'],
                                 born_machine_config={'use_logits': True, 'conditioning_dim': 0, 'init_method': 'uniform'})
    np.testing.assert_array_equal(vi.born_machine.params.detach().numpy(), g["params"][0])
    assert vi.num_possible_latent_states == 8 and len(vi.all_latent_states_tuples) == 8
    assert vi.born_machine.all_outcome_tuples == generate_all_binary_outcomes(3)


def test_argument_errors_before_any_gpu_call():
    w = torch.zeros(1, 8)
    with pytest.raises(backend.BornviError, match="mode"):
        backend.born_table_probs(w, 2)
    with pytest.raises(backend.BornviError, match="power of two"):
        backend.born_table_probs(torch.zeros(1, 6), 0)
    with pytest.raises(backend.BornviError, match="rows"):
        backend.born_table_probs(torch.zeros(8), 0)
    with pytest.raises(backend.BornviError, match="entropy_weight"):
        backend.born_table_vjp(w, w.double(), 0, entropy_weight=float("nan"))
    with pytest.raises(backend.BornviError, match="loss_out"):
        backend.born_table_vjp(w, w.double(), 0, y=w.double(), loss_out=torch.zeros(1, dtype=torch.float64))
    bm = ClassicalBornMachine(3)
    with pytest.raises(ValueError, match="conditioning_dim is 0"):
        bm.get_probabilities(torch.ones(1))
    with pytest.raises(ValueError, match="not conditional"):
        bm.get_log_q_z_x(torch.zeros(2, 3), torch.ones(1))
    cbm = ClassicalBornMachine(3, conditioning_dim=1)
    with pytest.raises(ValueError, match="must be provided"):
        cbm.get_probabilities()
    with pytest.raises(ValueError, match="must be provided"):
        cbm.get_log_q_z_x(torch.zeros(2, 3))
    vi = KSDVariationalInference(get_sprinkler_network(False), ['C', 'S', 'R'], ['W'],
                                 born_machine_config={'use_logits': True, 'conditioning_dim': 2})
    with pytest.raises(ValueError, match="Keys in x_observation_dict"):
        vi.train({'X': 1}, num_epochs=1, lr_born_machine=0.01, verbose=False)
    with pytest.raises(ValueError, match="conditioning_dim must match"):
        vi.train({'W': 1}, num_epochs=1, lr_born_machine=0.01, verbose=False)


def test_fixed_probs_are_host_only():
    bm = ClassicalBornMachine(2)
    p = torch.tensor([0.1, 0.2, 0.3, 0.4])
    bm.set_fixed_probs(p)
    assert torch.equal(bm.get_probabilities(), p.unsqueeze(0))
    d = bm.get_prob_dict()
    assert list(d) == [(0, 0), (0, 1), (1, 0), (1, 1)] and np.isclose(d[(1, 1)], 0.4)
    lq = bm.get_log_q_z_x(torch.tensor([[1.0, 0.0], [0.0, 1.0]]))
    np.testing.assert_allclose(lq.numpy(), np.log([0.3, 0.2]), rtol=1e-6)
    with pytest.raises(ValueError, match=r"Sample \(2, 0\) is not a valid outcome"):
        bm.get_log_q_z_x(torch.tensor([[2.0, 0.0]]))
    assert abs(float(bm.entropy()) - float(-(p * p.log()).sum())) < 1e-6
    bm.clear_fixed_probs()
    assert bm._fixed_probs is None and not bm._use_fixed_probs
