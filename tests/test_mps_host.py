"""The MPS Born machine's mathematics on the CPU (mps_mirror.py) and the module's host side: no GPU needed."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_mirror as mm


@pytest.mark.parametrize("n,D", [(1, 1), (1, 3), (2, 2), (4, 3), (6, 2), (5, 5)])
def test_mirror_gradients_agree(n, D):
    """The per-z outer-product gradient (extended precision), torch autograd (float64) and the doubling form (float64) are the
    same numbers: to 64 n D units of EPS64 of the absolute-value gradient (two float64 evaluations of n D-term chains each)."""
    rng = np.random.default_rng([n, D])
    cores = (np.eye(D)[None, None] + 0.3 * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0)
    g = rng.standard_normal(1 << n)
    ref = mm.reference(cores, g)
    for other in (mm.autograd_gradient(cores, g), mm.doubling(cores, g)["grad"]):
        r, at = hp.worst(hp.ratio(other, ref["grad"], ref["grad_abs"], X=hp._LongDouble))
        assert r <= 64 * n * D, (r, at)
    dbl = mm.doubling(cores)
    assert np.allclose(dbl["q"], hp.to_f64(ref["q"]), rtol=1e-12, atol=1e-300)
    assert abs(float(ref["q"].sum()) - 1.0) < 1e-14
    # unused entries of the first and last core
    if D > 1:
        assert np.all(hp.to_f64(ref["grad"])[0][:, 1:, :] == 0.0) and np.all(hp.to_f64(ref["grad"])[n - 1][:, :, 1:] == 0.0)


def test_bond_one_is_a_product_distribution():
    n = 6
    rng = np.random.default_rng(3)
    a = rng.standard_normal((n, 2))
    q = hp.to_f64(mm.reference(a.reshape(n, 2, 1, 1))["q"])
    B = mm.bits_of(n)
    want = np.ones(1 << n)
    for k in range(n):
        want *= a[k, B[:, k]] ** 2 / (a[k, 0] ** 2 + a[k, 1] ** 2)
    assert np.allclose(q, want, rtol=1e-13, atol=0)


def test_ghz_state():
    """A_k[s] = e_s e_s^T in the bulk, first site row 0 -> e_s, last site e_s -> column 0: mass 1/2 on 0..0 and on 1..1."""
    n = 5
    cores = np.zeros((n, 2, 2, 2))
    for s in (0, 1):
        cores[0, s, 0, s] = 1.0
        cores[1:n - 1, s, s, s] = 1.0
        cores[n - 1, s, s, 0] = 1.0
    q = hp.to_f64(mm.reference(cores)["q"])
    want = np.zeros(1 << n)
    want[0] = want[-1] = 0.5
    assert np.array_equal(q, want)


def test_module_construction():
    from tensornetworks_amd import MPSBornMachine
    torch.manual_seed(5)
    a = MPSBornMachine(4, bond_dim=3)
    torch.manual_seed(5)
    b = MPSBornMachine(4, bond_dim=3)
    torch.manual_seed(5)
    want = mm.init_cores(4, 3)
    assert a.cores.dtype == torch.float64 and tuple(a.cores.shape) == (4, 2, 3, 3)
    assert torch.equal(a.cores, b.cores) and torch.equal(a.cores.detach(), want)
    assert a.num_parameters == 4 * 2 * 9 and [p.shape for p in a.parameters()] == [a.cores.shape]
    z = MPSBornMachine(3, bond_dim=2, init_method='zero')
    assert torch.equal(z.cores.detach(), (torch.eye(2, dtype=torch.float64) / np.sqrt(2.0)).expand(3, 2, 2, 2))
    assert np.allclose(mm.doubling(z.cores.detach().numpy())["q"], 1.0 / 8, rtol=1e-15)
    torch.manual_seed(1)
    r = MPSBornMachine(3, bond_dim=2, init_method='random')
    torch.manual_seed(1)
    assert torch.equal(r.cores.detach(), mm.init_cores(3, 2, 'random'))
    assert MPSBornMachine(3).bond_dim == 4


def test_module_errors():
    from tensornetworks_amd.born_machine_mps import MPSBornMachine
    with pytest.raises(ValueError, match="conditioning_dim"):
        MPSBornMachine(3, conditioning_dim=2)
    for bad in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="bond_dim"):
            MPSBornMachine(3, bond_dim=bad)
    for bad in (0, 27):
        with pytest.raises(ValueError, match="num_latent_vars"):
            MPSBornMachine(bad)
    with pytest.raises(ValueError, match="init_method"):
        MPSBornMachine(3, init_method='uniform')
    bm = MPSBornMachine(3, bond_dim=2)
    with pytest.raises(ValueError, match="x_condition provided but conditioning_dim is 0."):
        bm.probabilities64(torch.zeros(1))
    with pytest.raises(ValueError, match="not conditional"):
        bm.get_log_q_z_x(torch.zeros(1, 3), torch.zeros(1))
    # fixed probabilities need no GPU
    p = torch.tensor([0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5])
    bm.set_fixed_probs(p)
    assert tuple(bm.get_probabilities().shape) == (1, 8) and torch.equal(bm.get_probabilities()[0], p)
    assert abs(float(bm.entropy()) - np.log(2.0)) < 1e-6
    assert float(bm.get_log_q_z_x(torch.tensor([[1.0, 1.0, 1.0]]))[0]) == pytest.approx(np.log(0.5))
    with pytest.raises(ValueError, match="is not a valid outcome"):
        bm.get_log_q_z_x(torch.tensor([[1.0, 2.0, 1.0]]))
    assert bm.sample(5).shape == (5, 3) and set(bm.get_prob_dict()) == set(bm.all_outcome_tuples)
    bm.clear_fixed_probs()
    assert bm._fixed_probs is None


def test_trainer_family_switch_on_host():
    """family absent or 'table': the table machine; 'mps': the MPS machine with the trainer's forced initialisation."""
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    from tensornetworks_amd.born_machine_classical_sim import ClassicalBornMachine
    from tensornetworks_amd.born_machine_mps import MPSBornMachine
    from tensornetworks_amd.elbo_vi import ELBOVariationalInference
    from tensornetworks_amd.ksd_vi import KSDVariationalInference
    bn = get_sprinkler_network(False)
    lat, obs = ['C', 'S', 'R'], ['W']
    for cls in (KSDVariationalInference, ELBOVariationalInference):
        assert isinstance(cls(bn, lat, obs, {'use_logits': True}).born_machine, ClassicalBornMachine)
        assert isinstance(cls(bn, lat, obs, {'family': 'table'}).born_machine, ClassicalBornMachine)
        torch.manual_seed(2)
        vi = cls(bn, lat, obs, {'family': 'mps', 'bond_dim': 2})
        torch.manual_seed(2)
        assert isinstance(vi.born_machine, MPSBornMachine) and torch.equal(vi.born_machine.cores.detach(), mm.init_cores(3, 2))
        with pytest.raises(ValueError, match="family"):
            cls(bn, lat, obs, {'family': 'tree'})
