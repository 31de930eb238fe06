"""The sampled trainers with born_machine_config['cores'] = 'purified' on the MI355X: the ELBO epochs against the float64 replay
(lps_mirror.replay), the estimator's mean against the exact reverse-KL gradient of the mirror, one short KSD and one short MMD run
against their replays, and the real and complex configurations' bits around a purified run.

Tolerances.  The sprinkler trace takes tests/test_gpu_cmps_trainer.py's 1e-6: the derived bound of the new kernels at (n, m, D, B) =
(3, 2, 2, 1024) is lps_mirror.c_score ~ 1e3 units of 2^-52 ~ 2e-13 of an entry's absolute-term sum per epoch, far below it, so the
complex family's tolerance stands.  The KSD and MMD runs compare a loss of either size (U ~ 2e3 for KSD, ~ 1e-2 for MMD) and take
the same 1e-6, relative to max(1, |value|): the losses depend on the drawn indices only (equal draws are asserted), the gradient
norms on the score call, whose derived bound is again ~ 1e-13 relative."""
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import lps_mirror as lp

pytestmark = pytest.mark.gpu

SPRINKLER_SEED = 5          # chosen on the CPU: lps_mirror.replay has no undecided draw (asserted below)
KSD_SEED, MMD_SEED = 4, 17  # likewise


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def test_sprinkler_trace_against_the_replay():
    """W = 1, n = 3, D = 2, m = 2, B = 1024, 60 epochs, lr 0.05: the loss and grad-norm traces equal the float64 CPU replay to
    1e-6, given that no draw of the replay lies within 1e-8 of a decision boundary: asserted, the seed was chosen for it on the
    CPU.  The exact KL (by probabilities64) ends below where it started."""
    from tensornetworks_amd import PurifiedSampledMPSBornMachine, SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    from tensornetworks_amd.stein_utils import true_posterior_table
    bn = get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    torch.manual_seed(11)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 1024, 'seed': SPRINKLER_SEED, 'cores': 'purified',
                                                        'purification_dim': 2}, device='cuda')
    assert type(vi.born_machine) is PurifiedSampledMPSBornMachine and tuple(vi.born_machine.cores.shape) == (3, 2, 2, 2, 2)
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    post, _ = true_posterior_table(bn, x, lat, dev())
    hist = vi.train(x, 60, 0.05, verbose=False, true_posterior_for_tvd=post)
    rep = lp.replay(cores0, lp.elbo_weights(pack_network(bn, lat, x)), 1024, SPRINKLER_SEED, 60, 0.05)
    assert rep["undecided"] == 0
    worst = np.abs(np.array(hist['loss_elbo']) - np.array(rep['loss'])).max()
    worst_g = np.abs(np.array(hist['grad_norm']) - np.array(rep['grad_norm'])).max()
    print(f"worst |loss - replay| over 60 epochs: {worst:.3e}, |grad norm - replay| {worst_g:.3e}; KL {hist['kl'][0]:.4f} -> {hist['kl'][-1]:.4f}")
    assert worst <= 1e-6
    assert worst_g <= 1e-6
    assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
    assert all(s == 0 for s in hist['status']) and set(hist) == {'loss_elbo', 'grad_norm', 'logq_mean', 'status', 'tvd', 'kl'}
    assert hist['kl'][-1] < hist['kl'][0]


def test_estimator_is_unbiased():
    """n = 3, D = 2, m = 2: the mean over 64 epochs of B = 1024 of the score-function estimate against the exact gradient of
    sum q (log q - log p) computed by the mirror over the 8 states, entry by entry within 5 standard errors of the mean, the
    standard error taken from the 64 epoch values themselves (test_lps_host.py::test_mirror_gradient_estimate_is_unbiased shows on
    the CPU that the mirror's own 64-epoch mean, same cores and seed, satisfies this); entries that do not enter psi are 0."""
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import pack_network, synthetic_network
    n, m, D, B = 3, 2, 2, 1024
    bn, lat, obs, x = synthetic_network(n, 0)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'purification_dim': m, 'num_samples': B, 'seed': 21, 'cores': 'purified'},
                                         device='cuda')
    cores = lp.random_cores(n, m, D, 31)
    with torch.no_grad():
        vi.born_machine.cores.copy_(torch.from_numpy(cores))
    vi._prepare_observation(x)
    est = torch.stack([vi.loss_and_grad(e)[1] for e in range(64)]).cpu().numpy()
    assert est.shape == (64, n, 2, m, D, D)
    mean, se = est.mean(axis=0), est.std(axis=0, ddof=1) / math.sqrt(64)
    exact = hp.to_f64(lp.exact_elbo_gradient(cores, lp.log_joint(pack_network(bn, lat, x), lp.all_bits(n))))
    z = np.abs(mean - exact) / np.where(se > 0, se, 1)
    print(f"worst |mean - exact| / standard error = {z.max():.2f} over {int((se > 0).sum())} entries")
    assert int((se > 0).sum()) >= 24
    assert np.all(np.abs(mean - exact) <= 5 * se + 1e-15)
    assert np.all(exact[se == 0] == 0.0) and np.all(mean[se == 0] == 0.0)


def test_ksd_run_against_its_replay():
    """synthetic_network(8, 0), D = 3, m = 2, B = 257, 3 epochs: U, the gradient norm and the last draws follow the replay."""
    from tensornetworks_amd import PurifiedSampledMPSBornMachine, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import pack_network, synthetic_network
    n = 8
    bn, lat, obs, x = synthetic_network(n, 0)
    torch.manual_seed(4)
    vi = SampledKSDVariationalInference(bn, lat, obs, {'bond_dim': 3, 'purification_dim': 2, 'num_samples': 257, 'seed': KSD_SEED,
                                                       'cores': 'purified'}, device='cuda')
    assert type(vi.born_machine) is PurifiedSampledMPSBornMachine
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    hist = vi.train(x, 3, 0.02, verbose=False)
    rep = lp.replay(cores0, lp.ksd_weights(pack_network(bn, lat, x), n), 257, KSD_SEED, 3, 0.02)
    assert rep["undecided"] == 0 and all(s == 0 for s in hist['status'])
    assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
    print(f"KSD: worst relative |U - replay| {close(hist['loss_ksd2'], rep['loss']):.3e}, |grad norm - replay| {close(hist['grad_norm'], rep['grad_norm']):.3e}")
    assert close(hist['loss_ksd2'], rep['loss']) <= 1e-6 and close(hist['grad_norm'], rep['grad_norm']) <= 1e-6


def test_mmd_run_against_its_replay():
    """n = 6, D = 2, m = 2, B = 257, 50 data points, 3 epochs: the estimate U, the gradient norm and the last draws follow the
    replay; the exact report (n <= 20) is filled."""
    from tensornetworks_amd import PurifiedSampledMPSBornMachine, SampledMMDTrainer
    n, N = 6, 50
    data = torch.from_numpy(np.random.default_rng([8, n]).integers(0, 1 << n, N))
    target = torch.bincount(data, minlength=1 << n).double() / N
    torch.manual_seed(5)
    vi = SampledMMDTrainer(n, {'bond_dim': 2, 'purification_dim': 2, 'num_samples': 257, 'seed': MMD_SEED, 'cores': 'purified'}, device='cuda')
    assert type(vi.born_machine) is PurifiedSampledMPSBornMachine
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    hist = vi.train(data, 3, 0.05, verbose=False, target_for_tvd=target)
    rep = lp.replay(cores0, lp.mmd_weights(data.numpy(), n, vi.objective.kernel.kappa), 257, MMD_SEED, 3, 0.05)
    assert rep["undecided"] == 0 and all(s == 0 for s in hist['status'])
    assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
    print(f"MMD: worst |U - replay| {close(hist['loss_mmd2'], rep['loss']):.3e}, |grad norm - replay| {close(hist['grad_norm'], rep['grad_norm']):.3e}")
    assert close(hist['loss_mmd2'], rep['loss']) <= 1e-6 and close(hist['grad_norm'], rep['grad_norm']) <= 1e-6
    assert set(hist) == {'loss_mmd2', 'grad_norm', 'logq_mean', 'status', 'tvd', 'kl', 'mmd2_exact'} and all(len(v) == 3 for v in hist.values())
    q = vi.born_machine.probabilities64().cpu().numpy()
    assert abs(q.sum() - 1.0) <= 1e-12


def test_real_and_complex_runs_keep_their_bits_around_a_purified_run():
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(12, 0)

    def run(cores, **extra):
        torch.manual_seed(3)
        vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 3, 'num_samples': 257, 'seed': 9, 'cores': cores, **extra}, device='cuda')
        hist = vi.train(x, 3, 0.02, verbose=False)
        return hist['loss_elbo'], hist['grad_norm'], vi.last_idx.cpu().numpy().copy(), vi.born_machine.cores.detach().cpu().numpy().copy()
    before = [run('real'), run('complex')]
    pur = run('purified', purification_dim=3)
    assert all(math.isfinite(v) for v in pur[0] + pur[1]) and pur[3].shape == (12, 2, 3, 3, 3)
    after = [run('real'), run('complex')]
    for a, b in zip(before, after):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    again = run('purified', purification_dim=3)
    assert pur[0] == again[0] and pur[1] == again[1] and np.array_equal(pur[2], again[2]) and np.array_equal(pur[3], again[3])
