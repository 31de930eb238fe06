"""The sampled trainers with born_machine_config['cores'] = 'tree' on the MI355X: the ELBO epochs against the float64 replay
(ttn_mirror.replay), the estimator's mean against the exact reverse-KL gradient of the mirror, one short KSD and one short MMD run
against their replays, and the real and purified configurations' bits around a tree run.

Tolerances.  The sprinkler trace takes tests/test_gpu_cmps_trainer.py's 1e-6: the derived bound of the new kernels at (n, D, B) =
(3, 2, 1024) is ttn_mirror.c_score ~ 2e2 units of 2^-52 ~ 4e-14 of an entry's absolute-term sum per epoch, far below it.  The KSD
and MMD runs compare a loss of either size (U ~ 2e3 for KSD, ~ 1e-2 for MMD) and take the same 1e-6, relative to max(1, |value|):
the losses depend on the drawn indices only (equal draws are asserted), the gradient norms on the score call."""
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import ttn_mirror as tt

pytestmark = pytest.mark.gpu

SPRINKLER_SEED = 5          # chosen on the CPU: ttn_mirror.replay has no undecided draw (asserted below)
KSD_SEED, MMD_SEED = 4, 17  # likewise
ESTIMATOR_SEED = 21         # chosen on the CPU: the mirror's own 64-epoch mean lies within 1.2 standard errors on every live entry


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def test_sprinkler_trace_against_the_replay():
    """W = 1, n = 3, D = 2, B = 1024, 60 epochs, lr 0.05: the loss and grad-norm traces equal the float64 CPU replay to 1e-6, given
    that no draw of the replay lies within 1e-8 of a decision boundary: asserted, the seed was chosen for it on the CPU.  The
    exact KL (by probabilities64) ends below where it started; the dead entries stay 0.0."""
    from tensornetworks_amd import SampledELBOVariationalInference, TreeSampledBornMachine
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    from tensornetworks_amd.stein_utils import true_posterior_table
    bn = get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    torch.manual_seed(11)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 1024, 'seed': SPRINKLER_SEED, 'cores': 'tree'}, device='cuda')
    assert type(vi.born_machine) is TreeSampledBornMachine and tuple(vi.born_machine.cores.shape) == (3, 2, 2, 2)
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    post, _ = true_posterior_table(bn, x, lat, dev())
    hist = vi.train(x, 60, 0.05, verbose=False, true_posterior_for_tvd=post)
    rep = tt.replay(cores0, 3, tt.elbo_weights(pack_network(bn, lat, x)), 1024, SPRINKLER_SEED, 60, 0.05)
    assert rep["undecided"] == 0
    worst = np.abs(np.array(hist['loss_elbo']) - np.array(rep['loss'])).max()
    worst_g = np.abs(np.array(hist['grad_norm']) - np.array(rep['grad_norm'])).max()
    print(f"worst |loss - replay| over 60 epochs: {worst:.3e}, |grad norm - replay| {worst_g:.3e}; KL {hist['kl'][0]:.4f} -> {hist['kl'][-1]:.4f}")
    assert worst <= 1e-6
    assert worst_g <= 1e-6
    assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
    assert all(s == 0 for s in hist['status']) and set(hist) == {'loss_elbo', 'grad_norm', 'logq_mean', 'status', 'tvd', 'kl'}
    assert hist['kl'][-1] < hist['kl'][0]
    final = vi.born_machine.cores.detach().cpu()
    assert bool((final[~vi.born_machine.live_mask().cpu()] == 0.0).all())


def test_estimator_is_unbiased():
    """n = 3, D = 2: the mean over 64 epochs of B = 1024 of the score-function estimate against the exact gradient of
    sum q (log q - log p) computed by the mirror over the 8 states, on every live entry within 4 standard errors of the mean, the
    standard error taken from the 64 epoch values themselves (with this seed the mirror's own 64-epoch mean lies within 1.2 on the
    CPU); the dead entries are 0."""
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import pack_network, synthetic_network
    n, D, B = 3, 2, 1024
    bn, lat, obs, x = synthetic_network(n, 0)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': ESTIMATOR_SEED, 'cores': 'tree'}, device='cuda')
    cores = tt.random_cores(n, D, 31)
    with torch.no_grad():
        vi.born_machine.cores.copy_(torch.from_numpy(cores))
    vi._prepare_observation(x)
    est = torch.stack([vi.loss_and_grad(e)[1] for e in range(64)]).cpu().numpy()
    assert est.shape == (64, 3, D, D, D)
    mean, se = est.mean(axis=0), est.std(axis=0, ddof=1) / math.sqrt(64)
    exact = hp.to_f64(tt.exact_elbo_gradient(cores, n, tt.log_joint(pack_network(bn, lat, x), tt.all_bits(n))))
    live = tt.live_mask(n, D)
    z = np.abs(mean - exact)[live] / se[live]
    print(f"worst |mean - exact| / standard error = {z.max():.2f} over {int(live.sum())} live entries")
    assert np.all(se[live] > 0) and z.max() <= 4.0
    assert np.all(exact[~live] == 0.0) and np.all(est[:, ~live] == 0.0)


def test_ksd_run_against_its_replay():
    """synthetic_network(8, 0), D = 3, B = 257, 3 epochs: U, the gradient norm and the last draws follow the replay."""
    from tensornetworks_amd import SampledKSDVariationalInference, TreeSampledBornMachine
    from tensornetworks_amd.bayesian_network import pack_network, synthetic_network
    n = 8
    bn, lat, obs, x = synthetic_network(n, 0)
    torch.manual_seed(4)
    vi = SampledKSDVariationalInference(bn, lat, obs, {'bond_dim': 3, 'num_samples': 257, 'seed': KSD_SEED, 'cores': 'tree'}, device='cuda')
    assert type(vi.born_machine) is TreeSampledBornMachine
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    hist = vi.train(x, 3, 0.02, verbose=False)
    rep = tt.replay(cores0, n, tt.ksd_weights(pack_network(bn, lat, x), n), 257, KSD_SEED, 3, 0.02)
    assert rep["undecided"] == 0 and all(s == 0 for s in hist['status'])
    assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
    print(f"KSD: worst relative |U - replay| {close(hist['loss_ksd2'], rep['loss']):.3e}, |grad norm - replay| {close(hist['grad_norm'], rep['grad_norm']):.3e}")
    assert close(hist['loss_ksd2'], rep['loss']) <= 1e-6 and close(hist['grad_norm'], rep['grad_norm']) <= 1e-6


def test_mmd_run_against_its_replay():
    """n = 6, D = 2, B = 257, 50 data points, 3 epochs: the estimate U, the gradient norm and the last draws follow the replay; the
    exact report (n <= 20) is filled."""
    from tensornetworks_amd import SampledMMDTrainer, TreeSampledBornMachine
    n, N = 6, 50
    data = torch.from_numpy(np.random.default_rng([8, n]).integers(0, 1 << n, N))
    target = torch.bincount(data, minlength=1 << n).double() / N
    torch.manual_seed(5)
    vi = SampledMMDTrainer(n, {'bond_dim': 2, 'num_samples': 257, 'seed': MMD_SEED, 'cores': 'tree'}, device='cuda')
    assert type(vi.born_machine) is TreeSampledBornMachine
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    hist = vi.train(data, 3, 0.05, verbose=False, target_for_tvd=target)
    rep = tt.replay(cores0, n, tt.mmd_weights(data.numpy(), n, vi.objective.kernel.kappa), 257, MMD_SEED, 3, 0.05)
    assert rep["undecided"] == 0 and all(s == 0 for s in hist['status'])
    assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
    print(f"MMD: worst |U - replay| {close(hist['loss_mmd2'], rep['loss']):.3e}, |grad norm - replay| {close(hist['grad_norm'], rep['grad_norm']):.3e}")
    assert close(hist['loss_mmd2'], rep['loss']) <= 1e-6 and close(hist['grad_norm'], rep['grad_norm']) <= 1e-6
    assert set(hist) == {'loss_mmd2', 'grad_norm', 'logq_mean', 'status', 'tvd', 'kl', 'mmd2_exact'} and all(len(v) == 3 for v in hist.values())
    q = vi.born_machine.probabilities64().cpu().numpy()
    assert abs(q.sum() - 1.0) <= 1e-12


def test_real_and_purified_runs_keep_their_bits_around_a_tree_run():
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(12, 0)

    def run(cores, **extra):
        torch.manual_seed(3)
        vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 3, 'num_samples': 257, 'seed': 9, 'cores': cores, **extra}, device='cuda')
        hist = vi.train(x, 3, 0.02, verbose=False)
        return hist['loss_elbo'], hist['grad_norm'], vi.last_idx.cpu().numpy().copy(), vi.born_machine.cores.detach().cpu().numpy().copy()
    before = [run('real'), run('purified', purification_dim=2)]
    tree = run('tree')
    assert all(math.isfinite(v) for v in tree[0] + tree[1]) and tree[3].shape == (15, 3, 3, 3)
    after = [run('real'), run('purified', purification_dim=2)]
    for a, b in zip(before, after):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    again = run('tree')
    assert tree[0] == again[0] and tree[1] == again[1] and np.array_equal(tree[2], again[2]) and np.array_equal(tree[3], again[3])
