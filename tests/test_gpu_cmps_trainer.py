"""The sampled trainers with born_machine_config['cores'] = 'complex' on the MI355X: the ELBO epochs against the float64 replay
(cmps_mirror.replay), the estimator's unbiasedness against the exact reverse-KL gradient of the mirror, a run at n = 40, and the
KSD trainer's epochs."""
import math

import numpy as np
import pytest
import torch

import cmps_mirror as cx
import hp_reference as hp

pytestmark = pytest.mark.gpu

SPRINKLER_SEED = 5          # chosen on the CPU: cmps_mirror.replay has no undecided draw (asserted below)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def test_sprinkler_trace_against_the_replay():
    """W = 1, n = 3, D = 2 complex, B = 1024, 60 epochs, lr 0.05: the loss and grad-norm traces equal the float64 CPU replay to
    1e-6 (the real trainer test's bound), given that no draw of the replay lies within 1e-8 of its decision boundary: asserted,
    the seed was chosen for it on the CPU.  The exact KL (by probabilities64) ends below where it started."""
    from tensornetworks_amd import ComplexSampledMPSBornMachine, SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    from tensornetworks_amd.stein_utils import true_posterior_table
    bn = get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    torch.manual_seed(11)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 1024, 'seed': SPRINKLER_SEED, 'cores': 'complex'},
                                         device='cuda')
    assert type(vi.born_machine) is ComplexSampledMPSBornMachine
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    post, _ = true_posterior_table(bn, x, lat, dev())
    hist = vi.train(x, 60, 0.05, verbose=False, true_posterior_for_tvd=post)
    rep = cx.replay(cores0, pack_network(bn, lat, x), 1024, SPRINKLER_SEED, 60, 0.05)
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
    """n = 4, D = 2: the mean over 64 epochs of B = 4096 of the score-function estimate against the exact gradient of
    sum q (log q - log p) computed by the mirror over the 16 states, entry by entry within 6 standard errors of the mean, the
    standard error taken from the 64 epoch values themselves; entries with zero spread (those that do not enter psi) are exactly 0."""
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import pack_network, synthetic_network
    bn, lat, obs, x = synthetic_network(4, 0)
    torch.manual_seed(1)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 4096, 'seed': 21, 'cores': 'complex'}, device='cuda')
    vi._prepare_observation(x)
    est = torch.stack([vi.loss_and_grad(e)[1] for e in range(64)]).cpu().numpy()
    assert est.shape == (64, 4, 2, 2, 2, 2)
    mean, se = est.mean(axis=0), est.std(axis=0, ddof=1) / math.sqrt(64)
    cores = vi.born_machine.cores.detach().cpu().numpy()
    logp = cx.log_joint(pack_network(bn, lat, x), cx.all_bits(4))
    exact = hp.to_f64(cx.exact_elbo_gradient(cores, logp))
    z = np.abs(mean - exact) / np.where(se > 0, se, 1)
    print(f"worst |mean - exact| / standard error = {z.max():.2f} over {int((se > 0).sum())} entries")
    assert int((se > 0).sum()) >= 32
    assert np.all(np.abs(mean - exact) <= 6 * se + 1e-15)
    assert np.all(exact[se == 0] == 0.0) and np.all(mean[se == 0] == 0.0)


def test_chain_of_forty():
    """synthetic_network(40, 0), D = 4 complex, B = 1024, 5 epochs: finite losses, status 0, a rerun is identical, and the first
    epoch's loss and gradient lie within the derived bound of the extended mirror evaluated on the GPU's own samples."""
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network, pack_network
    bn, lat, obs, x = synthetic_network(40, 0)
    n, D, B = 40, 4, 1024
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 9, 'cores': 'complex'}, device='cuda')
        cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
        vi._prepare_observation(x)
        loss0, grad0, _, st0 = vi.loss_and_grad(0)
        first = (float(loss0.item()), grad0.cpu().numpy().copy(), vi.last_idx.cpu().numpy().copy(), int(st0.item()))
        hist = vi.train(x, 5, 0.02, verbose=False)
        runs.append((first, hist, vi.last_idx.cpu().numpy().copy(), vi.born_machine.cores.detach().cpu().numpy().copy()))
    (first, hist, last, cend), (first2, hist2, last2, cend2) = runs
    assert all(math.isfinite(v) for v in hist['loss_elbo']) and all(s == 0 for s in hist['status']) and first[3] == 0
    assert 'tvd' not in hist and 'kl' not in hist
    assert np.array_equal(first[2], first2[2]) and np.array_equal(last, last2) and hist['loss_elbo'] == hist2['loss_elbo']
    assert hist['grad_norm'] == hist2['grad_norm'] and np.array_equal(cend, cend2)
    assert hist['loss_elbo'][0] == first[0]
    # the mirror on the GPU's samples
    bits = cx.bits_of_idx(first[2], n)
    env = cx.environments(cores0)
    logp = cx.log_joint(pack_network(bn, lat, x), bits)
    lq = cx.conditionals(cores0, bits, env)
    f = hp.to_f64(lq["logq"]) - logp
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(lq["psi_abs"] / np.abs(lq["psi"]))
    ferr = hp.EPS64 * (cx.logq_bound(n, D, kb, kZ, hp.to_f64(lq["logq"]), float(np.log(env["Z"]))) + 45 * np.abs(logp) + 2 * np.abs(f))
    assert abs(first[0] - f.mean()) <= ferr.mean() + hp.EPS64 * 16 * np.abs(f).mean()
    w = (f - f.mean()) / (B - 1)
    ref = cx.score_gradient(cores0, bits, w, env)
    # w itself is known to the kernel only to ferr (and the mean's): a perturbation dw moves an entry by at most sum |dw_b| |grad log q_b|
    dw = (ferr + ferr.mean() + hp.EPS64 * 16 * np.abs(f).mean() + 4 * hp.EPS64 * np.abs(f - f.mean())) / (B - 1)
    pert = cx.score_gradient(cores0, bits, dw, env)["grad_abs"]
    C = cx.c_score(n, D, B, float(ref["kappa"].max()), kZ)
    err = np.abs(hp.to_f64(first[1].astype(cx.LD) - ref["grad"]))
    bound = hp.to_f64(C * hp.EPS64 * ref["grad_abs"] + pert)
    print(f"n=40: loss {first[0]:.6f}, worst gradient error / bound = {np.max(err / np.where(bound > 0, bound, 1)):.3f}")
    assert np.all(err <= bound)


def test_ksd_trainer_runs_with_complex_cores():
    """n = 12, 3 epochs: finite U, status 0, and a rerun is identical (KSD needs idx and logq of the machine only)."""
    from tensornetworks_amd import ComplexSampledMPSBornMachine, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(12, 0)
    runs = []
    for _ in range(2):
        torch.manual_seed(4)
        vi = SampledKSDVariationalInference(bn, lat, obs, {'bond_dim': 3, 'num_samples': 257, 'seed': 4, 'cores': 'complex'}, device='cuda')
        assert type(vi.born_machine) is ComplexSampledMPSBornMachine
        hist = vi.train(x, 3, 0.02, verbose=False)
        runs.append((hist, vi.last_idx.cpu().numpy().copy(), vi.born_machine.cores.detach().cpu().numpy().copy()))
    (hist, last, cend), (hist2, last2, cend2) = runs
    assert len(hist['loss_ksd2']) == 3 and all(math.isfinite(v) for v in hist['loss_ksd2'] + hist['loss_ksd'] + hist['grad_norm'])
    assert all(s == 0 for s in hist['status'])
    assert hist['loss_ksd2'] == hist2['loss_ksd2'] and hist['grad_norm'] == hist2['grad_norm']
    assert np.array_equal(last, last2) and np.array_equal(cend, cend2)
