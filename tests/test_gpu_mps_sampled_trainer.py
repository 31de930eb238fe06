"""SampledELBOVariationalInference on the MI355X: the epochs against the float64 replay (mps_sampled_mirror.replay), a run at
n = 40 that no enumerating engine can open, and the estimator's unbiasedness against the exact reverse-KL gradient."""
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_mirror as mm
import mps_sampled_mirror as sm
from tensornetworks_amd import backend
from tensornetworks_amd.backend import mps_environments, mps_sample, mps_score_vjp, bn_logjoint_samples  # noqa: F401

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def test_sprinkler_trace_against_the_replay():
    """W = 1, n = 3, D = 2, B = 1024, 60 epochs: the loss trace equals the float64 CPU replay to 1e-6 (the bound of the MPS
    trainer test), given that no draw of the replay lies within 1e-8 of its decision boundary: asserted, the seed was chosen
    for it on the CPU.  The exact KL (by mps_probs) ends below where it started."""
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    from tensornetworks_amd.stein_utils import true_posterior_table
    bn = get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    torch.manual_seed(11)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 1024, 'seed': 5}, device='cuda')
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    post, _ = true_posterior_table(bn, x, lat, dev())
    hist = vi.train(x, 60, 0.05, verbose=False, true_posterior_for_tvd=post)
    rep = sm.replay(cores0, pack_network(bn, lat, x), 1024, 5, 60, 0.05)
    assert rep["undecided"] == 0
    worst = np.abs(np.array(hist['loss_elbo']) - np.array(rep['loss'])).max()
    print(f"worst |loss - replay| over 60 epochs: {worst:.3e}; KL {hist['kl'][0]:.4f} -> {hist['kl'][-1]:.4f}")
    assert worst <= 1e-6
    assert np.abs(np.array(hist['grad_norm']) - np.array(rep['grad_norm'])).max() <= 1e-6
    assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
    assert all(s == 0 for s in hist['status']) and set(hist) == {'loss_elbo', 'grad_norm', 'logq_mean', 'status', 'tvd', 'kl'}
    assert hist['kl'][-1] < hist['kl'][0]


def test_chain_of_forty():
    """synthetic_network(40, 0), D = 4, B = 1024, 5 epochs: finite losses, status 0, the same idx on a rerun, and the first
    epoch's loss and gradient equal to the extended-precision mirror evaluated on the GPU's own samples."""
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network, pack_network
    from test_gpu_mps_sampled_kernel import c_score, logq_bound
    bn, lat, obs, x = synthetic_network(40, 0)
    n, D, B = 40, 4, 1024
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 9}, device='cuda')
        cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
        vi._prepare_observation(x)
        loss0, grad0, _, st0 = vi.loss_and_grad(0)
        first = (float(loss0.item()), grad0.cpu().numpy().copy(), vi.last_idx.cpu().numpy().copy(), int(st0.item()))
        hist = vi.train(x, 5, 0.02, verbose=False)
        runs.append((first, hist, vi.last_idx.cpu().numpy().copy()))
    (first, hist, last), (first2, hist2, last2) = runs
    assert all(math.isfinite(v) for v in hist['loss_elbo']) and all(s == 0 for s in hist['status']) and first[3] == 0
    assert 'tvd' not in hist and 'kl' not in hist
    assert np.array_equal(first[2], first2[2]) and np.array_equal(last, last2) and hist['loss_elbo'] == hist2['loss_elbo']
    assert hist['loss_elbo'][0] == first[0]
    # the mirror on the GPU's samples
    bits = sm.bits_of_idx(first[2], n)
    env = sm.environments(cores0)
    logp = sm.log_joint(pack_network(bn, lat, x), bits)
    lq = sm.conditionals(cores0, bits, env)
    f = hp.to_f64(lq["logq"]) - logp
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(lq["psi_abs"] / np.abs(lq["psi"]))
    ferr = hp.EPS64 * (logq_bound(n, D, kb, kZ, hp.to_f64(lq["logq"]), float(np.log(env["Z"]))) + 45 * np.abs(logp) + 2 * np.abs(f))
    assert abs(first[0] - f.mean()) <= ferr.mean() + hp.EPS64 * 16 * np.abs(f).mean()
    w = (f - f.mean()) / (B - 1)
    ref = sm.score_gradient(cores0, bits, w, env)
    # w itself is known to the kernel only to ferr (and the mean's): a perturbation dw moves an entry by at most sum |dw_b| |grad log q_b|
    dw = (ferr + ferr.mean() + hp.EPS64 * 16 * np.abs(f).mean() + 4 * hp.EPS64 * np.abs(f - f.mean())) / (B - 1)
    pert = sm.score_gradient(cores0, bits, dw, env)["grad_abs"]
    C = c_score(n, D, B, float(ref["kappa"].max()), kZ)
    err = np.abs(hp.to_f64(first[1].astype(sm.LD) - ref["grad"]))
    bound = hp.to_f64(C * hp.EPS64 * ref["grad_abs"] + pert)
    print(f"n=40: loss {first[0]:.6f}, worst gradient error / bound = {np.max(err / np.where(bound > 0, bound, 1)):.3f}")
    assert np.all(err <= bound)


def test_estimator_is_unbiased():
    """n = 4, D = 2: the mean over 64 epochs of B = 4096 of the score-function estimate against the exact gradient of
    sum q (log q - log p) (mps_vjp with g = bornvi_elbo_weights' w), entry by entry within 6 standard errors of the mean,
    the standard error taken from the 64 epoch values themselves (2 n D^2 = 32 entries; those that do not enter psi are exactly 0
    in every epoch and in the exact gradient)."""
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    from tensornetworks_amd.elbo_objective import ElboObjective
    bn, lat, obs, x = synthetic_network(4, 0)
    torch.manual_seed(1)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 4096, 'seed': 21}, device='cuda')
    vi._prepare_observation(x)
    est = torch.stack([vi.loss_and_grad(e)[1] for e in range(64)]).cpu().numpy()
    mean, se = est.mean(axis=0), est.std(axis=0, ddof=1) / math.sqrt(64)
    obj = ElboObjective(bn, lat, 'cuda')
    obj.prepare(x)
    cores, _ = vi.born_machine.kernel_input()
    _, q64, _, _ = backend.mps_probs(cores, want_q32=False)
    _, _, dldq = obj.weights(q64)
    backend.mps_probs(cores, want_q32=False)
    exact = backend.mps_vjp(cores, dldq.reshape(-1).contiguous()).cpu().numpy()
    z = np.abs(mean - exact) / np.where(se > 0, se, 1)
    print(f"worst |mean - exact| / standard error = {z.max():.2f} over {int((se > 0).sum())} entries")
    assert np.all(np.abs(mean - exact) <= 6 * se + 1e-15)
    assert np.all(exact[se == 0] == 0.0)
