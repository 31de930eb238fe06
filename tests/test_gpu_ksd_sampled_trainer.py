"""SampledKSDVariationalInference on the MI355X: the epochs against the float64 replay (ksd_sampled_mirror.replay), a run at
n = 40 that no enumerating engine can open, the estimator's unbiasedness against the exact gradient of q^T K_p q, and the
'ksd' objective's factor."""
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import ksd_sampled_mirror as km
import mps_sampled_mirror as sm
from tensornetworks_amd import backend
from tensornetworks_amd.backend import bn_score_samples, stein_pairs_rowsum  # noqa: F401  (fails at import without the feature)

pytestmark = pytest.mark.gpu
EPS = hp.EPS64


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _exact_ksd2(vi, K):
    cores, _ = vi.born_machine.kernel_input()
    _, q64, _, _ = backend.mps_probs(cores, want_q32=False)
    return float(backend.stein_quadform(K, q64, vi.num_latent_vars, want_y=False)[0].item())


def test_sprinkler_trace_against_the_replay():
    """W = 1, n = 3, D = 2, B = 1024, seed 6, 40 epochs at lr 0.05 (chosen on the CPU with the replay: no draw within 1e-8 of
    its decision boundary, asserted; U falls from 3.3e3 to 0.49): loss_ksd2 and grad_norm equal the float64 CPU replay to the
    ELBO trainer test's 1e-6.  On the CPU replay the exact q^T K_p q of the final cores is 0.37671733582779543 (3605.55 at the
    start); the GPU run's, through mps_probs and the dense quadratic form, must end below twice that and below its own start."""
    from tensornetworks_amd import SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    from tensornetworks_amd.stein_utils import true_posterior_table
    bn = get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    packed = pack_network(bn, lat, x)
    torch.manual_seed(11)
    vi = SampledKSDVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 1024, 'seed': 6}, device='cuda')
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    S_tab, _ = backend.score_from_packed(packed, 3, dev())
    K = backend.stein_gram(S_tab, 3, 1.0)
    start = _exact_ksd2(vi, K)
    post, _ = true_posterior_table(bn, x, lat, dev())
    hist = vi.train(x, 40, 0.05, verbose=False, true_posterior_for_tvd=post)
    end = _exact_ksd2(vi, K)
    rep = km.replay(cores0, packed, 1024, 6, 40, 0.05)
    assert rep["undecided"] == 0
    worst = np.abs(np.array(hist['loss_ksd2']) - np.array(rep['loss'])).max()
    worst_g = np.abs(np.array(hist['grad_norm']) - np.array(rep['grad_norm'])).max()
    print(f"worst |loss_ksd2 - replay| over 40 epochs: {worst:.3e}, |grad_norm - replay|: {worst_g:.3e}; "
          f"exact q^T K_p q {start:.4f} -> {end:.6f}; U {hist['loss_ksd2'][0]:.4f} -> {hist['loss_ksd2'][-1]:.6f}")
    assert worst <= 1e-6 and worst_g <= 1e-6
    assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
    assert all(s == 0 for s in hist['status'])
    assert set(hist) == {'loss_ksd2', 'loss_ksd', 'grad_norm', 'logq_mean', 'status', 'tvd', 'kl'}
    assert hist['loss_ksd'] == [math.sqrt(max(u, 1e-12)) for u in hist['loss_ksd2']]
    assert end < 2 * 0.37671733582779543 and end < start


def test_chain_of_forty():
    """synthetic_network(40, 0), D = 4, B = 1024, 3 epochs: finite losses, status 0, identical bits on a rerun, and the first
    epoch's U and gradient equal to the extended-precision mirror evaluated on the GPU's own samples and score rows.
    U: the row-sum kernel's bound on the total (test_gpu_ksd_sampled_kernel.py), divided by B (B - 1), one more unit for the
    division.  Gradient: w_b is known to the kernel only to dw_b -- the bounds of r_b and T through m_b and w_b, four units
    for the elementwise operations on each of their terms -- and a perturbation dw moves an entry by at most
    sum_b |dw_b| |grad log q_b| (as test_gpu_mps_sampled_trainer.py: test_chain_of_forty)."""
    from tensornetworks_amd import SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    from test_gpu_mps_sampled_kernel import c_score
    bn, lat, obs, x = synthetic_network(40, 0)
    n, D, B = 40, 4, 1024
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        vi = SampledKSDVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 9}, device='cuda')
        cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
        vi._prepare_observation(x)
        loss0, grad0, _, st0 = vi.loss_and_grad(0)
        S0 = vi.scores(vi.last_idx).cpu().numpy()
        first = (float(loss0.item()), grad0.cpu().numpy().copy(), vi.last_idx.cpu().numpy().copy(), int(st0.item()))
        hist = vi.train(x, 3, 0.02, verbose=False)
        runs.append((first, hist, vi.last_idx.cpu().numpy().copy(), vi.born_machine.cores.detach().cpu().numpy().copy()))
    (first, hist, last, cend), (first2, hist2, last2, cend2) = runs
    assert all(math.isfinite(v) for v in hist['loss_ksd2'] + hist['loss_ksd']) and all(s == 0 for s in hist['status']) and first[3] == 0
    assert 'tvd' not in hist and 'kl' not in hist
    assert np.array_equal(first[2], first2[2]) and np.array_equal(last, last2) and np.array_equal(first[1], first2[1])
    assert hist['loss_ksd2'] == hist2['loss_ksd2'] and hist['grad_norm'] == hist2['grad_norm'] and np.array_equal(cend, cend2)
    assert hist['loss_ksd2'][0] == first[0]
    # the mirror on the GPU's samples and score rows
    idx = first[2]
    K, Bt = km.kappa(idx, S0, n, 1.0)
    r, T = km.rowsums(K)
    br, bT = km.rowsums(Bt)
    U, m, w = km.weights(r, T, B)
    Ce, Cs, Ct = km.AMPLIFICATION * km.c_entry(n), km.c_sum(B), km.c_total(B)
    dT = EPS * (Ce + Cs + Ct) * bT
    ratio_U = abs(first[0] - float(U)) / float((dT + EPS * abs(T)) / (B * (B - 1)))
    dr = EPS * (Ce + Cs) * br
    dm = (dT + 2 * dr) / ((B - 1) * (B - 2)) + 4 * EPS * (np.abs(T) + 2 * np.abs(r)) / ((B - 1) * (B - 2))
    dw = (2.0 / B) * (dr / (B - 1) + dm) + 4 * EPS * (2.0 / B) * (np.abs(r) / (B - 1) + np.abs(m))
    bits = sm.bits_of_idx(idx, n)
    env = sm.environments(cores0)
    ref = sm.score_gradient(cores0, bits, hp.to_f64(w), env)
    pert = sm.score_gradient(cores0, bits, hp.to_f64(dw) + EPS * np.abs(hp.to_f64(w)), env)["grad_abs"]
    kZ = float(env["Z_abs"] / env["Z"])
    Cg = c_score(n, D, B, float(ref["kappa"].max()), kZ)
    err = np.abs(hp.to_f64(first[1].astype(sm.LD) - ref["grad"]))
    bound = hp.to_f64(Cg * EPS * ref["grad_abs"] + pert)
    print(f"n=40: U {first[0]:.6e}, error / bound = {ratio_U:.4f}; worst gradient error / bound = "
          f"{np.max(err / np.where(bound > 0, bound, 1)):.3f}")
    assert ratio_U <= 1.0
    assert np.all(err <= bound)


def test_estimator_is_unbiased():
    """n = 4, D = 2, B = 1024: the mean over 64 epochs of the estimate against the exact gradient of q^T K_p q (mps_probs,
    y = 2 K_p q by the dense contraction, mps_vjp), entry by entry within 6 standard errors of the mean, the standard error
    taken from the 64 epoch values themselves; the entries that do not enter psi are exactly 0 in every epoch and in the exact
    gradient."""
    from tensornetworks_amd import SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network, pack_network
    bn, lat, obs, x = synthetic_network(4, 0)
    torch.manual_seed(1)
    vi = SampledKSDVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 1024, 'seed': 21}, device='cuda')
    vi._prepare_observation(x)
    out = [vi.loss_and_grad(e) for e in range(64)]
    est = torch.stack([o[1] for o in out]).cpu().numpy()
    Us = torch.stack([o[0] for o in out]).cpu().numpy()
    mean, se = est.mean(axis=0), est.std(axis=0, ddof=1) / math.sqrt(64)
    S_tab, _ = backend.score_from_packed(pack_network(bn, lat, x), 4, dev())
    K = backend.stein_gram(S_tab, 4, 1.0)
    cores, _ = vi.born_machine.kernel_input()
    _, q64, _, _ = backend.mps_probs(cores, want_q32=False)
    ksd2, y = backend.stein_quadform(K, q64, 4)
    backend.mps_probs(cores, want_q32=False)
    exact = backend.mps_vjp(cores, (2.0 * y).reshape(-1).contiguous()).cpu().numpy()
    z = np.abs(mean - exact) / np.where(se > 0, se, 1)
    zU = abs(Us.mean() - float(ksd2.item())) / (Us.std(ddof=1) / math.sqrt(64))
    print(f"worst |mean - exact| / standard error = {z.max():.2f} over {int((se > 0).sum())} entries; U: {zU:.2f}")
    assert np.all(np.abs(mean - exact) <= 6 * se + 1e-15)
    assert np.all(exact[se == 0] == 0.0)
    assert zU <= 6.0


def test_ksd_objective_scales_the_weights():
    """objective='ksd': epoch 0's gradient is the score-function gradient of w / (2 sqrt(U)) bit for bit (w and U those of
    'ksd2' on the same draws), and so 1 / (2 sqrt(U)) times the 'ksd2' gradient up to the rounding of the B products."""
    from tensornetworks_amd import SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(12, 0)
    made = {}
    for objective in ('ksd2', 'ksd'):
        torch.manual_seed(2)
        vi = SampledKSDVariationalInference(bn, lat, obs, {'bond_dim': 3, 'num_samples': 257, 'seed': 4}, device='cuda',
                                            base_kernel_length_scale=0.25, objective=objective)
        vi._prepare_observation(x)
        U, grad, _, st = vi.loss_and_grad(0)
        made[objective] = (vi, U.clone(), grad.clone(), vi.last_idx.clone())
        assert int(st.item()) == 0
    (vi2, U2, g2, i2), (vi1, U1, g1, i1) = made['ksd2'], made['ksd']
    assert torch.equal(i1, i2) and torch.equal(U1, U2) and float(U2.item()) > 1e-12
    cores, idx, logq, _ = vi2.draw(0)
    _, w = vi2.sample_weights(idx, logq)
    factor = 0.5 / torch.sqrt(U2)
    want, _, _ = backend.mps_score_vjp(cores, idx, (w * factor).contiguous())
    assert torch.equal(want, g1)
    scale = float(factor.item())
    assert torch.allclose(g1, scale * g2, rtol=1e-10, atol=1e-12 * float(g2.abs().max()) * scale)
