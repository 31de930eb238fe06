"""The sampled MPS trainers with natural_gradient='cg' on the MI355X: the Sprinkler traces of
test_gpu_sample_gram_trainer.py against the float64 blocks='full' replay (a converged CG solves the same system), and the
forty-variable chain at a sample count that 'sample' refuses."""
import math

import numpy as np
import pytest
import torch

import sampled_fisher_mirror as fm
from tensornetworks_amd.backend import cg_step, mps_score_jvp  # noqa: F401  (fails without the feature)
from tensornetworks_amd.natural_gradient import CGFisherPreconditioner

pytestmark = pytest.mark.gpu
TRACE = {"elbo": dict(seed=5, key="loss_elbo", damping=1e-3), "ksd": dict(seed=6, key="loss_ksd2", damping=1e-1)}
EPOCHS, LR, B = 10, 0.05, 1024


def _trainer(kind):
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    return SampledELBOVariationalInference if kind == "elbo" else SampledKSDVariationalInference


@pytest.mark.parametrize("kind", ["elbo", "ksd"])
def test_sprinkler_trace_against_the_full_replay(kind):
    """W = 1, n = 3, D = 2, B = 1024, SGD without momentum at lr 0.05, the seeds and dampings of the sample-space test, 10
    epochs (the float64 replay runs a Cholesky per epoch).  CGFisherPreconditioner(lam, max_iters=64, rel_tol=1e-10): P = 24,
    so CG ends within 25 steps in exact arithmetic.  Loss and step norm within 1e-6 of the float64 blocks='full' replay, the
    tolerance the other routes are held to against the same reference; no fallback; natgrad_iters recorded."""
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    seed, key, lam = TRACE[kind]["seed"], TRACE[kind]["key"], TRACE[kind]["damping"]
    bn = get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    torch.manual_seed(11)
    pre = CGFisherPreconditioner(lam, max_iters=64, rel_tol=1e-10)
    vi = _trainer(kind)(bn, lat, obs, {'bond_dim': 2, 'num_samples': B, 'seed': seed}, device='cuda', natural_gradient=pre)
    assert vi.natural_gradient is pre
    packed = pack_network(bn, lat, x)
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    hist = vi.train(x, EPOCHS, LR, verbose=False, optimizer_type="sgd", sgd_momentum=0.0)
    full = fm.replay(kind, cores0, packed, B, seed, EPOCHS, LR, lam, "full", momentum=0.0)
    assert full["undecided"] == 0
    worst = np.abs(np.array(hist[key]) - np.array(full['loss'])).max()
    worst_g = np.abs(np.array(hist['grad_norm']) - np.array(full['grad_norm'])).max()
    print(f"{kind} against the blocks='full' replay: worst |loss - replay| over {EPOCHS} epochs: {worst:.3e}, "
          f"|grad_norm - replay|: {worst_g:.3e}; loss {hist[key][0]:.4f} -> {hist[key][-1]:.4f}, CG iterations "
          f"{hist['natgrad_iters']}, last relres {float(pre.relres.item()):.2e}")
    assert worst <= 1e-6 and worst_g <= 1e-6
    assert np.array_equal(vi.last_idx.cpu().numpy(), full["idx"][-1])
    assert full['natgrad_info'] == [0] * EPOCHS
    assert all(s == 0 for s in hist['status'])
    assert hist['natgrad_info'] == [0] * EPOCHS and pre.info.tolist() == [0]
    assert len(hist['natgrad_iters']) == EPOCHS and all(1 <= k <= 64 for k in hist['natgrad_iters'])
    assert set(hist) == {key, 'grad_norm', 'logq_mean', 'status', 'natgrad_info', 'natgrad_iters'} \
        | ({'loss_ksd'} if kind == "ksd" else set())


@pytest.mark.parametrize("kind", ["elbo", "ksd"])
def test_chain_of_forty(kind):
    """synthetic_network(40, 0), D = 4, num_samples = 2048 with 'cg': P = 1280 and B = 2048, which blocks='full' and 'sample'
    both refuse.  3 epochs: finite losses, status 0, no fallback, the same bits on a rerun."""
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(40, 0)
    key = TRACE[kind]["key"]
    cfg = {'bond_dim': 4, 'num_samples': 2048, 'seed': 9}
    for spec in ('sample', 'full'):
        with pytest.raises(ValueError):
            _trainer(kind)(bn, lat, obs, cfg, device='cuda', natural_gradient=spec)
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        vi = _trainer(kind)(bn, lat, obs, cfg, device='cuda', natural_gradient='cg')
        hist = vi.train(x, 3, 0.02, verbose=False)
        runs.append((hist, vi.last_idx.cpu().numpy().copy(), vi.born_machine.cores.detach().cpu().numpy().copy(),
                     vi.natural_gradient.info.tolist()))
    (hist, last, cend, info), (hist2, last2, cend2, info2) = runs
    print(f"{kind}: losses {hist[key]}, CG iterations {hist['natgrad_iters']}")
    assert all(math.isfinite(v) for v in hist[key] + hist['grad_norm']) and all(s == 0 for s in hist['status'])
    assert hist['natgrad_info'] == [0, 0, 0] and info == [0] == info2
    assert all(1 <= k <= CGFisherPreconditioner.MAX_ITERS for k in hist['natgrad_iters'])
    assert hist[key] == hist2[key] and hist['grad_norm'] == hist2['grad_norm'] and hist['natgrad_iters'] == hist2['natgrad_iters']
    assert np.array_equal(last, last2) and np.array_equal(cend, cend2)
