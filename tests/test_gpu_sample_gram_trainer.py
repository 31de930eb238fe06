"""The sampled MPS trainers with natural_gradient='sample' on the MI355X: the Sprinkler traces of
test_gpu_sampled_natgrad_trainer.py against the float64 replays (the sample-space one, sample_gram_mirror.replay, and the
primal sampled_fisher_mirror.replay with blocks='full'), and the forty-variable chain that blocks='full' refuses, its first
step against the mirror's extended-precision primal solve at P = 1280."""
import functools
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_sampled_mirror as sm
import sample_gram_mirror as gm
import sampled_fisher_mirror as fm
from tensornetworks_amd.backend import mps_score_sample_gram  # noqa: F401  (fails without the feature)
from tensornetworks_amd.natural_gradient import SampleSpaceFisherPreconditioner

pytestmark = pytest.mark.gpu
EPS = hp.EPS64
TRACE = {"elbo": dict(seed=5, key="loss_elbo", spec='sample', damping=1e-3),
         "ksd": dict(seed=6, key="loss_ksd2", spec=1e-1, damping=1e-1)}
EPOCHS, LR, B = 40, 0.05, 1024


def _trainer(kind):
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    return SampledELBOVariationalInference if kind == "elbo" else SampledKSDVariationalInference


@pytest.mark.parametrize("kind", ["elbo", "ksd"])
def test_sprinkler_trace_against_the_replays(kind):
    """W = 1, n = 3, D = 2, B = 1024, SGD without momentum at lr 0.05, 40 epochs, the seeds of the site-block test (no draw
    within 1e-8 of its decision boundary, asserted).  ELBO with 'sample' (damping 1e-3), KSD with
    SampleSpaceFisherPreconditioner(1e-1) (at 1e-3 the float64 replays themselves differ by 2.6e-6 in the step norm).  Loss
    and step norm within 1e-6 of the float64 sample-space replay and of the float64 blocks='full' replay; no failed solve."""
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    seed, key, lam = TRACE[kind]["seed"], TRACE[kind]["key"], TRACE[kind]["damping"]
    spec = 'sample' if TRACE[kind]["spec"] == 'sample' else SampleSpaceFisherPreconditioner(lam)
    bn = get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    torch.manual_seed(11)
    vi = _trainer(kind)(bn, lat, obs, {'bond_dim': 2, 'num_samples': B, 'seed': seed}, device='cuda', natural_gradient=spec)
    assert isinstance(vi.natural_gradient, SampleSpaceFisherPreconditioner) and vi.natural_gradient.damping == lam
    packed = pack_network(bn, lat, x)
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    hist = vi.train(x, EPOCHS, LR, verbose=False, optimizer_type="sgd", sgd_momentum=0.0)
    dual = gm.replay(kind, cores0, packed, B, seed, EPOCHS, LR, lam)
    full = fm.replay(kind, cores0, packed, B, seed, EPOCHS, LR, lam, "full", momentum=0.0)
    assert dual["undecided"] == 0 and full["undecided"] == 0
    for name, rep in (("sample-space", dual), ("blocks='full'", full)):
        worst = np.abs(np.array(hist[key]) - np.array(rep['loss'])).max()
        worst_g = np.abs(np.array(hist['grad_norm']) - np.array(rep['grad_norm'])).max()
        print(f"{kind} against the {name} replay: worst |loss - replay| over {EPOCHS} epochs: {worst:.3e}, "
              f"|grad_norm - replay|: {worst_g:.3e}; loss {hist[key][0]:.4f} -> {hist[key][-1]:.4f}, "
              f"largest step norm {max(hist['grad_norm']):.3f}")
        assert worst <= 1e-6 and worst_g <= 1e-6
        assert np.array_equal(vi.last_idx.cpu().numpy(), rep["idx"][-1])
        assert rep['natgrad_info'] == [0] * EPOCHS
    assert all(s == 0 for s in hist['status'])
    assert hist['natgrad_info'] == [0] * EPOCHS and vi.natural_gradient.info.tolist() == [0]
    assert set(hist) == {key, 'grad_norm', 'logq_mean', 'status', 'natgrad_info'} | ({'loss_ksd'} if kind == "ksd" else set())


@functools.lru_cache(maxsize=1)
def _primal_factor(cores_bytes, idx_bytes, shape, lam):
    """(X [P, B], the lower Cholesky factor of X X^T / B + lam I) in extended precision; both objectives share the epoch's
    cores and samples, so it is built once.  Only the blocks on and below the diagonal of the product are formed.  Host cost: np.longdouble
    has no BLAS, and the 0.8e9 extended-precision multiply-adds of the product take about 5 s, the factorisation (one
    vectorised column update per pivot) about 1.5 s: 7 s once per session, no GPU time.  It is what the reference at
    P = 1280 costs in extended precision; the first of the two cases pays it."""
    cores = np.frombuffer(cores_bytes, dtype=np.float64).reshape(shape)
    idx = np.frombuffer(idx_bytes, dtype=np.int64)
    n = shape[0]
    X = fm.score_rows(cores, sm.bits_of_idx(idx, n))["rows"].reshape(-1, idx.size)
    P, Bn = X.shape
    Xt = np.ascontiguousarray(X.T)
    W = np.zeros((P, P), X.dtype)
    step = 128
    for i in range(0, P, step):
        W[i:i + step, :i + step] = X[i:i + step] @ Xt[:, :i + step]
    W = np.tril(W) + np.tril(W, -1).T
    W /= X.dtype.type(Bn)
    W[np.arange(P), np.arange(P)] += X.dtype.type(lam)
    Lc = np.zeros_like(W)
    for j in range(P):
        piv = W[j, j] - Lc[j, :j] @ Lc[j, :j]
        assert piv > 0 and np.isfinite(piv)
        Lc[j, j] = np.sqrt(piv)
        if j + 1 < P:
            Lc[j + 1:, j] = (W[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    return X, Lc


def _primal_delta(X, Lc, w):
    """(X X^T / B + lam I)^-1 X w by the factor (sampled_fisher_mirror.damped_solve's two substitutions)."""
    g = X @ np.asarray(w, dtype=np.float64).astype(X.dtype)
    P = g.size
    y = np.zeros(P, X.dtype)
    for j in range(P):
        y[j] = (g[j] - Lc[j, :j] @ y[:j]) / Lc[j, j]
    x = np.zeros(P, X.dtype)
    for j in range(P - 1, -1, -1):
        x[j] = (y[j] - Lc[j + 1:, j] @ x[j + 1:]) / Lc[j, j]
    return x


@pytest.mark.parametrize("kind", ["elbo", "ksd"])
def test_chain_of_forty(kind):
    """synthetic_network(40, 0), D = 4, B = 1024 with 'sample': P = 1280, the shape blocks='full' refuses.  Epoch 0's delta
    against the mirror's extended-precision primal solve, err <= 1e3 EPS amp with amp = (||T||_inf + lam) / lam from the
    mirror; then 3 epochs: finite losses, status 0, no failed solve, the same bits on a rerun."""
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(40, 0)
    key, lam = TRACE[kind]["key"], 1e-3
    cfg = {'bond_dim': 4, 'num_samples': 1024, 'seed': 9}
    torch.manual_seed(3)
    vi = _trainer(kind)(bn, lat, obs, cfg, device='cuda', natural_gradient='sample')
    vi._prepare_observation(x)
    cores, idx, logq, _ = vi.draw(0)
    _, w = vi.sample_weights(idx, logq)
    delta, info = vi.natural_gradient.precondition_weights(cores, idx, w.contiguous())
    assert info.tolist() == [0] and int(vi.natural_gradient.status.item()) == 0
    cn, idn = cores.detach().cpu().numpy(), idx.cpu().numpy()
    X, Lc = _primal_factor(cn.tobytes(), idn.tobytes(), tuple(cn.shape), lam)
    ref = hp.to_f64(_primal_delta(X, Lc, w.cpu().numpy()))
    X64 = hp.to_f64(X)                                           # the norm of the mirror's T, the rows rounded to float64
    amp = (float(np.abs(X64.T @ X64).sum(axis=1).max()) / X.shape[1] + lam) / lam
    err = np.abs(delta.cpu().numpy().reshape(-1) - ref).max() / np.abs(ref).max()
    print(f"{kind}: relative error of epoch 0's delta at P = {X.shape[0]}: {err:.3e}, bound {1e3 * EPS * amp:.3e} (amp {amp:.3e})")
    assert err <= 1e3 * EPS * amp
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        vi = _trainer(kind)(bn, lat, obs, cfg, device='cuda', natural_gradient='sample')
        hist = vi.train(x, 3, 0.02, verbose=False)
        runs.append((hist, vi.last_idx.cpu().numpy().copy(), vi.born_machine.cores.detach().cpu().numpy().copy(),
                     vi.natural_gradient.info.tolist()))
    (hist, last, cend, info), (hist2, last2, cend2, info2) = runs
    assert all(math.isfinite(v) for v in hist[key] + hist['grad_norm']) and all(s == 0 for s in hist['status'])
    assert hist['natgrad_info'] == [0, 0, 0] and info == [0] == info2
    assert hist[key] == hist2[key] and hist['grad_norm'] == hist2['grad_norm']
    assert np.array_equal(last, last2) and np.array_equal(cend, cend2)
