"""GPU parity of the three MMD trainers (mmd_quantum.py, mmd_classical.py, mmd_sampled.py) with the mirror (tests/mmd_mirror.py):
the quantum step and its three gradient routes, a 20-epoch Adam trace and its deferred / graph-replayed run, the classical
families against torch autograd through the dense kernel matrix, the sampled estimator on the epoch's own draws, and the
refusals.  The tolerances are those of tests/test_gpu_elbo_trainer.py and tests/test_gpu_mps_trainer.py for the same
comparisons."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import mmd_mirror as mm
import mps_mirror as mpm
from oracle import circuit as oc
from tensornetworks_amd import backend
from tensornetworks_amd.hamming_kernel import HammingMixtureKernel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALES = (0.25, 1.0, 4.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def data_indices(n, N, seed):
    return torch.from_numpy(np.random.default_rng([seed, n]).integers(0, 1 << n, N))


def make_quantum(n, L, ansatz="hardware_efficient", seed=0, theta0=None):
    from tensornetworks_amd import QuantumMMDTrainer
    torch.manual_seed(seed)
    vi = QuantumMMDTrainer(n, L, ansatz, pytorch_device=DEV, length_scales=SCALES)
    if theta0 is not None:
        with torch.no_grad():
            vi.born_machine.theta.copy_(torch.as_tensor(theta0).to(vi.born_machine.theta.device))
    return vi


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


# ---- quantum ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ansatz,n,L", [("hardware_efficient", 5, 2), ("basic", 4, 2), ("all_to_all", 8, 1)])
def test_step_matches_the_mirror(dev, ansatz, n, L):
    vi = make_quantum(n, L, ansatz, seed=3)
    data = data_indices(n, 50, 1)
    vi.objective.prepare(data)
    target = np.bincount(data.numpy(), minlength=1 << n) / 50.0
    assert np.array_equal(vi.objective.target.cpu().numpy(), target)
    loss, grad, q = vi.loss_and_grad()
    th = vi.born_machine.theta.detach().double().cpu().numpy()
    loss_m, g_m, q_m, w_m = mm.loss_and_grad(ansatz, n, L, th, target, vi.objective.kernel.spectrum)
    np.testing.assert_allclose(q.cpu().numpy(), q_m, rtol=1e-10, atol=1e-14)
    assert math.isclose(loss.item(), loss_m, rel_tol=1e-10), (loss.item(), loss_m)
    np.testing.assert_allclose(grad.cpu().numpy(), g_m, rtol=1e-7, atol=1e-9 * np.abs(g_m).max())
    assert loss.item() > 0


def test_fused_stored_and_adjoint_routes_agree(dev):
    """(hardware_efficient, n = 14, L = 2): the first size with the fused dot.  Fused against stored probabilities to 1e-12 of
    the largest entry, the adjoint engine to the ELBO trainer test's tolerance."""
    ansatz, n, L = "hardware_efficient", 14, 2
    vi = make_quantum(n, L, ansatz, seed=4)
    vi.objective.prepare(data_indices(n, 200, 2))
    P = vi.born_machine.num_ansatz_params
    assert backend.paramshift_dot_supported(ansatz, n, L, dev, P)
    out = {}
    for route in ("fused", "stored", "adjoint"):
        vi.fused_dot = route == "fused"
        vi.grad_engine = "adjoint" if route == "adjoint" else "paramshift"
        loss, grad, q = vi.loss_and_grad()
        out[route] = (loss.clone(), grad.clone(), q.clone())
    g_s = out["stored"][1]
    gmax = float(g_s.abs().max())
    assert gmax > 0 and abs(float(out["stored"][2].sum()) - 1) < 1e-12
    assert torch.equal(out["fused"][2], out["stored"][2]) and torch.equal(out["fused"][0], out["stored"][0])
    assert float((out["fused"][1] - g_s).abs().max()) <= 1e-12 * gmax
    np.testing.assert_allclose(out["adjoint"][2].cpu().numpy(), out["stored"][2].cpu().numpy(), rtol=1e-10, atol=1e-15)
    assert math.isclose(float(out["adjoint"][0]), float(out["stored"][0]), rel_tol=1e-10)
    np.testing.assert_allclose(out["adjoint"][1].cpu().numpy(), g_s.cpu().numpy(), rtol=1e-8, atol=1e-10 * gmax)


@pytest.fixture(scope="module")
def trace_case():
    """n = 4: the target is the circuit's own q at another theta, so the minimum 0 is reachable; the mirror's 20 epochs, once."""
    ansatz, n, L = "hardware_efficient", 4, 2
    P = oc.num_params(ansatz, n, L)
    rng = np.random.default_rng(5)
    target = oc.probs(ansatz, n, L, 0.8 * rng.standard_normal(P))
    th0 = (0.1 * rng.standard_normal(P)).astype(np.float32)
    lam = HammingMixtureKernel(n, SCALES).spectrum
    return ansatz, n, L, target, th0, mm.train(ansatz, n, L, target, lam, th0, 0.05, 20)


def test_adam_trace_follows_the_mirror(dev, trace_case):
    ansatz, n, L, target, th0, ref = trace_case
    vi = make_quantum(n, L, ansatz, theta0=th0)
    hist = quiet(vi.train, torch.from_numpy(target), 20, 0.05, verbose=True)
    assert set(hist) == {'loss_mmd2', 'tvd', 'grad_norm'} and all(len(v) == 20 for v in hist.values())
    print(f"loss {hist['loss_mmd2'][0]:.6e} -> {hist['loss_mmd2'][-1]:.6e}; max rel loss err "
          f"{np.max(np.abs(np.array(hist['loss_mmd2']) / ref['loss_mmd2'] - 1)):.3e}; max theta err "
          f"{np.max(np.abs(vi.born_machine.theta.detach().cpu().numpy() - ref['theta'][-1])):.3e}")
    np.testing.assert_allclose(hist['loss_mmd2'], ref["loss_mmd2"], rtol=1e-6)
    np.testing.assert_allclose(vi.born_machine.theta.detach().cpu().numpy(), ref["theta"][-1], rtol=0, atol=2e-6)
    np.testing.assert_allclose([float(v) for v in hist['grad_norm']], ref["grad_norm"], rtol=1e-5)
    assert hist['loss_mmd2'][-1] < hist['loss_mmd2'][0] and min(hist['loss_mmd2']) >= 0.0
    assert all(np.isnan(hist['tvd']))


def test_deferred_run_gives_the_eager_history(dev, trace_case):
    """train(host_sync=False): at n = 4 without a TVD the epochs are one HIP graph's replays."""
    ansatz, n, L, target, th0, _ = trace_case
    runs = []
    for host_sync in (True, False):
        vi = make_quantum(n, L, ansatz, theta0=th0)
        h = quiet(vi.train, torch.from_numpy(target), 20, 0.05, verbose=True, host_sync=host_sync)
        runs.append((h, vi.born_machine.theta.detach().cpu().numpy().copy()))
    (h0, t0), (h1, t1) = runs
    assert set(h1) == set(h0) == {'loss_mmd2', 'tvd', 'grad_norm'} and all(len(v) == 20 for v in h1.values())
    np.testing.assert_allclose(h1["loss_mmd2"], h0["loss_mmd2"], rtol=2e-5)
    np.testing.assert_allclose(h1["grad_norm"], [float(v) for v in h0["grad_norm"]], rtol=2e-4)
    np.testing.assert_allclose(t1, t0, rtol=0, atol=2e-5)
    assert h1["loss_mmd2"][-1] < h1["loss_mmd2"][0]


# ---- classical -------------------------------------------------------------------------------------------------------------
def dense_loss(q, target, K):
    d = q - target
    return d @ (K @ d)


@pytest.mark.parametrize("use_logits", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.013])
def test_classical_table_step_against_autograd(dev, use_logits, lam):
    from tensornetworks_amd import ClassicalMMDTrainer
    n = 4
    torch.manual_seed(7)
    vi = ClassicalMMDTrainer(n, {"use_logits": use_logits}, device=DEV, length_scales=SCALES)
    with torch.no_grad():
        vi.born_machine.params.mul_(20.0)              # (small_random is 0.1 N(0, 1): nearly uniform q otherwise)
    vi.objective.prepare(data_indices(n, 50, 3))
    loss, ent, q, grads = vi.loss_and_grads(None, lam)
    assert len(grads) == 1 and grads[0][0] is vi.born_machine.params
    g = grads[0][1]
    K = vi.objective.kernel.dense()
    w64 = vi.born_machine.params.detach().double().cpu().requires_grad_(True)
    qr = torch.softmax(w64, dim=-1) if use_logits else w64.abs() / w64.abs().sum()
    loss_r = dense_loss(qr, vi.objective.target.cpu(), K)
    H_r = -(qr * torch.log(qr.clamp(min=1e-10))).sum()
    (loss_r - lam * H_r).backward()
    torch.testing.assert_close(loss.cpu()[0], loss_r.detach(), rtol=2e-6, atol=1e-6)
    torch.testing.assert_close(ent.cpu().double().reshape(-1)[0], H_r.detach(), rtol=2e-6, atol=1e-6)
    assert g.dtype == torch.float32 and g.shape == vi.born_machine.params.shape
    assert float(((g.double().cpu() - w64.grad).abs() / w64.grad.abs().max()).max()) < 1e-5


def test_classical_mlp_step_reaches_the_network(dev):
    from tensornetworks_amd import ClassicalMMDTrainer
    n = 4
    torch.manual_seed(2)
    vi = ClassicalMMDTrainer(n, {"use_logits": True, "conditioning_dim": 1}, device=DEV, length_scales=SCALES, condition=[1.0])
    vi.born_machine.eval()                             # (no Dropout draws: the two forwards below see the same network)
    vi.objective.prepare(data_indices(n, 50, 4))
    xc = torch.tensor([1.0], device=DEV)
    loss, ent, q, grads = vi.loss_and_grads(xc, 0.0)
    vi.apply_grads(grads)
    got = [p.grad.detach().double().cpu().clone() for p in vi.born_machine.parameters()]
    for p in vi.born_machine.parameters():
        p.grad = None
    qr = torch.softmax(vi.born_machine.raw_params(xc).double(), dim=-1).reshape(-1)
    ref = dense_loss(qr, vi.objective.target, vi.objective.kernel.dense(DEV))
    ref.backward()
    torch.testing.assert_close(loss[0], ref.detach(), rtol=2e-6, atol=1e-6)
    for a, p in zip(got, vi.born_machine.parameters()):
        scale = float(p.grad.abs().max())
        assert float((a - p.grad.double().cpu()).abs().max()) <= 1e-4 * scale + 1e-7


def test_classical_mps_step_against_autograd(dev):
    from tensornetworks_amd import ClassicalMMDTrainer
    n, D = 4, 2
    torch.manual_seed(11)
    vi = ClassicalMMDTrainer(n, {'family': 'mps', 'bond_dim': D}, device=DEV, length_scales=SCALES)
    vi.objective.prepare(data_indices(n, 50, 5))
    loss, ent, q, grads = vi.loss_and_grads(None, 0.0)
    assert grads[0][0] is vi.born_machine.cores and grads[0][1].dtype == torch.float64
    cores = vi.born_machine.cores.detach().cpu().clone().requires_grad_(True)
    ref = dense_loss(mpm._q_of(cores), vi.objective.target.cpu(), vi.objective.kernel.dense())
    ref.backward()
    np.testing.assert_allclose(loss.cpu().numpy()[0], float(ref.detach()), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(grads[0][1].cpu().numpy(), cores.grad.numpy(), rtol=1e-10, atol=1e-10)


def test_classical_train_improves(dev):
    from tensornetworks_amd import ClassicalMMDTrainer
    n = 4
    data = data_indices(n, 50, 6)
    target = torch.bincount(data, minlength=1 << n).double() / 50.0
    for cfg in ({"use_logits": True}, {'family': 'mps', 'bond_dim': 2}):
        torch.manual_seed(0)
        vi = ClassicalMMDTrainer(n, cfg, device=DEV, length_scales=SCALES)
        hist = quiet(vi.train, data, 60, 0.05, verbose=True, target_for_tvd=target.to(DEV))
        assert set(hist) == {'loss_mmd2', 'tvd', 'grad_norm', 'entropy'}
        assert hist['loss_mmd2'][-1] < hist['loss_mmd2'][0] and hist['tvd'][-1] < hist['tvd'][0] and min(hist['loss_mmd2']) >= 0.0


# ---- sampled ---------------------------------------------------------------------------------------------------------------
def make_sampled(cores, natural_gradient=None, seed=9):
    from tensornetworks_amd import SampledMMDTrainer
    torch.manual_seed(seed)
    return SampledMMDTrainer(6, {'bond_dim': 2, 'num_samples': 64, 'seed': 17, 'cores': cores}, device=DEV, length_scales=SCALES,
                             natural_gradient=natural_gradient)


@pytest.mark.parametrize("cores", ["real", "complex"])
def test_sampled_epoch_matches_the_mirror(dev, cores):
    """U to 1e-13 of itself; w_b to 1e-13 of the largest entry (a w_b is a difference of terms near 1 / B: an entry close to 0
    carries the rounding of those terms, so the scale of the comparison is the vector's, not the entry's)."""
    n, B, N = 6, 64, 50
    data = data_indices(n, N, 7)
    vi = make_sampled(cores)
    vi._prepare_observation(data)
    U, grad, lq, st = vi.loss_and_grad(0)
    idx = vi.last_idx
    assert idx.shape == (B,) and int(st.item()) == 0 and bool(torch.isfinite(grad).all())
    U2, w = vi.objective.sample_weights(idx)
    assert torch.equal(U2, U)
    U_m, w_m, rxx, rxy, Tyy = mm.sampled(idx.cpu().numpy(), data.numpy(), n, vi.objective.kernel.kappa)
    assert abs(vi.objective.Tyy.item() - Tyy) <= 1e-13 * Tyy
    print(f"{cores}: U {U.item():.6e} (mirror {U_m:.6e}, rel {abs(U.item() - U_m) / abs(U_m):.2e}); w worst "
          f"{np.abs(w.cpu().numpy() - w_m).max() / np.abs(w_m).max():.2e} of its largest entry")
    assert abs(U.item() - U_m) <= 1e-13 * abs(U_m)
    np.testing.assert_allclose(w.cpu().numpy(), w_m, rtol=0, atol=1e-13 * np.abs(w_m).max())
    assert abs(float(w.sum())) <= 1e-13 * float(w.abs().sum())


@pytest.mark.parametrize("cores", ["real", "complex"])
def test_sampled_train_and_the_exact_check(dev, cores):
    n, N = 6, 50
    data = data_indices(n, N, 8)
    target = torch.bincount(data, minlength=1 << n).double() / N
    vi = make_sampled(cores)
    hist = quiet(vi.train, data, 3, 0.05, verbose=True, target_for_tvd=target)
    assert set(hist) == {'loss_mmd2', 'grad_norm', 'logq_mean', 'status', 'tvd', 'kl', 'mmd2_exact'}
    assert all(len(v) == 3 for v in hist.values()) and all(np.isfinite(v).all() for v in hist.values())
    q = vi.born_machine.probabilities64().detach().contiguous()
    want = backend.mmd_weights(q, vi.objective.target, vi.objective.kernel.spectrum_on(q.device), want_w=False)[0]
    assert hist['mmd2_exact'][-1] == want.item()            # bit for bit: the check between the two kernels


def test_sampled_natural_gradient_starts_from_the_same_samples(dev):
    data = data_indices(6, 50, 9)
    plain = quiet(make_sampled("real").train, data, 3, 0.05, verbose=False)
    nat = quiet(make_sampled("real", natural_gradient='site').train, data, 3, 0.05, verbose=False)
    assert nat['loss_mmd2'][0] == plain['loss_mmd2'][0]
    assert 'natgrad_info' in nat and all(np.isfinite(v).all() for v in nat.values())


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from tensornetworks_amd import ClassicalMMDTrainer, QuantumMMDTrainer, SampledMMDTrainer
    with pytest.raises(ValueError):
        QuantumMMDTrainer(4, 1, pytorch_device=DEV, qbm_shots=100)
    with pytest.raises(ValueError):
        QuantumMMDTrainer(4, 1, pytorch_device=DEV, natural_gradient=True)
    with pytest.raises(ValueError):
        SampledMMDTrainer(6, {'bond_dim': 2, 'num_samples': 2}, device=DEV)
    vi = make_quantum(4, 1)
    theta_before = vi.born_machine.theta.detach().clone()
    sv = make_sampled("real")
    cv = ClassicalMMDTrainer(4, {}, device=DEV)
    for trainer in (vi, sv, cv):
        n = 6 if trainer is sv else 4
        for bad in (torch.zeros(0, dtype=torch.int64), torch.tensor([1 << n]), torch.tensor([-1]), torch.full((3, n), 2)):
            with pytest.raises(ValueError):
                trainer.train(bad, 2, 0.05, verbose=False)
    assert torch.equal(vi.born_machine.theta.detach(), theta_before)
    with pytest.raises(ValueError):
        sv.train(torch.full((64,), 1.0 / 64, dtype=torch.float64), 2, 0.05, verbose=False)      # a table has no data points
    with pytest.raises(ValueError):
        vi.loss_and_grad()                                                                        # before prepare
