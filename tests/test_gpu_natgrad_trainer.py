"""GPU checks of natural-gradient training (natural_gradient.py and the two quantum trainers): the Fisher matrix of real
circuits and the preconditioned step against the float64 mirror (natgrad_mirror.py), the Sprinkler ELBO run against the
mirror's recorded trace, the read-back modes, and the untouched default path.

Sprinkler run (hardware_efficient, n = 3, L = 4, damping 1e-3, SGD without momentum, lr 0.3, 40 epochs, theta0 handed to
both sides): float32 theta rounding flips are amplified by the solve, so the tolerance is 10 x the deviation measured once
on an MI355X, never tighter than test_gpu_elbo_trainer.py's (loss rtol 1e-6, theta atol 2e-6).  Measured: largest relative
loss deviation 5.1e-15, largest theta deviation 0 (every float32 theta of the 40 epochs equal to the mirror's), so the
floors are the tolerances in force."""
import numpy as np
import pytest
import torch

import elbo_mirror as em
import natgrad_mirror as nm
import test_gpu_fisher_kernel as fk
import test_gpu_spd_solve as sk
from conftest import golden
from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network

pytestmark = pytest.mark.gpu

SPRINKLER = (['C', 'S', 'R'], ['W'], {'W': 1})
MEASURED_LOSS, MEASURED_THETA = 5.2e-15, 0.0             # measured deviations of the Sprinkler run (see the docstring)
LOSS_RTOL = max(1e-6, 10 * MEASURED_LOSS)
THETA_ATOL = max(2e-6, 10 * MEASURED_THETA)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def make_vi(kind, bn, lat, obs, n, L, seed=0, theta0=None, **kw):
    from tensornetworks_amd.elbo_vi_quantum import ELBOVariationalInference
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    torch.manual_seed(seed)
    cls = {"ksd": KSDVariationalInference, "elbo": ELBOVariationalInference}[kind]
    vi = cls(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, pytorch_device="cuda:0", **kw)
    if theta0 is not None:
        with torch.no_grad():
            vi.born_machine.theta.copy_(torch.as_tensor(theta0).to(vi.born_machine.theta.device))
    return vi


def prepare(vi, kind, x):
    if kind == "ksd":
        vi._prepare_stein(x)
    else:
        vi.objective.prepare(x)
    return vi


def step(vi, kind):
    return vi.ksd_and_grad() if kind == "ksd" else vi.elbo_and_grad()


@pytest.mark.parametrize("n", [3, 10])
def test_fisher_of_real_circuits_is_the_mirror(dev, n):
    """hardware_efficient, L = 2: FisherPreconditioner.fisher on backend.paramshift_probs rows against the mirror on the same
    rows; both sit within the Gram bound of the exact matrix, so they differ by at most twice that bound."""
    from tensornetworks_amd import backend
    from tensornetworks_amd.natural_gradient import FisherPreconditioner
    ansatz, L = "hardware_efficient", 2
    P = backend.num_params(ansatz, n, L)
    theta = torch.from_numpy(np.random.default_rng(n).standard_normal(P)).to(dev)
    probs = backend.paramshift_probs(ansatz, n, L, theta, 0, P, include_base=True)
    q, rows = probs[0], probs[1:]
    F = FisherPreconditioner().fisher(rows, q)
    rows_h, q_h = rows.cpu().numpy(), q.cpu().numpy()
    F_m = nm.fisher(rows_h, q_h)
    d = np.abs(0.5 * (rows_h[0::2] - rows_h[1::2]))
    r = np.where(q_h >= nm.Q_FLOOR, 1.0 / np.maximum(q_h, nm.Q_FLOOR), 0.0)
    bound = 2 * (fk.C_TERM + fk.c_chain(n)) * 2.0 ** -52 * ((d * r) @ d.T)
    err = np.abs(F.cpu().numpy() - F_m)
    print(f"n={n} P={P}: worst |F - mirror| / (2 x bound) {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all() and torch.equal(F, F.t())
    # the rows of the oracle's circuits give the same matrix to circuit accuracy
    if n == 3:
        F_o = nm.fisher(nm.shifted_rows(ansatz, n, L, theta.cpu().numpy()), q_h)
        np.testing.assert_allclose(F.cpu().numpy(), F_o, rtol=0, atol=1e-10 * np.abs(F_o).max())


@pytest.mark.parametrize("kind", ["ksd", "elbo"])
def test_preconditioned_step_is_the_mirrors_solve(dev, kind):
    """One step with natural_gradient=True: delta solves (F + damping I) delta = g for the F and the g of that step, within
    the solve's residual bound, and equals the mirror's solve of the same F and g to the condition number times that
    bound; loss and q are the plain step's bits."""
    n, L = 5, 2
    bn, lat, obs, x = synthetic_network(n, 0)
    nat = prepare(make_vi(kind, bn, lat, obs, n, L, seed=3, natural_gradient=True), kind, x)
    plain = prepare(make_vi(kind, bn, lat, obs, n, L, seed=3), kind, x)
    plain.fused_dot = False
    loss, delta, q = step(nat, kind)
    loss_p, g, q_p = step(plain, kind)
    assert torch.equal(loss, loss_p) and torch.equal(q, q_p) and int(nat._natgrad_info) == 0
    F = nat.natural_gradient._F.cpu().numpy()
    lam = nat.natural_gradient.damping
    g_h, d_h = g.cpu().numpy(), delta.cpu().numpy()
    ratio = sk.residual_ratio(F, lam, d_h, g_h)
    x_m, info_m = nm.spd_solve(F, g_h, lam)
    P = g_h.size
    gamma = (3 * P + 1) * sk.U / (1 - (3 * P + 1) * sk.U)
    M = F + lam * np.eye(P)
    fwd = 2 * gamma * P * np.linalg.cond(M) * np.linalg.norm(M) / np.linalg.norm(M, 2) * np.linalg.norm(x_m)
    print(f"{kind}: residual / bound {ratio:.3e}; |delta - mirror| {np.linalg.norm(d_h - x_m):.3e} <= {fwd:.3e}; "
          f"|delta| / |g| {np.linalg.norm(d_h) / np.linalg.norm(g_h):.3f}")
    assert info_m == 0 and ratio <= 1.0 and np.linalg.norm(d_h - x_m) <= fwd
    assert not np.allclose(d_h, g_h)


def sprinkler_train(natural, theta0, epochs=nm.SPRINKLER_EPOCHS):
    """The recorded run's epochs on the device: training_step with plain SGD (no momentum, constant rate)."""
    lat, obs, x = SPRINKLER
    vi = make_vi("elbo", get_sprinkler_network(False), lat, obs, 3, 4, theta0=theta0,
                 natural_gradient=nm.DAMPING if natural else None)
    vi.objective.prepare(x)
    params = list(vi.born_machine.parameters())
    opt = torch.optim.SGD(params, lr=nm.SPRINKLER_LR, momentum=0.0)
    h = {"loss_elbo": [], "natgrad_info": [], "theta": []}
    for _ in range(epochs):
        loss, _, _ = vi.training_step(params, opt, None, 10.0)
        h["loss_elbo"].append(loss)
        h["natgrad_info"].append(int(vi._natgrad_info) if natural else 0)
        h["theta"].append(vi.born_machine.theta.detach().cpu().numpy().copy())
    h["kl"] = [v + vi.objective.log_evidence for v in h["loss_elbo"]]
    q = vi.born_machine.get_probabilities().detach().double().cpu().numpy().reshape(-1)
    log_p, log_ev = em.log_joint(get_sprinkler_network(False), lat, x)
    h["tvd"] = 0.5 * float(np.abs(q - np.exp(log_p - log_ev)).sum())
    return h


def test_sprinkler_run_follows_the_mirror(dev):
    g = golden("natgrad_sprinkler_trace.npz")
    h = sprinkler_train(True, g["theta0"])
    sgd = sprinkler_train(False, g["theta0"])
    dl = float(np.max(np.abs(np.array(h["loss_elbo"]) / g["loss_elbo"] - 1)))
    dt = float(np.max(np.abs(np.array(h["theta"]) - g["theta"])))
    print(f"natural gradient: kl[0] {h['kl'][0]:.6e} kl[-1] {h['kl'][-1]:.6e} tvd {h['tvd']:.3e}; max rel loss deviation "
          f"{dl:.3e}; max theta deviation {dt:.3e}; plain SGD, same rate and epochs: kl[-1] {sgd['kl'][-1]:.6e} "
          f"tvd {sgd['tvd']:.3e}")
    assert all(v == 0 for v in h["natgrad_info"])
    assert h["kl"][-1] < nm.KL_THRESHOLD and h["kl"][-1] < h["kl"][0]
    np.testing.assert_allclose(h["loss_elbo"], g["loss_elbo"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(np.array(h["theta"]), g["theta"], rtol=0, atol=THETA_ATOL)


@pytest.mark.parametrize("kind,n,L", [("elbo", 3, 2), ("elbo", 8, 2), ("ksd", 5, 2)])
def test_read_back_modes_give_the_same_history(dev, kind, n, L, capsys):
    """train(host_sync=False) -- the HIP-graph replay of the step, Fisher matrix and solve included -- against train():
    the tolerances of the existing trainer tests for the same pair."""
    if n == 3:
        bn, (lat, obs, x) = get_sprinkler_network(False), SPRINKLER
    else:
        bn, lat, obs, x = synthetic_network(n, 5)
    runs = []
    for host_sync in (True, False):
        vi = make_vi(kind, bn, lat, obs, n, L, seed=3, natural_gradient=True)
        h = vi.train(x, 12, 0.05, verbose=False, host_sync=host_sync)
        runs.append((h, vi.born_machine.theta.detach().cpu().numpy().copy()))
    capsys.readouterr()
    (h0, t0), (h1, t1) = runs
    key = 'loss_elbo' if kind == "elbo" else 'loss_ksd'
    assert set(h1) == set(h0) and 'natgrad_info' in h0 and all(len(v) == 12 for v in h1.values())
    assert all(v == 0 for v in h0['natgrad_info']) and all(v == 0 for v in h1['natgrad_info'])
    np.testing.assert_allclose(h1[key], h0[key], rtol=2e-5)
    np.testing.assert_allclose(h1["grad_norm"], [float(v) for v in h0["grad_norm"]], rtol=2e-4)
    np.testing.assert_allclose(t1, t0, rtol=0, atol=2e-5)


@pytest.mark.parametrize("kind", ["ksd", "elbo"])
def test_default_path_is_untouched(dev, kind):
    """natural_gradient=None: one step is bitwise the step of a trainer constructed without the keyword, on the fused and
    on the stored route (n = 14: the first size with the fused dot)."""
    for n, L in ((5, 2), (14, 2)):
        bn, lat, obs, x = synthetic_network(n, 2)
        a = prepare(make_vi(kind, bn, lat, obs, n, L, seed=4), kind, x)
        b = prepare(make_vi(kind, bn, lat, obs, n, L, seed=4, natural_gradient=None), kind, x)
        assert b.natural_gradient is None and b._extra_keys == type(b)._extra_keys
        for fused in (True, False):
            a.fused_dot = b.fused_dot = fused
            ra, rb = step(a, kind), step(b, kind)
            assert all(torch.equal(u, v) for u, v in zip(ra, rb))
            assert len(b._step_extras()) == len(a._step_extras()) == (1 if kind == "elbo" else 0)
