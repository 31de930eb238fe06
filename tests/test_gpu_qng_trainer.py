"""GPU checks of quantum-natural-gradient training (natural_gradient.QuantumFisherPreconditioner and the two quantum
trainers): the composed Q of real circuits against the float64 mirror (qng_mirror.py), the Loewner bound Q >= F on the
device, the Sprinkler ELBO run against the mirror's recorded trace, the same theta on every gradient route, the untouched
default path, graph replay and the failed solve.

Sprinkler run: the settings of the natural-gradient golden run (natgrad_mirror.SPRINKLER_*) with the quantum metric; loss
rtol 1e-6 and theta atol 2e-6, the floors of test_gpu_elbo_trainer.py and test_gpu_natgrad_trainer.py."""
import numpy as np
import pytest
import torch

import natgrad_mirror as nm
import qng_mirror as qm
import test_gpu_qfi_kernel as qk
from conftest import golden
from oracle import circuit as oc
from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
from test_gpu_natgrad_trainer import SPRINKLER, make_vi, prepare, step

pytestmark = pytest.mark.gpu
LOSS_RTOL, THETA_ATOL = 1e-6, 2e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def device_qfi(ansatz, n, L, theta, dev):
    from tensornetworks_amd.natural_gradient import QuantumFisherPreconditioner
    pre = QuantumFisherPreconditioner().bind(ansatz, n, L)
    return pre.qfi(torch.from_numpy(theta).to(dev)).clone()


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n", [3, 5])
def test_composed_q_is_the_mirrors(dev, ansatz, n):
    """paramshift_states + qfi_gram against the mirror on the oracle's states.  Both sides' states carry at most
    64 eps (gates) per amplitude (test_gpu_paramshift_states.py); an entry of Q is bilinear in unit vectors, so it moves by
    at most 2 sqrt(2^n) of that per factor -- 8 sqrt(2^n) 64 eps gates with the projection term -- plus the Gram bound."""
    L = 2
    theta = np.random.default_rng([n, 31]).standard_normal(oc.num_params(ansatz, n, L))
    Q = device_qfi(ansatz, n, L, theta, dev)
    Qm = qm.qfi_of_circuit(ansatz, n, L, theta)
    tol = 8 * np.sqrt(2.0 ** n) * 64 * 2.0 ** -52 * len(oc.gate_list(ansatz, n, L)) + 4 * (qk.C_TERM + qk.c_chain(n) + 1) * 2.0 ** -52
    err = float(np.abs(Q.cpu().numpy() - Qm).max())
    print(f"{ansatz} n={n}: max |Q - mirror| {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol and torch.equal(Q, Q.t())


@pytest.mark.parametrize("n", [4, 10])
def test_loewner_bound_on_the_device(dev, n):
    """Q - F >= 0 with F = bornvi_fisher_gram of the same circuit (a floor below every q_z)."""
    from tensornetworks_amd import backend
    ansatz, L = "hardware_efficient", 2
    P = oc.num_params(ansatz, n, L)
    theta = np.random.default_rng([n, 37]).standard_normal(P)
    Q = device_qfi(ansatz, n, L, theta, dev).cpu().numpy()
    probs = backend.paramshift_probs(ansatz, n, L, torch.from_numpy(theta).to(dev), 0, P, include_base=True)
    floor = 0.5 * float(probs[0].min())
    assert floor > 0
    F = backend.fisher_gram(probs[1:], probs[0], floor).cpu().numpy()
    lo = np.linalg.eigvalsh(Q - F).min()
    print(f"n={n}: smallest eigenvalue of Q - F {lo:.3e}, |Q| {np.linalg.norm(Q, 2):.3e}")
    assert lo >= -1e-12 * np.linalg.norm(Q, 2)


def sprinkler_train(theta0, natural="quantum", epochs=nm.SPRINKLER_EPOCHS, engine=None, fused=None):
    lat, obs, x = SPRINKLER
    vi = make_vi("elbo", get_sprinkler_network(False), lat, obs, 3, 4, theta0=theta0, natural_gradient=natural)
    if engine is not None:
        vi.grad_engine = engine
    if fused is not None:
        vi.fused_dot = fused
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
    return h


def test_sprinkler_run_follows_the_mirror(dev):
    g = golden("qng_sprinkler_trace.npz")
    h = sprinkler_train(g["theta0"])
    dl = float(np.max(np.abs(np.array(h["loss_elbo"]) / g["loss_elbo"] - 1)))
    dt = float(np.max(np.abs(np.array(h["theta"]) - g["theta"])))
    print(f"quantum natural gradient: kl[0] {h['kl'][0]:.6e} kl[-1] {h['kl'][-1]:.6e}; max rel loss deviation {dl:.3e}; "
          f"max theta deviation {dt:.3e}")
    assert all(v == 0 for v in h["natgrad_info"])
    assert h["kl"][-1] < nm.KL_THRESHOLD and h["kl"][-1] < h["kl"][0]
    np.testing.assert_allclose(h["loss_elbo"], g["loss_elbo"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(np.array(h["theta"]), g["theta"], rtol=0, atol=THETA_ATOL)


@pytest.mark.parametrize("kind", ["ksd", "elbo"])
def test_same_theta_on_every_gradient_route(dev, kind, capsys):
    """Fused dot, stored rows and the adjoint engine under the quantum preconditioner: the same theta after 5 epochs
    (n = 14, L = 1: the first size with the fused dot).  The optimiser is SGD, as in the recorded runs: the first layer's
    RX acts on |+>, so Q and the gradient are exactly zero in those 14 directions, the computed gradient there is
    rounding noise that differs between the routes, delta = noise / damping, and Adam's m / (sqrt(v) + 1e-8) turns
    a delta far below its epsilon into a step of lr / 1e-8 times delta: 5e-6 per epoch from 1e-15 of noise (measured:
    2.4e-5 after 5 epochs between the stored and the fused route).  That gain is Adam's on any preconditioner with a
    null direction, not a difference between the routes; under SGD the same noise moves theta by 1e-13."""
    n, L = 14, 1
    bn, lat, obs, x = synthetic_network(n, 2)
    thetas = {}
    for route in ("fused", "stored", "adjoint"):
        vi = make_vi(kind, bn, lat, obs, n, L, seed=6, natural_gradient="quantum")
        vi.fused_dot = route == "fused"
        if route == "adjoint":
            vi.grad_engine = "adjoint"
        h = vi.train(x, 5, 0.05, verbose=False, optimizer_type="sgd")
        assert all(v == 0 for v in h["natgrad_info"]) and len(h["natgrad_info"]) == 5
        thetas[route] = vi.born_machine.theta.detach().cpu().numpy().copy()
    capsys.readouterr()
    from tensornetworks_amd import backend
    assert backend.paramshift_dot_supported("hardware_efficient", n, L, dev, 3 * n * L)      # "fused" did run fused
    start = make_vi(kind, bn, lat, obs, n, L, seed=6).born_machine.theta.detach().cpu().numpy()
    assert float(np.abs(thetas["fused"] - start).max()) > 1e-3                               # and theta did move
    for route in ("stored", "adjoint"):
        d = float(np.abs(thetas[route] - thetas["fused"]).max())
        print(f"{kind} {route} against fused: max theta deviation {d:.3e}")
        assert d <= THETA_ATOL


@pytest.mark.parametrize("kind", ["ksd", "elbo"])
def test_off_means_bitwise_off(dev, kind, capsys):
    """natural_gradient=None: 5 epochs are bitwise the epochs of a trainer built without the keyword."""
    n, L = 5, 2
    bn, lat, obs, x = synthetic_network(n, 2)
    runs = []
    for kw in ({}, {"natural_gradient": None}):
        vi = make_vi(kind, bn, lat, obs, n, L, seed=4, **kw)
        assert vi.natural_gradient is None and vi._extra_keys == type(vi)._extra_keys
        h = vi.train(x, 5, 0.05, verbose=False)
        runs.append((h, vi.born_machine.theta.detach().cpu().numpy().copy()))
    capsys.readouterr()
    (h0, t0), (h1, t1) = runs
    assert set(h0) == set(h1) and 'natgrad_info' not in h1
    assert np.array_equal(t0, t1)
    for k in h0:
        a, b = (np.array([float(v) for v in h[k]]) for h in (h0, h1))      # (grad_norm: device scalars; tvd: NaN without a posterior)
        assert np.array_equal(a, b, equal_nan=True), k


@pytest.mark.parametrize("kind,n,L", [("elbo", 3, 2), ("ksd", 5, 2)])
def test_graph_replay_equals_eager(dev, kind, n, L, capsys):
    """train(host_sync=False) -- the HIP-graph replay of the step, states, metric and solve included -- against train():
    the tolerances of the natural-gradient trainer test for the same pair."""
    if n == 3:
        bn, (lat, obs, x) = get_sprinkler_network(False), SPRINKLER
    else:
        bn, lat, obs, x = synthetic_network(n, 5)
    runs = []
    for host_sync in (True, False):
        vi = make_vi(kind, bn, lat, obs, n, L, seed=3, natural_gradient="quantum")
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


def test_failed_solve_steps_along_the_plain_gradient(dev):
    """A non-finite gradient: natgrad_info = P + 1 and delta is the gradient, bit for bit (NaN positions included)."""
    from tensornetworks_amd.natural_gradient import QuantumFisherPreconditioner
    ansatz, n, L = "hardware_efficient", 4, 2
    P = oc.num_params(ansatz, n, L)
    pre = QuantumFisherPreconditioner().bind(ansatz, n, L)
    theta = torch.from_numpy(np.random.default_rng(2).standard_normal(P)).to(dev)
    g = torch.from_numpy(np.random.default_rng(3).standard_normal(P)).to(dev)
    delta, info = pre.precondition(theta, g)
    assert int(info) == 0 and not torch.equal(delta, g)
    x_m, info_m, _ = qm.precondition(ansatz, n, L, theta.cpu().numpy(), g.cpu().numpy())
    assert info_m == 0
    np.testing.assert_allclose(delta.cpu().numpy(), x_m, rtol=1e-6, atol=1e-9 * np.abs(x_m).max())
    g[5] = float("inf")
    delta, info = pre.precondition(theta, g)
    assert int(info) == P + 1 and torch.equal(delta, g)
    g[5] = float("nan")
    delta, info = pre.precondition(theta, g)
    assert int(info) == P + 1
    assert torch.equal(torch.isnan(delta), torch.isnan(g)) and torch.equal(delta[~torch.isnan(g)], g[~torch.isnan(g)])
