"""GPU parity of the two ELBO trainers (elbo_vi_quantum.py, elbo_vi.py): one step against the float64 mirror
(elbo_mirror.py), the three gradient routes against each other, the strided deal, train() against the mirror's recorded
Sprinkler run, the read-back modes, the skipped step, and the classical family against torch autograd."""
import math

import numpy as np
import pytest
import torch

import elbo_mirror as em
from conftest import golden
from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network

pytestmark = pytest.mark.gpu

SPRINKLER = (['C', 'S', 'R'], ['W'], {'W': 1})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def make_vi(bn, lat, obs, n, L, ansatz="hardware_efficient", seed=0, theta0=None, **kw):
    from tensornetworks_amd.elbo_vi_quantum import ELBOVariationalInference
    torch.manual_seed(seed)
    vi = ELBOVariationalInference(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, qbm_ansatz_type=ansatz,
                                  pytorch_device="cuda:0", **kw)
    if theta0 is not None:
        with torch.no_grad():
            vi.born_machine.theta.copy_(torch.as_tensor(theta0).to(vi.born_machine.theta.device))
    return vi


@pytest.mark.parametrize("ansatz,n,L", [("hardware_efficient", 5, 2), ("basic", 4, 2), ("all_to_all", 8, 1)])
def test_step_matches_the_mirror(dev, ansatz, n, L):
    bn, lat, obs, x = synthetic_network(n, 0)
    vi = make_vi(bn, lat, obs, n, L, ansatz, seed=3)
    vi.objective.prepare(x)
    log_p, log_ev = em.log_joint(bn, lat, x)
    np.testing.assert_allclose(vi.objective.log_p.cpu().numpy(), log_p, rtol=1e-13)
    assert math.isclose(vi.objective.log_evidence, log_ev, rel_tol=1e-13)
    loss, grad, q = vi.elbo_and_grad()
    th = vi.born_machine.theta.detach().double().cpu().numpy()
    loss_m, ent_m, g_m, q_m = em.loss_and_grad(ansatz, n, L, th, log_p)
    np.testing.assert_allclose(q.cpu().numpy(), q_m, rtol=1e-10, atol=1e-14)
    assert math.isclose(loss.item(), loss_m, rel_tol=1e-10), (loss.item(), loss_m)
    assert math.isclose(float(vi._entropy), ent_m, rel_tol=1e-10)
    np.testing.assert_allclose(grad.cpu().numpy(), g_m, rtol=1e-7, atol=1e-9 * np.abs(g_m).max())
    assert loss.item() + log_ev >= -1e-12


def test_fused_stored_and_adjoint_routes_agree_and_the_deal_is_exact(dev):
    """(hardware_efficient, n = 14, L = 2): the first size with the fused dot.  Fused against stored probabilities to
    1e-12 of the largest entry, the adjoint engine to the KSD trainer test's tolerance; the two ranks of a strided deal
    (0, P, 2) and (1, P, 2), interleaved, are the full gradient -- bitwise on the stored path."""
    from tensornetworks_amd import backend
    ansatz, n, L = "hardware_efficient", 14, 2
    bn, lat, obs, x = synthetic_network(n, 2)
    vi = make_vi(bn, lat, obs, n, L, ansatz, seed=4)
    vi.objective.prepare(x)
    P = vi.born_machine.num_ansatz_params
    assert backend.paramshift_dot_supported(ansatz, n, L, dev, P) and backend.paramshift_dot_supported(ansatz, n, L, dev, P // 2)
    theta64 = vi.born_machine.theta.detach().double().contiguous()
    out = {}
    for route in ("fused", "stored", "adjoint"):
        vi.fused_dot = route == "fused"
        vi.grad_engine = "adjoint" if route == "adjoint" else "paramshift"
        loss, grad, q = vi.elbo_and_grad()
        out[route] = (loss.clone(), grad.clone(), q.clone())
        if route != "adjoint":
            halves = [vi.elbo_and_grad_local(theta64, r, P, 2) for r in (0, 1)]
            deal = torch.empty(P, dtype=torch.float64, device=dev)
            deal[0::2], deal[1::2] = halves[0][1], halves[1][1]
            assert all(torch.equal(h[0], loss) and torch.equal(h[2], q) for h in halves)
            out[route + "-deal"] = deal
    g_s = out["stored"][1]
    gmax = float(g_s.abs().max())
    assert gmax > 0 and abs(float(out["stored"][2].sum()) - 1) < 1e-12
    assert torch.equal(out["fused"][2], out["stored"][2]) and torch.equal(out["fused"][0], out["stored"][0])
    assert float((out["fused"][1] - g_s).abs().max()) <= 1e-12 * gmax
    assert torch.equal(out["stored-deal"], g_s)
    assert float((out["fused-deal"] - out["fused"][1]).abs().max()) <= 1e-12 * gmax
    np.testing.assert_allclose(out["adjoint"][2].cpu().numpy(), out["stored"][2].cpu().numpy(), rtol=1e-10, atol=1e-15)
    assert math.isclose(float(out["adjoint"][0]), float(out["stored"][0]), rel_tol=1e-10)
    np.testing.assert_allclose(out["adjoint"][1].cpu().numpy(), g_s.cpu().numpy(), rtol=1e-8, atol=1e-10 * gmax)
    with pytest.raises(ValueError):
        vi.grad_engine = "finite-difference"
        vi.elbo_and_grad()


def test_sprinkler_train_follows_the_mirror(dev, capsys):
    """200 epochs, lr 0.05, theta0 handed to both sides: the history of the mirror's recorded run
    (tests/golden/elbo_sprinkler_trace.npz; test_elbo_host.py pins it to the mirror) and KL < 1e-6 at the end."""
    g = golden("elbo_sprinkler_trace.npz")
    lat, obs, x = SPRINKLER
    vi = make_vi(get_sprinkler_network(False), lat, obs, 3, 4, theta0=g["theta0"])
    hist = vi.train(x, 200, 0.05, verbose=True)
    out = capsys.readouterr().out
    assert "Precomputing log p(x,z)..." in out and "Epoch 1/200 | ELBO:" in out and "| LR:" in out and "KSD" not in out
    assert set(hist) == {'loss_elbo', 'kl', 'entropy', 'tvd', 'grad_norm'} and all(len(v) == 200 for v in hist.values())
    print(f"kl[0] {hist['kl'][0]:.6e} kl[-1] {hist['kl'][-1]:.6e}  max rel loss err "
          f"{np.max(np.abs(np.array(hist['loss_elbo']) / g['loss_elbo'] - 1)):.3e}  max theta err "
          f"{np.max(np.abs(vi.born_machine.theta.detach().cpu().numpy() - g['theta_final'])):.3e}")
    np.testing.assert_allclose(hist['loss_elbo'], g["loss_elbo"], rtol=1e-6)
    np.testing.assert_allclose(vi.born_machine.theta.detach().cpu().numpy(), g["theta_final"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(hist['entropy'], g["entropy"], rtol=1e-5)
    assert hist['kl'][-1] < 1e-6 and hist['kl'][-1] < hist['kl'][0]
    assert all(np.isnan(hist['tvd']))


@pytest.mark.parametrize("n,L,with_tvd", [(3, 2, True), (8, 2, False)])
def test_read_back_modes_give_the_same_history(dev, n, L, with_tvd, capsys):
    """train(host_sync=False) -- the asynchronous step, or without a per-epoch TVD its HIP-graph replay -- against
    train(): the KSD trainer test's tolerances for the same comparison."""
    from tensornetworks_amd import stein_utils
    if n == 3:
        bn, (lat, obs, x) = get_sprinkler_network(False), SPRINKLER
    else:
        bn, lat, obs, x = synthetic_network(n, 5)
    runs = []
    for host_sync in (True, False):
        vi = make_vi(bn, lat, obs, n, L, seed=3)
        post = stein_utils.true_posterior_table(bn, x, lat, dev)[0] if with_tvd else None
        h = vi.train(x, 12, 0.05, verbose=True, true_posterior_for_tvd=post, host_sync=host_sync)
        log = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch ")]
        runs.append((h, vi.born_machine.theta.detach().cpu().numpy().copy(), log))
    (h0, t0, log0), (h1, t1, log1) = runs
    assert set(h1) == set(h0) == {'loss_elbo', 'kl', 'entropy', 'tvd', 'grad_norm'} and all(len(v) == 12 for v in h1.values())
    np.testing.assert_allclose(h1["loss_elbo"], h0["loss_elbo"], rtol=2e-5)
    np.testing.assert_allclose(h1["kl"], h0["kl"], rtol=2e-5, atol=2e-5 * abs(h0["loss_elbo"][0]))
    np.testing.assert_allclose(h1["entropy"], h0["entropy"], rtol=2e-5)
    np.testing.assert_allclose(h1["grad_norm"], [float(v) for v in h0["grad_norm"]], rtol=2e-4)
    np.testing.assert_allclose(t1, t0, rtol=0, atol=2e-5)
    if with_tvd:
        np.testing.assert_allclose(h1["tvd"], h0["tvd"], rtol=0, atol=1e-5)
    else:
        assert all(np.isnan(v) for v in h1["tvd"])
    assert len(log1) == len(log0) and all(a.split(" | ")[0] == b.split(" | ")[0] for a, b in zip(log0, log1))
    assert h1["kl"][-1] < h1["kl"][0] and min(h1["kl"]) >= -1e-12


def test_nonfinite_table_entry_skips_the_step(dev):
    """A NaN in the objective's table (set after prepare) reaches the loss; the optimiser hand-off's guard leaves theta
    and the optimiser state where they were, in the torch-optimiser step and in the one-launch DeviceAdam step."""
    lat, obs, x = SPRINKLER
    bn = get_sprinkler_network(False)
    vi = make_vi(bn, lat, obs, 3, 2, seed=11)
    vi.objective.prepare(x)
    params, opt, sched = vi.make_optimizer(0.05, 5, False, "adam", (0.9, 0.999))
    l0, _, _, e0 = vi.training_step_async(params, opt, sched, 10.0)
    assert math.isfinite(float(l0)) and math.isfinite(float(e0))
    theta_before = vi.born_machine.theta.detach().clone()
    state_before = {k: v.clone() for k, v in opt.state[params[0]].items() if torch.is_tensor(v)}
    good = vi.objective.log_p.clone()
    vi.objective.log_p[5] = float("nan")
    l1, _, q, _ = vi.training_step_async(params, opt, sched, 10.0)
    assert float(q[5]) > 0 and not math.isfinite(float(l1))
    assert torch.equal(vi.born_machine.theta.detach(), theta_before)
    for k, v in state_before.items():
        assert torch.equal(opt.state[params[0]][k], v), k
    vi.objective.log_p.copy_(good)
    l2, _, _, _ = vi.training_step_async(params, opt, sched, 10.0)
    assert math.isfinite(float(l2)) and not torch.equal(vi.born_machine.theta.detach(), theta_before)
    # the one-launch hand-off
    from tensornetworks_amd.ksd_vi_quantum import DeviceAdam
    vi = make_vi(bn, lat, obs, 3, 2, seed=11)
    vi.objective.prepare(x)
    adam = DeviceAdam(vi.born_machine.theta, 0.05)
    vi.objective.log_p[5] = float("inf")
    loss, grad, _ = vi.elbo_and_grad(theta64=adam.theta64)
    theta_before = vi.born_machine.theta.detach().clone()
    adam.step(grad, loss, 10.0)
    assert not math.isfinite(float(loss)) and torch.equal(vi.born_machine.theta.detach(), theta_before)
    assert int(adam.counters[0]) == 0


def autograd_reference(w, mode, log_p, lam):
    """(loss, entropy, d (loss - lam H) / d w) through softmax / |w| / sum |w| in float64 on the CPU."""
    w64 = w.detach().double().cpu().requires_grad_(True)
    q = torch.softmax(w64, dim=-1) if mode == 0 else w64.abs() / w64.abs().sum()
    l = torch.log(q.clamp(min=1e-10))
    loss = (q * (l - log_p.cpu())).sum()
    H = -(q * l).sum()
    (loss - lam * H).backward()
    return loss.detach(), H.detach(), w64.grad


@pytest.mark.parametrize("n", [3, 6])
@pytest.mark.parametrize("use_logits", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.013])
def test_classical_step_against_autograd(dev, n, use_logits, lam):
    """loss_and_grads of the table machine against torch autograd: the loss and entropy are float64 sums over float32
    probabilities, the gradient carries the float32 q and the float32 rounding of dL/dq (test_gpu_classical.py's
    tolerances for the KSD gradient: 1e-5 of the row's largest entry)."""
    from tensornetworks_amd.elbo_vi import ELBOVariationalInference
    if n == 3:
        bn, (lat, obs, x) = get_sprinkler_network(False), SPRINKLER
    else:
        bn, lat, obs, x = synthetic_network(n, 1)
    torch.manual_seed(7)
    vi = ELBOVariationalInference(bn, lat, obs, {"use_logits": use_logits}, device="cuda:0")
    with torch.no_grad():
        vi.born_machine.params.mul_(20.0)              # (small_random is 0.1 N(0, 1): nearly uniform q otherwise)
    vi.objective.prepare(x)
    loss, ent, q, grads = vi.loss_and_grads(None, lam)
    assert len(grads) == 1 and grads[0][0] is vi.born_machine.params
    g = grads[0][1]
    loss_r, H_r, g_r = autograd_reference(vi.born_machine.params, vi.born_machine.born_mode, vi.objective.log_p, lam)
    torch.testing.assert_close(loss.cpu()[0], loss_r, rtol=2e-6, atol=1e-6)
    torch.testing.assert_close(ent.cpu()[0], H_r, rtol=2e-6, atol=1e-6)
    assert g.dtype == torch.float32 and g.shape == vi.born_machine.params.shape
    assert float(((g.double().cpu() - g_r).abs() / g_r.abs().max()).max()) < 1e-5
    assert float(loss) + vi.objective.log_evidence >= -1e-6


def test_classical_mlp_step_reaches_the_network(dev):
    """Conditioned machine: the logits' gradient from the kernels, carried into the network by torch.autograd."""
    from tensornetworks_amd.elbo_vi import ELBOVariationalInference
    lat, obs, x = SPRINKLER
    torch.manual_seed(2)
    vi = ELBOVariationalInference(get_sprinkler_network(False), lat, obs, {"use_logits": True, "conditioning_dim": 1},
                                  device="cuda:0")
    vi.born_machine.eval()                             # (no Dropout draws: the two forwards below see the same network)
    vi.objective.prepare(x)
    xc = torch.tensor([1.0], device="cuda:0")
    loss, ent, q, grads = vi.loss_and_grads(xc, 0.0)
    vi.apply_grads(grads)
    got = [p.grad.detach().double().cpu().clone() for p in vi.born_machine.parameters()]
    for p in vi.born_machine.parameters():
        p.grad = None
    logits = vi.born_machine.raw_params(xc).double()
    qr = torch.softmax(logits, dim=-1)
    ref = (qr * (torch.log(qr.clamp(min=1e-10)) - vi.objective.log_p)).sum()
    ref.backward()
    torch.testing.assert_close(loss[0], ref.detach(), rtol=2e-6, atol=1e-6)
    for a, p in zip(got, vi.born_machine.parameters()):
        scale = float(p.grad.abs().max())
        assert float((a - p.grad.double().cpu()).abs().max()) <= 1e-4 * scale + 1e-7


@pytest.mark.parametrize("use_logits", [True, False])
def test_classical_sprinkler_run_improves(dev, use_logits, capsys):
    from tensornetworks_amd.elbo_vi import ELBOVariationalInference
    lat, obs, x = SPRINKLER
    bn = get_sprinkler_network(False)
    post, _ = bn.get_true_posterior(lat, x)
    torch.manual_seed(0)
    vi = ELBOVariationalInference(bn, lat, obs, {"use_logits": use_logits}, device="cuda:0")
    hist = vi.train(x, 300, 0.05, verbose=True, true_posterior_for_tvd=post)
    out = capsys.readouterr().out
    assert "| ELBO:" in out and "| Entropy:" in out and "KSD" not in out
    assert set(hist) == {'loss_elbo', 'kl', 'entropy', 'tvd', 'grad_norm'}
    print(f"use_logits={use_logits}: kl {hist['kl'][0]:.4e} -> {hist['kl'][-1]:.4e}, tvd {hist['tvd'][0]:.4e} -> {hist['tvd'][-1]:.4e}")
    assert hist['kl'][-1] < hist['kl'][0] and hist['tvd'][-1] < hist['tvd'][0]
    assert min(hist['kl']) >= -1e-6                    # (the loss is evaluated on float32 probabilities)
