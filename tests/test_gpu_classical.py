"""Classical Born machine and its KSD trainer on the MI355X: kernel-level checks of born_table_probs / born_table_vjp
against float64 torch autograd of the reference's formulas, replays of the reference's recorded classical traces,
the MLP epoch with Dropout active against the torch restatement (classical_mirror.py), early stopping, the sampler and
the example script."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classical_mirror as mirror
from conftest import REPO, golden
from oracle import stein as os_
from tensornetworks_amd import backend
from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
from tensornetworks_amd.born_machine_classical_sim import ClassicalBornMachine
from tensornetworks_amd.ksd_vi import KSDVariationalInference
from tensornetworks_amd.utils import generate_all_binary_outcomes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT, OBS, X = ['C', 'S', 'R'], ['W'], {'W': 1}
CASES = ["classical_sprinkler_logits", "classical_sprinkler_abs", "classical_sprinkler_sgd", "classical_synthetic_n6",
         "classical_sprinkler_mlp"]


# ---- kernel level ----------------------------------------------------------------------------------------------
def reference_terms(w, mode, y, ksd2, lam):
    """float64 torch autograd of the reference's graph per row: q = softmax(w - max w) or |w| / sum |w|,
    H = -sum q log clamp(q, 1e-10), L = sqrt(clamp(ksd2, 1e-12)) (through dL/dq = y / L) - lam H.  On the CPU: torch's
    float64 softmax on the GPU is itself ~1e-6 relative off a correctly rounded one, the CPU's is not."""
    w, y, ksd2 = w.cpu(), y.cpu(), ksd2.cpu()
    w64 = w.detach().double().requires_grad_(True)
    if mode == 0:
        q = torch.softmax(w64 - w64.max(dim=-1, keepdim=True)[0], dim=-1)
    else:
        a = torch.abs(w64)
        q = a / a.sum(dim=-1, keepdim=True)
    H = -(q * torch.log(q.clamp(min=1e-10))).sum(dim=-1)
    loss = torch.sqrt(ksd2.clamp(min=1e-12))
    scale = torch.where(ksd2 >= 1e-12, 1.0 / loss, torch.zeros_like(loss))
    L = ((q * y).sum(dim=-1) * scale).sum() - lam * H.sum()
    L.backward()
    return q.detach(), H.detach(), w64.grad, loss


def make_rows(n, rows, kind, gen):
    N = 1 << n
    if kind == "random":
        return (torch.randn(rows, N, generator=gen) * 2.0).to(DEV)
    if kind == "spread":           # logits over a range of 200: most q underflow to 0, the entropy clamp is active
        return (torch.rand(rows, N, generator=gen) * 200.0 - 200.0).to(DEV)
    if kind == "equal":
        return torch.full((rows, N), 0.37).to(DEV)
    if kind == "zeros":            # abs mode: sign(0) = 0 entries
        w = torch.randn(rows, N, generator=gen)
        w[:, ::3] = 0.0
        return w.to(DEV)
    raise ValueError(kind)


@pytest.mark.parametrize("n", [1, 3, 8, 12, 16, 20])
@pytest.mark.parametrize("mode,kind", [(0, "random"), (0, "spread"), (0, "equal"),
                                       (1, "random"), (1, "spread"), (1, "equal"), (1, "zeros")])
def test_kernels_against_autograd(n, mode, kind):
    """The coarse check against torch: q to 3 float32 ulps, H to 2e-6, the gradient relative to its row's largest entry (so
    entries proportional to a small q, and the entropy clamp's indicator, weigh nothing here).  The per-entry bounds
    against extended precision, the clamp's edge and the unaligned (scalar) path are test_gpu_classical_precision.py's."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * mode + len(kind))
    rows = 3 if n < 20 else 2
    w = make_rows(n, rows, kind, gen)
    if kind == "spread" and mode == 1:
        w = w.abs()
    y = (torch.randn(rows, 1 << n, generator=gen, dtype=torch.float64)).to(DEV)
    ksd2 = torch.tensor([2.5, 1e-13, 0.7][:rows], dtype=torch.float64, device=DEV)     # row 1: the clamp is active
    lam = 0.013
    q32, q64, H = backend.born_table_probs(w, mode)
    assert torch.equal(q64, q32.double())                   # the exact upcast
    loss = torch.empty(rows, dtype=torch.float64, device=DEV)
    g = backend.born_table_vjp(w, q64, mode, y=y, ksd2=ksd2, entropy_weight=lam, loss_out=loss)
    q_ref, H_ref, g_ref, loss_ref = (t.to(DEV) for t in reference_terms(w, mode, y, ksd2, lam))
    # q: one float32 rounding of a float64 value
    torch.testing.assert_close(q32.double(), q_ref, rtol=2e-7, atol=1e-12)
    # H: float64 sums over float32 probabilities
    torch.testing.assert_close(H.double(), H_ref, rtol=2e-6, atol=1e-6)
    torch.testing.assert_close(loss, loss_ref, rtol=1e-15, atol=0)
    # the gradient: float32 q and the float32 rounding of y / L (the reference's upcast backward) against float64
    # (relative to the row's largest entry; a row whose gradient cancels to rounding noise -- equal logits with the
    # KSD term clamped away -- is held to an absolute 1e-5 of lambda)
    scale = g_ref.abs().amax(dim=-1, keepdim=True).clamp(min=lam)
    assert ((g.double() - g_ref).abs() / scale).max() < 1e-5
    if kind == "zeros":
        assert bool((g[:, ::3] == 0).all())


def test_kernels_each_term_alone_and_generic_backward():
    gen = torch.Generator().manual_seed(3)
    w = (torch.randn(2, 256, generator=gen)).to(DEV).requires_grad_(True)
    from tensornetworks_amd.born_machine_classical_sim import _TableEntropy, _TableProbs
    c = torch.randn(2, 256, generator=gen).to(DEV)
    (_TableProbs.apply(w, 0) * c).sum().backward()
    g1 = w.grad.clone()
    w.grad = None
    _TableEntropy.apply(w, 0).backward()
    g2 = w.grad.clone()
    w64 = w.detach().double().requires_grad_(True)
    q = torch.softmax(w64, dim=-1)
    (q * c.double()).sum().backward()
    torch.testing.assert_close(g1.double(), w64.grad, rtol=1e-4, atol=1e-7)
    w64.grad = None
    q = torch.softmax(w64, dim=-1)
    (-(q * torch.log(q.clamp(min=1e-10))).sum()).backward()
    torch.testing.assert_close(g2.double(), w64.grad, rtol=1e-4, atol=1e-7)


def test_kernels_bitwise_deterministic():
    gen = torch.Generator().manual_seed(9)
    for mode in (0, 1):
        w = torch.randn(1, 1 << 16, generator=gen).to(DEV)
        y = torch.randn(1, 1 << 16, generator=gen, dtype=torch.float64).to(DEV)
        ksd2 = torch.tensor([3.0], dtype=torch.float64, device=DEV)
        a = backend.born_table_probs(w, mode)
        b = backend.born_table_probs(w, mode)
        ga = backend.born_table_vjp(w, a[1], mode, y=y, ksd2=ksd2, entropy_weight=0.01)
        gb = backend.born_table_vjp(w, b[1], mode, y=y, ksd2=ksd2, entropy_weight=0.01)
        for s, t in zip(a + (ga,), b + (gb,)):
            assert torch.equal(s, t)


def test_nan_reaches_loss_and_trainer_skips():
    w = torch.randn(1, 64).to(DEV)
    w[0, 5] = float("nan")
    q32, q64, H = backend.born_table_probs(w, 0)
    assert bool(torch.isnan(q32).all()) and bool(torch.isnan(H).all())
    torch.manual_seed(0)
    vi = KSDVariationalInference(get_sprinkler_network(False), LAT, OBS, {'use_logits': True, 'conditioning_dim': 0},
                                 device=DEV)
    with torch.no_grad():
        vi.born_machine.params[2] = float("nan")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        hist = vi.train(X, num_epochs=2, lr_born_machine=0.01, verbose=False)
    assert out.getvalue().count("Warning: NaN or Inf loss: nan. Skipping update.") == 2
    assert all(np.isnan(hist['loss_ksd'])) and hist['grad_norm'] == [0.0, 0.0] and all(np.isnan(hist['entropy']))


# ---- replays of the reference's traces -----------------------------------------------------------------------
def recording(vi):
    """Wraps vi.loss_and_grads: records the q of every loss forward and the parameters each epoch starts from."""
    rec = {"q": [], "params": []}
    orig = vi.loss_and_grads

    def spy(*a, **k):
        rec["params"].append(torch.cat([p.detach().reshape(-1) for p in vi.born_machine.parameters()]).cpu().numpy())
        out = orig(*a, **k)
        rec["q"].append(out[2].detach().cpu().numpy().copy())
        return out
    vi.loss_and_grads = spy
    return rec


def test_replays_classical_trace():
    g = golden("classical_trace.npz")
    torch.manual_seed(7)
    vi = KSDVariationalInference(get_sprinkler_network(False), LAT, OBS, {'use_logits': True, 'conditioning_dim': 0},
                                 device=DEV)
    rec = recording(vi)
    with contextlib.redirect_stdout(io.StringIO()):
        hist = vi.train(X, num_epochs=5, lr_born_machine=0.01, verbose=False, true_posterior_for_tvd=None,
                        entropy_weight=0.0)
    np.testing.assert_allclose(np.array(rec["q"]), g["q_all"][::2], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(hist['loss_ksd'], g["loss_ksd"], rtol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_replays_reference_golden(name):
    """The drop-in against the reference's own run of the same seed and hyper-parameters.  Tolerances are float32-level:
    the kernels round a float64 softmax once (torch computes it in float32: <= 2 ulp apart), K_p q is summed in a
    different order (1e-15), and 40 optimiser steps carry these into the parameters (Adam steps by lr m/sqrt(v): a
    relative gradient error e moves a step by ~e lr), so 1e-5 relative on everything and 1e-4 on the parameters."""
    g = golden(name + ".npz")
    n = int(g["n"])
    if n == 3:
        bn, lat, obs, x = get_sprinkler_network(False), LAT, OBS, {'W': int(g["x_value"][0])}
    else:
        bn, lat, obs, x = synthetic_network(n, 0)
    post = dict(zip(generate_all_binary_outcomes(n), (float(v) for v in g["posterior"])))
    torch.manual_seed(int(g["seed"]))
    vi = KSDVariationalInference(bn, lat, obs, {'use_logits': bool(g["use_logits"]),
                                                'conditioning_dim': int(g["conditioning_dim"])}, device=DEV)
    if int(g["conditioning_dim"]) > 0:
        vi.born_machine.param_generator_net.eval()
    rec = recording(vi)
    E = len(g["loss_ksd"])
    with contextlib.redirect_stdout(io.StringIO()):
        hist = vi.train(x, num_epochs=E, lr_born_machine=float(g["lr"]), verbose=False, true_posterior_for_tvd=post,
                        gradient_clip_norm=float(g["clip"]), optimizer_type="sgd" if bool(g["sgd"]) else "adam",
                        entropy_weight=float(g["entropy_weight"]), patience=200)
    rec["params"].append(torch.cat([p.detach().reshape(-1) for p in vi.born_machine.parameters()]).cpu().numpy())
    np.testing.assert_array_equal(rec["params"][0], g["params"][0])
    np.testing.assert_allclose(np.array(rec["q"]), g["q"], rtol=1e-5, atol=1e-6)
    for key in ("loss_ksd", "entropy", "tvd"):
        np.testing.assert_allclose(hist[key], g[key], rtol=1e-5, atol=1e-6, err_msg=key)
    # the norm of a gradient of size ~300 summed in float32 by clip_grad_norm_ over gradients that differ in their last
    # float32 bits: 1e-4 relative
    np.testing.assert_allclose(hist["grad_norm"], g["grad_norm"], rtol=1e-4, atol=1e-6)
    params = np.array(rec["params"])[g["param_epochs"]]
    np.testing.assert_allclose(params, g["params"], rtol=1e-4, atol=1e-5)
    fixed = vi.born_machine._fixed_probs.cpu().numpy()
    np.testing.assert_allclose(fixed, g["fixed_probs"], rtol=1e-5, atol=1e-6)


def test_tensor_posterior_gives_the_same_history():
    from tensornetworks_amd.stein_utils import true_posterior_table
    bn = get_sprinkler_network(False)
    runs = []
    for table in (False, True):
        torch.manual_seed(2)
        vi = KSDVariationalInference(bn, LAT, OBS, {'use_logits': True, 'conditioning_dim': 0}, device=DEV)
        post = true_posterior_table(bn, X, LAT, device=DEV)[0] if table else bn.get_true_posterior(LAT, X)[0]
        with contextlib.redirect_stdout(io.StringIO()):
            runs.append(vi.train(X, num_epochs=15, lr_born_machine=0.02, verbose=False, true_posterior_for_tvd=post))
    for key in ("loss_ksd", "entropy", "grad_norm"):
        assert runs[0][key] == runs[1][key]
    # (the dict path subtracts float32 probabilities from Python floats in float32, the table path in float64)
    np.testing.assert_allclose(runs[0]["tvd"], runs[1]["tvd"], rtol=1e-5, atol=1e-6)


# ---- MLP with Dropout active against the torch restatement -------------------------------------------------------
def test_mlp_dropout_epochs_equal_torch_restatement():
    bn = get_sprinkler_network(False)
    torch.manual_seed(0)
    vi = KSDVariationalInference(bn, LAT, OBS, {'use_logits': True, 'conditioning_dim': 1}, device=DEV)
    bm = mirror.MirrorBornMachine(3, use_logits=True, conditioning_dim=1).to(DEV)
    bm.load_state_dict(vi.born_machine.state_dict())
    assert vi.born_machine.training and bm.training
    K = torch.from_numpy(os_.gram_closed_form(os_.score_matrix(bn, X, LAT, OBS), 3)).to(DEV)
    post = bn.get_true_posterior(LAT, X)[0]
    E = 12
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        hist = vi.train(X, num_epochs=E, lr_born_machine=0.003, verbose=False, true_posterior_for_tvd=post,
                        gradient_clip_norm=5.0, entropy_weight=0.001)
    torch.manual_seed(11)
    h_ref, _, fixed_ref = mirror.train(bm, K, post, torch.tensor([1.0], device=DEV), num_epochs=E, lr=0.003, clip=5.0,
                                       entropy_weight=0.001)
    # same Dropout masks (same generator draws in the same order); the rest is float32 rounding
    for key in ("loss_ksd", "entropy", "grad_norm", "tvd"):
        np.testing.assert_allclose(hist[key], h_ref[key], rtol=1e-4, atol=1e-6, err_msg=key)
    np.testing.assert_allclose(vi.born_machine._fixed_probs.cpu().numpy(), fixed_ref, rtol=1e-4, atol=1e-6)
    ours = torch.cat([p.detach().reshape(-1) for p in vi.born_machine.param_generator_net.parameters()])
    theirs = torch.cat([p.detach().reshape(-1) for p in bm.param_generator_net.parameters()])
    torch.testing.assert_close(ours, theirs, rtol=1e-4, atol=1e-6)


# ---- early stopping, restore -----------------------------------------------------------------------------------
def test_early_stopping_follows_the_reference_rule():
    torch.manual_seed(1)
    bn = get_sprinkler_network(False)
    vi = KSDVariationalInference(bn, LAT, OBS, {'use_logits': True, 'conditioning_dim': 0}, device=DEV)
    patience, epochs = 1, 420
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        hist = vi.train(X, num_epochs=epochs, lr_born_machine=0.3, verbose=True,
                        true_posterior_for_tvd=bn.get_true_posterior(LAT, X)[0], patience=patience)
    tvd = hist['tvd']
    best, stale, stop = float('inf'), 0, None
    for e, t in enumerate(tvd):
        if t < best:
            best, stale = t, 0
        else:
            stale += 1
        if stale > patience and e > 300:
            stop = e
            break
    # the run stops exactly where the reference's rule first holds on its own TVD history, and nowhere else
    if stop is None:
        assert len(tvd) == epochs and "Early stopping" not in out.getvalue()
    else:
        assert len(tvd) == stop + 1 == len(hist['loss_ksd']) == len(hist['entropy'])
        assert f"Early stopping at epoch {stop + 1} (no improvement for {patience} epochs)" in out.getvalue()
    assert "Successfully restored best probabilities!" in out.getvalue()
    assert vi.born_machine._use_fixed_probs


def test_restore_happens_without_verbose():
    torch.manual_seed(1)
    bn = get_sprinkler_network(False)
    vi = KSDVariationalInference(bn, LAT, OBS, {'use_logits': False, 'conditioning_dim': 0}, device=DEV)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        hist = vi.train(X, num_epochs=10, lr_born_machine=0.05, verbose=False,
                        true_posterior_for_tvd=bn.get_true_posterior(LAT, X)[0])
    assert vi.born_machine._use_fixed_probs and "Restoring" not in out.getvalue()
    best = int(np.argmin(hist['tvd']))
    d = vi.born_machine.get_prob_dict()
    post = bn.get_true_posterior(LAT, X)[0]
    from tensornetworks_amd.utils import calculate_tvd
    assert abs(calculate_tvd(post, d) - hist['tvd'][best]) <= 1e-6


# ---- sampler, log q, fixed probabilities ------------------------------------------------------------------------
def test_sample_log_q_and_fixed_probs():
    torch.manual_seed(5)
    bm = ClassicalBornMachine(4).to(DEV)
    with torch.no_grad():
        bm.params.copy_(torch.linspace(-2, 2, 16))
    q = bm.get_probabilities()
    assert q.shape == (1, 16) and q.dtype == torch.float32 and q.device.type == "cuda"
    z = bm.sample(200000)
    assert z.shape == (200000, 4) and z.dtype == torch.float32 and set(z.unique().tolist()) <= {0.0, 1.0}
    idx = (z.long() * torch.tensor([8, 4, 2, 1], device=z.device)).sum(1)
    freq = torch.bincount(idx, minlength=16).double() / 200000
    assert (freq - q[0].double()).abs().max() < 0.01
    lq = bm.get_log_q_z_x(z[:100])
    torch.testing.assert_close(lq, torch.log(q[0].clamp(min=1e-10))[idx[:100]])
    with pytest.raises(ValueError, match="is not a valid outcome"):
        bm.get_log_q_z_x(torch.tensor([[0.0, 1.0, 3.0, 0.0]], device=DEV))
    d = bm.get_prob_dict()
    assert len(d) == 16 and abs(sum(float(v) for v in d.values()) - 1.0) < 1e-6
    torch.testing.assert_close(bm.entropy(), -(q * torch.log(q.clamp(min=1e-10))).sum(), rtol=1e-5, atol=1e-6)
    bm.set_fixed_probs(q[0])
    assert torch.equal(bm.get_probabilities(), q)
    bm.clear_fixed_probs()

    cbm = ClassicalBornMachine(3, conditioning_dim=1).to(DEV)
    cbm.eval()
    xs = torch.tensor([[0.0], [1.0]], device=DEV)
    zs = cbm.sample(7, xs)
    assert zs.shape == (2, 7, 3)
    qb = cbm.get_probabilities(xs)
    lq = cbm.get_log_q_z_x(zs[:, 0, :], xs)              # B_x = B_z
    ib = (zs[:, 0, :].long() * torch.tensor([4, 2, 1], device=DEV)).sum(1)
    torch.testing.assert_close(lq, torch.log(qb.clamp(min=1e-10))[torch.arange(2), ib])
    with pytest.raises(ValueError, match="Batch size mismatch"):
        cbm.get_log_q_z_x(torch.zeros(3, 3, device=DEV), xs)
    with pytest.raises(ValueError, match="single distribution"):
        cbm.get_prob_dict(xs)


def test_example_script_runs():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "run_sprinkler_ksd.py"), "--epochs", "30", "--quiet"],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Final TVD:" in r.stdout and "(1, 1, 1)" in r.stdout
