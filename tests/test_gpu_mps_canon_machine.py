"""The MPS machines' canonical-form surface on the MI355X: canonicalise_, compress_ and expand_ leave q alone, the spectrum of
an expanded model has exact zeros, and bond_dim changes between train() calls.

Bounds.  The canonicaliser changes psi / sqrt(Z) by at most C EPS64 in norm, C = mps_canon_mirror.derived_constant (the
first-order worst case; test_gpu_mps_canon_kernel.py states it).  A sum of q over a set of states of mass m then moves by at
most 2 C EPS64 sqrt(m): a marginal by 2 C EPS64, a log-marginal or log q(z) by 2 C EPS64 / sqrt(m).  To that the bounds of the
two calls compared are added (they dominate: kappa of the environments grows with n, so at n <= 12 the normalised state is also
enumerated in extended precision before and after and compared against C EPS64 alone): c_marg (marginals), logm_bound (log-marginals) of test_gpu_mps_query_kernel.py, logq_bound
(log q of a state) of test_gpu_mps_sampled_kernel.py, and for the enumerated machine q64's own of test_gpu_mps_kernel.py."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_canon_mirror as cm
import mps_query_mirror as qm
import mps_sampled_mirror as sm
import test_gpu_mps_query_kernel as tq
import test_gpu_mps_sampled_kernel as tk

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
EVIDENCES = lambda n: [{0: 1}, {1: 0, n - 1: 1}, {2: 1, n // 2: 0, n - 2: 1}]


def sampled_machine(n, D, seed=5):
    from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine
    torch.manual_seed(seed)
    return SampledMPSBornMachine(n, bond_dim=D, init_method="small_random", seed=11).to("cuda")


def snapshot(bm, idx=None):
    """(marginals, log-marginals of the three evidences, log q of 65 drawn states, the states) and the calls' own bounds."""
    n, D = bm.num_latent_vars, bm.bond_dim
    cores = bm.cores.detach().cpu().numpy()
    env = sm.environments(cores)
    kZ = float(env["Z_abs"] / env["Z"])
    if idx is None:
        idx, _ = bm.sample_indices(65, epoch=2)
    m1 = bm.marginals().cpu().numpy()
    lm = bm.log_marginal(EVIDENCES(n)).cpu().numpy()
    lq = bm.log_prob(idx).cpu().numpy()
    ref_m = qm.marginals(cores, env)
    b_m1 = EPS * tq.c_marg(n, D, kZ) * hp.to_f64(ref_m["m1_abs"])
    refs = [qm.log_marginal(cores, ev, env) for ev in EVIDENCES(n)]
    b_lm = np.array([EPS * tq.logm_bound(n, D, r) for r in refs])
    mass = np.array([float(np.exp(r["logm"])) for r in refs])
    cond = sm.conditionals(cores, sm.bits_of_idx(idx.cpu().numpy(), n), env)
    kb = hp.to_f64(cond["psi_abs"] / np.abs(cond["psi"]))
    b_lq = EPS * tk.logq_bound(n, D, kb, kZ, hp.to_f64(cond["logq"]), float(np.log(env["Z"])))
    out = dict(m1=m1, lm=lm, lq=lq, idx=idx, b_m1=b_m1, b_lm=b_lm, b_lq=b_lq, mass=mass, q_of_idx=np.exp(hp.to_f64(cond["logq"])))
    if n <= 12:                                  # the normalised state itself, enumerated in extended precision: no query in between
        psi, Z = cm.psi_of(cores)
        out["state"] = psi / np.sqrt(Z)
    return out


def assert_same_q(a, b, C, what):
    r1 = np.abs(a["m1"] - b["m1"]) / (a["b_m1"] + b["b_m1"] + 2 * C * EPS)
    r2 = np.abs(a["lm"] - b["lm"]) / (a["b_lm"] + b["b_lm"] + 2 * C * EPS / np.sqrt(a["mass"]))
    r3 = np.abs(a["lq"] - b["lq"]) / (a["b_lq"] + b["b_lq"] + 2 * C * EPS / np.sqrt(a["q_of_idx"]))
    print(f"{what}: worst ratio to the bound: marginals {r1.max():.2e}, log-marginals {r2.max():.2e}, log q {r3.max():.2e}")
    assert r1.max() <= 1.0 and r2.max() <= 1.0 and r3.max() <= 1.0
    if "state" in a:
        e = float(np.abs(a["state"] - b["state"]).max() / cm.LD(EPS))
        print(f"    max_z |psi / sqrt(Z) - the same before| = {e:.1f} EPS64 (C {C:.0f})")
        assert e <= C


@pytest.mark.parametrize("n,D", [(6, 4), (40, 4)])
def test_sampled_machine_keeps_q(n, D):
    bm = sampled_machine(n, D)
    C = cm.derived_constant(n, 8)
    before = snapshot(bm)
    param = bm.cores
    spectrum = bm.bond_spectrum()
    entropies = bm.bond_entropies()
    assert spectrum.shape == (n - 1, D) and entropies.shape == (n - 1,) and spectrum.device.type == "cuda"
    assert not spectrum.requires_grad and spectrum.dtype == torch.float64
    p = spectrum.cpu().numpy() ** 2
    want = -(p * np.log(np.where(p > 0, p, 1.0))).sum(axis=1)
    assert np.abs(entropies.cpu().numpy() - want).max() <= 16 * D * EPS and bool((entropies >= 0).all())
    cores_c, report = bm.canonical_cores()
    assert bm.cores is param and set(report) == {"rank", "discarded", "log_norm", "status"}
    assert cores_c.shape == bm.cores.shape and not cores_c.requires_grad

    report = bm.canonicalise_()
    assert bm.cores is param and int(report["status"].item()) == 0                 # in place: the same parameter
    assert torch.equal(bm.cores.detach(), cores_c)
    assert_same_q(before, snapshot(bm, before["idx"]), C, f"({n}, {D}) canonicalise_")
    assert abs(float(bm.canonical_cores()[1]["log_norm"].item())) <= 4 * C * EPS   # its own Z is 1

    report = bm.compress_(bond_dim=D)
    assert bm.cores is not param and isinstance(bm.cores, torch.nn.Parameter) and bm.bond_dim == D
    assert int(report["status"].item()) == 0 and float(report["discarded"].sum().item()) == 0.0
    assert_same_q(before, snapshot(bm, before["idx"]), C, f"({n}, {D}) compress_(bond_dim=D)")

    old_spectrum = bm.bond_spectrum().cpu().numpy()
    bm.expand_(8)
    assert bm.bond_dim == 8 and tuple(bm.cores.shape) == (n, 2, 8, 8) and bm.cores.device.type == "cuda"
    assert_same_q(before, snapshot(bm, before["idx"]), C, f"({n}, {D}) expand_(8)")
    grown = bm.bond_spectrum().cpu().numpy()
    for k in range(n - 1):
        rk = int((old_spectrum[k] > 0).sum())
        assert np.all(grown[k, rk:] == 0.0) and np.all(grown[k, :rk] > 0.0)        # exact zeros beyond the old rank
    assert np.abs(grown[:, :D] - old_spectrum).max() <= 2 * C * EPS
    report = bm.compress_()                                                        # back to the largest kept rank
    assert bm.bond_dim == int(report["rank"].max().item()) <= D
    assert_same_q(before, snapshot(bm, before["idx"]), C, f"({n}, {D}) compress_()")


def test_enumerated_machine_keeps_q():
    from tensornetworks_amd.born_machine_mps import MPSBornMachine
    n, D = 6, 4
    torch.manual_seed(6)
    bm = MPSBornMachine(n, bond_dim=D, init_method="small_random").to("cuda")
    C = cm.derived_constant(n, 8)

    def q_and_bound():
        cores = bm.cores.detach().cpu().numpy()
        env = sm.environments(cores)
        kZ = float(env["Z_abs"] / env["Z"])
        cond = sm.conditionals(cores, sm.bits_of_idx(np.arange(1 << n), n), env)
        kz = hp.to_f64(cond["psi_abs"] / np.abs(cond["psi"]))
        q = bm.probabilities64().detach().cpu().numpy()
        return q, EPS * q * ((2 * (n * bm.bond_dim + 2) + 1) * (kz + kZ) + 2 + 29)       # test_gpu_mps_kernel.py's bound of q64

    q0, b0 = q_and_bound()
    steps = [("canonicalise_", lambda: bm.canonicalise_()), ("compress_(bond_dim=D)", lambda: bm.compress_(bond_dim=D)),
             ("expand_(8)", lambda: bm.expand_(8)), ("compress_()", lambda: bm.compress_())]
    for name, step in steps:
        param = bm.cores
        report = step()
        assert (bm.cores is param) == (name == "canonicalise_")
        if report is not None:
            assert int(report["status"].item()) == 0
        q1, b1 = q_and_bound()
        ratio = np.abs(q1 - q0) / (b0 + b1 + 2 * C * EPS * np.sqrt(q0))
        print(f"enumerated ({n}, {D}) {name}: worst |q - q before| / bound = {ratio.max():.2e}")
        assert ratio.max() <= 1.0
    assert bm.bond_dim <= D
    spectrum = bm.bond_spectrum()
    assert spectrum.shape == (n - 1, bm.bond_dim) and bool((bm.bond_entropies() >= 0).all())
    loss = (bm.probabilities64() ** 2).sum()
    loss.backward()
    assert bm.cores.grad is not None and bm.cores.grad.shape == bm.cores.shape       # the new parameter trains


@pytest.mark.parametrize("natural_gradient", [None, "site"])
def test_train_expand_train_compress_train(natural_gradient):
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(12, 0)
    torch.manual_seed(3)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': 2, 'num_samples': 512, 'seed': 7}, device='cuda',
                                         natural_gradient=natural_gradient)
    bm = vi.born_machine
    hist = [vi.train(x, 20, 0.05, verbose=False)]
    assert bm.bond_entropies().shape == (11,)
    bm.expand_(4, noise=1e-2, seed=1)
    assert bm.bond_dim == 4
    hist.append(vi.train(x, 20, 0.05, verbose=False))
    report = bm.compress_(cutoff=1e-8)
    assert int(report["status"].item()) == 0 and bm.bond_dim == int(report["rank"].max().item())
    assert float(report["discarded"].max().item()) <= 1e-8
    hist.append(vi.train(x, 20, 0.05, verbose=False))
    key = vi.LOSS_KEYS[0]
    for h in hist:
        assert len(h[key]) == 20 and np.all(np.isfinite(h[key]))
    assert tuple(bm.cores.shape) == (12, 2, bm.bond_dim, bm.bond_dim) and bool(torch.isfinite(bm.cores).all())
