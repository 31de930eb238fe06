"""Host checks of the two-site sweeps, no device: the mirror's mathematics (tests/mps_twosite_mirror.py)
against torch autograd and against its own invariants, the effect on the 10-variable chain, the new header and the Python
argument checks.

Bounds: hp.measured_constant(what the extended mirror itself shows, mps_twosite_mirror.derived_constant) in units of EPS64
against 1 -- the state has norm 1."""
import functools
import os

import numpy as np
import pytest
import torch

import amortised_mirror as am
import hp_reference as hp
import mps_canon_mirror as cm
import mps_twosite_mirror as tm
from conftest import REPO
from tensornetworks_amd.bayesian_network import pack_network_for_sampling

EPS = hp.EPS64

# The chain case: 10 variables (true bond rank 2), cap 8, the product state, one set of B draws of amortised_mirror.bn_sample
# (seed SAMPLE_SEED, epoch 0), lr 0.1, 5 steps a bond, 5 round trips.  CHAIN_SEED and SAMPLE_SEED are the committed seeds.
CHAIN = dict(n=10, cap=8, B=8192, lr=0.1, steps=5, sweeps=5, chain_seed=0, sample_seed=0)


def random_canonical(n, D, seed):
    rng = np.random.default_rng(seed)
    return tm.canonical((np.eye(D) + 0.3 * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0))


def test_merged_gradient_equals_autograd():
    rng = np.random.default_rng(7)
    D, B = 3, 40
    M = rng.standard_normal((2, 2, D, D))
    l, r = rng.standard_normal((B, D)), rng.standard_normal((B, D))
    s, t = rng.integers(0, 2, B), rng.integers(0, 2, B)
    w = rng.uniform(0.1, 1.0, B)
    loss, grad, good = tm.loss_and_grad(M, l, r, s, t, w)
    assert good.all()
    Mt = torch.tensor(M, requires_grad=True)
    lt, rt, wt = torch.tensor(l), torch.tensor(r), torch.tensor(w)
    psi = torch.einsum("ba,bac,bc->b", lt, Mt[torch.tensor(s), torch.tensor(t)], rt)
    L = wt.sum() * torch.log((Mt * Mt).sum()) - (wt * torch.log(psi * psi)).sum()
    L.backward()
    scale = float(np.abs(grad).max())
    assert abs(float(L.detach()) - float(loss)) <= 64 * EPS * (1.0 + abs(float(loss)))
    assert np.abs(Mt.grad.numpy() - grad).max() <= 64 * B * EPS * scale          # two B-term sums in different orders
    # the gradient is orthogonal to M at |M| = 1
    Mn = M / np.sqrt((M * M).sum())
    _, gn, _ = tm.loss_and_grad(Mn, l, r, s, t, w)
    assert abs(float((gn * Mn).sum())) <= 64 * B * EPS * float(np.abs(gn).max())


def test_round_trip_with_lr_zero_returns_psi_and_keeps_Z():
    n, D, B = 6, 3, 65
    c = random_canonical(n, D, 1)
    idx = np.random.default_rng(2).integers(0, 1 << n, B)
    psi0, Z0 = cm.psi_of(c)
    seen = []
    r = tm.sweep(c, idx, lr=0.0, steps=1, on_bond=lambda j, cc: seen.append(float(abs(cm.psi_of(hp.to_f64(cc))[1] - 1) / EPS)))
    rl = tm.sweep(c, idx, lr=0.0, steps=1, dtype=tm.LD)
    derived = tm.derived_constant(n, D, 1)
    own = float(np.abs(cm.psi_of(hp.to_f64(rl["cores"]))[0] - psi0).max() / EPS)       # the extended mirror, rounded to float64 cores
    C = hp.measured_constant(own, derived)
    e = float(np.abs(cm.psi_of(hp.to_f64(r["cores"]))[0] - psi0).max() / EPS)
    print(f"lr = 0: max_z |psi_out - psi_in| = {e:.1f} EPS64 (C {C:.0f}, extended mirror {own:.1f}); |Z - 1| after every bond <= {max(seen):.1f} EPS64")
    assert r["status"] == 0 and e <= C
    assert len(seen) == 2 * (n - 1) and max(seen) <= 2 * C                               # Z is the square of the norm
    assert np.array_equal(r["rank"], rl["rank"])


def test_Z_stays_one_with_steps_and_cuts():
    n, D, B = 6, 4, 200
    c = random_canonical(n, D, 3)
    q = tm.probabilities(c)
    idx = np.random.default_rng(4).choice(1 << n, size=B, p=q / q.sum())
    seen = []
    r = tm.sweep(c, idx, lr=0.05, steps=3, D_keep=3, cutoff=1e-3,
                 on_bond=lambda j, cc: seen.append(float(abs(cm.psi_of(hp.to_f64(cc))[1] - 1) / EPS)))
    C = tm.derived_constant(n, D, 3)
    print(f"|Z - 1| after every bond <= {max(seen):.1f} EPS64 (derived {C:.0f}); ranks {r['rank'].tolist()}")
    assert r["status"] == 0 and max(seen) <= 2 * C and r["rank"].max() <= 3
    out = hp.to_f64(r["cores"])
    assert np.all(out[0, :, 1:, :] == 0.0) and np.all(out[n - 1, :, :, 1:] == 0.0)
    for k in range(2, n + 1):                                                           # the entry gauge again
        rk = int(r["rank"][k - 2])
        A = out[k - 1]
        assert np.all(A[:, rk:, :] == 0.0)
        assert np.abs(A[0] @ A[0].T + A[1] @ A[1].T - np.eye(D))[:rk, :rk].max() <= C * EPS


@functools.lru_cache(maxsize=None)
def chain_run(cutoff, dtype=np.float64):
    """The chain case with the mirror: (ranks of the last round trip, exact KL(p || q), the cores, the per-sweep reports)."""
    S = CHAIN
    bn, sites = tm.chain_network(S["n"], S["chain_seed"])
    packed = pack_network_for_sampling(bn, sites)
    p = am.site_joint(bn, sites)
    idx = am.bn_sample(packed, S["n"], S["sample_seed"], 0, S["B"])["idx"].astype(np.int64)
    c = tm.product_state(S["n"], S["cap"])
    reports = []
    for _ in range(S["sweeps"]):
        r = tm.sweep(tm.canonical(c), idx, lr=S["lr"], steps=S["steps"], cutoff=cutoff, dtype=dtype)
        c = hp.to_f64(r["cores"])
        reports.append(r)
    return reports[-1]["rank"].tolist(), tm.forward_kl(c, p), c, reports


def check_chain_condition(rank_cut, kl_cut, kl_full, cap):
    """What the chain case must show: with cutoff 1e-4 every bond ends below the cap, and its exact KL is below half of the
    cutoff-0 run's."""
    assert max(rank_cut) < cap, rank_cut
    assert kl_cut < 0.5 * kl_full, (kl_cut, kl_full)


def test_chain_ranks_follow_the_data():
    rank_cut, kl_cut, _, _ = chain_run(1e-4)
    rank_full, kl_full, _, _ = chain_run(0.0)
    print(f"cutoff 1e-4: ranks {rank_cut}, KL {kl_cut:.5f};  cutoff 0: ranks {rank_full}, KL {kl_full:.5f}")
    check_chain_condition(rank_cut, kl_cut, kl_full, CHAIN["cap"])


def test_header_parses_and_leaves_the_bornvi_h_tables_alone():
    from tensornetworks_amd import _ext
    with open(os.path.join(REPO, "include", "bornvi.h")) as f:
        limits, _, protos = _ext.parse_header(f.read())
    assert _ext.LIMITS == limits and _ext.PROTOTYPES == protos and _ext.EXPORTED_SYMBOLS == tuple(protos)
    assert len(_ext.PROTOTYPES) == 99
    assert not any("twosite" in k.lower() for k in list(_ext.LIMITS) + list(_ext.PROTOTYPES))
    assert _ext.TWOSITE_LIMITS == {"BORNVI_MPS_TWOSITE_MAX_BOND": 16, "BORNVI_MPS_TWOSITE_MAX_BATCH": 1 << 20,
                                   "BORNVI_MPS_TWOSITE_MAX_STEPS": 64}
    assert list(_ext.TWOSITE_PROTOTYPES) == ["bornvi_mps_twosite_workspace_bytes", "bornvi_mps_twosite_sweep"]
    res, args = _ext.TWOSITE_PROTOTYPES["bornvi_mps_twosite_sweep"]
    assert res is _ext.C.c_int and len(args) == 19 and args[7] is _ext.C.c_double and args[10] is _ext.C.c_double
    lib = _ext.lib()
    for name in _ext.TWOSITE_PROTOTYPES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _ext.TWOSITE_PROTOTYPES[name][1]


def test_python_argument_errors_need_no_device():
    from tensornetworks_amd import backend
    from tensornetworks_amd._ext import BornviError
    from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference
    from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine
    c = torch.as_tensor(tm.product_state(4, 2))
    idx = torch.zeros(5, dtype=torch.int64)
    ok = dict(w=None, lr=0.1, steps=2, bond_dim_keep=None, cutoff=0.0)
    bad = [dict(steps=0), dict(steps=65), dict(steps=True), dict(steps=1.0), dict(lr=-1e-3), dict(lr=float("nan")), dict(lr=float("inf")),
           dict(cutoff=-1e-9), dict(cutoff=1.0), dict(cutoff=float("nan")), dict(bond_dim_keep=0), dict(bond_dim_keep=3),
           dict(bond_dim_keep=True), dict(w=torch.ones(4, dtype=torch.float64)), dict(w=torch.ones(5, dtype=torch.float32)), dict(w=[0.2] * 5)]
    for change in bad:
        with pytest.raises(BornviError):
            backend.mps_twosite_sweep(c, idx, **{**ok, **change})
    for cores, samples in ((torch.zeros(1, 2, 2, 2, dtype=torch.float64), idx), (torch.zeros(4, 2, 17, 17, dtype=torch.float64), idx),
                           (c.to(torch.float32), idx), (c, idx.to(torch.int32)), (c, torch.zeros(0, dtype=torch.int64)),
                           (c, torch.zeros(2, 3, dtype=torch.int64)), (c[:, :, :, :1], idx), (c.numpy(), idx)):
        with pytest.raises(BornviError):
            backend.mps_twosite_sweep(cores, samples, **ok)
    # the machine and the trainer raise ValueError, before any device call
    bm = SampledMPSBornMachine(4, bond_dim=2, init_method="zero")
    for kw in (dict(lr=-0.1), dict(lr="0.1"), dict(steps=0), dict(steps=65), dict(cutoff=1.0), dict(cutoff=-1.0), dict(max_rank=3), dict(max_rank=0),
               dict(weights=torch.ones(4)), dict(weights=-torch.ones(5))):
        with pytest.raises(ValueError):
            bm.two_site_sweep_(idx, **{**dict(lr=0.1, steps=2, cutoff=0.0), **kw})
    for samples in (torch.full((5,), 16, dtype=torch.int64), torch.full((5,), -1, dtype=torch.int64), torch.zeros(5), torch.full((5, 4), 2),
                    torch.zeros(5, 3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            bm.two_site_sweep_(samples, lr=0.1, steps=2, cutoff=0.0)
    for sweeps in (0, True, 1.5):
        with pytest.raises(ValueError):
            bm.fit_two_site(idx, sweeps)
    with pytest.raises(ValueError):
        SampledMPSBornMachine(4, bond_dim=17, init_method="zero").two_site_sweep_(idx, lr=0.1, steps=2, cutoff=0.0)
    with pytest.raises(ValueError):
        SampledMPSBornMachine(1, bond_dim=2, init_method="zero").two_site_sweep_(torch.zeros(5, dtype=torch.int64), lr=0.1, steps=2, cutoff=0.0)
    bn, sites = tm.chain_network(4, 0)
    vi = AmortisedMPSInference(bn, sites[:2], sites[2:], {'bond_dim': 2, 'num_samples': 64, 'seed': 1, 'init_method': 'zero'})
    for args in ((0, 0.1), (2, -0.1), (True, 0.1)):
        with pytest.raises(ValueError):
            vi.train_two_site(*args, verbose=False)
    for kw in (dict(descent_steps=0), dict(cutoff=1.0), dict(max_rank=3)):
        with pytest.raises(ValueError):
            vi.train_two_site(2, 0.1, verbose=False, **kw)
