"""AmortisedMPSInference.train_two_site and SampledMPSBornMachine.fit_two_site / two_site_sweep_ on the GPU.

Sprinkler (4 sites) and the 10-variable chain, from the product state (init_method 'zero': identity matrices over sqrt 2) at cap
8: the device run against the mirror's replay on the mirrored draws (amortised_mirror.bn_sample with (seed, sweep); per sweep
mps_canon_mirror.canonicalise, then mps_twosite_mirror.sweep; between the calls the cores are float64, as on the device).
Bounds: per sweep e (counted from 1) the losses in units of loss_scale, hp.measured_constant(r64, derived), r64 what the float64
replay shows against the extended one and derived = e (mps_twosite_mirror.derived_constant + mps_canon_mirror.derived_constant):
the sweeps' errors add.  Ranks must equal the extended replay's; that the float64 replay's equal them too is asserted as a
condition on the inputs.

The chain's settings (B = 4096 fresh draws a sweep, lr 0.03, 5 steps, 3 sweeps, seed 1) are ones at which the MIRROR meets the
host test's condition (test_mps_twosite_host.check_chain_condition); the device result is held to the same condition."""
import functools

import numpy as np
import pytest
import torch

import amortised_mirror as am
import hp_reference as hp
import mps_canon_mirror as cm
import mps_twosite_mirror as tm
from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference
from tensornetworks_amd.bayesian_network import get_sprinkler_network
from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine
from test_mps_twosite_host import check_chain_condition

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
CAP = 8
RUNS = {"sprinkler": dict(B=1000, lr=0.05, steps=3, sweeps=2, seed=3),
        "chain": dict(B=4096, lr=0.03, steps=5, sweeps=3, seed=1)}


def network(name):
    if name == "sprinkler":
        return get_sprinkler_network(False), ['C', 'S', 'R'], ['W']
    bn, sites = tm.chain_network(10, 0)
    return bn, sites[:9], sites[9:]


def make(name, bond_dim=CAP, init_method='zero'):
    bn, lat, obs = network(name)
    S = RUNS[name]
    return AmortisedMPSInference(bn, lat, obs, {'bond_dim': bond_dim, 'num_samples': S["B"], 'seed': S["seed"], 'init_method': init_method},
                                 device='cuda')


@functools.lru_cache(maxsize=None)
def device_run(name, cutoff):
    vi = make(name)
    S = RUNS[name]
    draws = []
    hist = vi.train_two_site(S["sweeps"], S["lr"], descent_steps=S["steps"], cutoff=cutoff, verbose=False,
                             sweep_callback=lambda e, v: draws.append(v.last_idx.cpu().numpy().copy()))
    return vi, hist, draws


@functools.lru_cache(maxsize=None)
def replay(name, cutoff, extended):
    """The mirror's run: per sweep dict(idx, report), and the final cores."""
    vi = make(name)
    S = RUNS[name]
    n = vi.num_sites
    dtype = tm.LD if extended else np.float64
    c = vi.born_machine.cores.detach().cpu().numpy().copy()
    out = []
    for e in range(S["sweeps"]):
        idx = am.bn_sample(vi._packed, n, S["seed"], e, S["B"])["idx"].astype(np.int64)
        c = hp.to_f64(cm.canonicalise(c, dtype=dtype)["cores_out"])
        r = tm.sweep(c, idx, lr=S["lr"], steps=S["steps"], cutoff=cutoff, dtype=dtype)
        c = hp.to_f64(r["cores"])
        out.append(dict(idx=idx, report=r))
    return out, c


@pytest.mark.parametrize("name", ["sprinkler", "chain"])
def test_train_two_site_matches_the_mirrors_replay(name):
    cutoff = 1e-4
    vi, hist, draws = device_run(name, cutoff)
    r64, _ = replay(name, cutoff, False)
    rld, _ = replay(name, cutoff, True)
    n, S = vi.num_sites, RUNS[name]
    assert len(hist["loss"]) == S["sweeps"] and all(len(b) == 2 * (n - 1) for b in hist["bond_loss"])
    per = tm.derived_constant(n, CAP, S["steps"]) + cm.derived_constant(n, CAP)
    for e in range(S["sweeps"]):
        assert np.array_equal(draws[e], rld[e]["idx"])                      # the mirrored draws
        a, b = r64[e]["report"], rld[e]["report"]
        assert hist["status"][e] == 0 and b["status"] == 0
        assert np.array_equal(a["rank"], b["rank"])                          # a condition on the inputs: both mirrors cut alike
        scale = b["loss_scale"]
        own = float((np.abs(a["loss"].astype(tm.LD) - b["loss"]) / scale).max() / tm.LD(EPS))
        Cl = hp.measured_constant(own, (e + 1) * per)
        err = float((np.abs(np.asarray(hist["bond_loss"][e]).astype(tm.LD) - b["loss"]) / scale).max() / tm.LD(EPS))
        print(f"{name} sweep {e}: loss {hist['loss'][e]:.6f}, ranks {hist['rank'][e]}; bond losses off by {err:.1f} EPS64 of their scale "
              f"(C {Cl:.0f}, float64 replay {own:.1f})")
        assert err <= Cl
        assert hist["rank"][e] == b["rank"].tolist()
        assert hist["loss"][e] == hist["bond_loss"][e][-1]
        assert float(np.abs(np.asarray(hist["discarded"][e]) - hp.to_f64(b["discarded"])).max()) <= Cl * EPS


def test_chain_ranks_follow_the_data_on_the_device():
    vi_cut, hist_cut, _ = device_run("chain", 1e-4)
    vi_full, hist_full, _ = device_run("chain", 0.0)
    kl_cut, kl_full = vi_cut.exact_forward_kl(), vi_full.exact_forward_kl()
    _, c_cut = replay("chain", 1e-4, False)
    _, c_full = replay("chain", 0.0, False)
    p = vi_cut.site_joint_table().numpy()
    print(f"cutoff 1e-4: ranks {hist_cut['rank'][-1]}, KL {kl_cut:.5f};  cutoff 0: ranks {hist_full['rank'][-1]}, KL {kl_full:.5f};  "
          f"mirror KL {tm.forward_kl(c_cut, p):.5f} and {tm.forward_kl(c_full, p):.5f}")
    check_chain_condition(hist_cut["rank"][-1], kl_cut, kl_full, CAP)


def test_fit_two_site_is_two_site_sweep_in_a_loop():
    n, D, B = 6, 4, 300
    data = torch.as_tensor(np.random.default_rng(5).integers(0, 2, (B, n)))
    a = SampledMPSBornMachine(n, bond_dim=D, init_method='zero').to('cuda')
    b = SampledMPSBornMachine(n, bond_dim=D, init_method='zero').to('cuda')
    hist = a.fit_two_site(data, 3, lr=0.05, steps=2, cutoff=1e-5, max_rank=3)
    idx = b.indices_of(data)
    reports = [b.two_site_sweep_(idx, lr=0.05, steps=2, cutoff=1e-5, max_rank=3) for _ in range(3)]
    assert torch.equal(a.cores.detach(), b.cores.detach())
    assert hist["bond_loss"] == [r["loss"].cpu().tolist() for r in reports]
    assert hist["rank"] == [r["rank"].cpu().tolist() for r in reports] and max(max(r) for r in hist["rank"]) <= 3
    assert hist["status"] == [0, 0, 0] and np.isfinite(hist["loss"]).all()


def test_train_then_sweeps_then_train():
    torch.manual_seed(11)
    vi = make("sprinkler", bond_dim=4, init_method='small_random')
    h1 = vi.train(3, 0.02, verbose=False)
    h2 = vi.train_two_site(2, 0.05, descent_steps=3, verbose=False)
    h3 = vi.train(3, 0.02, verbose=False)
    assert all(np.isfinite(h["loss"]).all() for h in (h1, h2, h3)) and h2["status"] == [0, 0]
    assert tuple(vi.born_machine.cores.shape) == (4, 2, 4, 4)
    m = vi.posterior_marginals({'W': 1})
    assert list(m) == ['C', 'S', 'R'] and all(0.0 <= v <= 1.0 for v in m.values())
    assert np.isfinite(vi.log_evidence({'W': 1}))
