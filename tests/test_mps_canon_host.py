"""The canonicaliser's mirror (mps_canon_mirror.py) against an independent route, and the host side of the Python surface
(MPSCores.expand_, the argument errors of bond_spectrum / canonical_cores / compress_ / expand_).  No GPU.

Bounds, units of EPS64 against 1 (Schmidt values are <= 1 and the normalised state has norm 1; the error of an orthogonal
change of gauge is norm-wise, it moves between entries, so no per-entry bound exists): mps_canon_mirror.derived_constant
for the float64 mirror; the extended mirror and LAPACK's SVD of the unfolded state, two references, differ by LAPACK's own
float64 error, which SVD_C = 8 max(2^k, 2^(n-k))^(1/2) <= 8 * 64 bounds generously at n <= 12."""
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_canon_mirror as cm
from tensornetworks_amd.born_machine_mps import MPSBornMachine
from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine

EPS = hp.EPS64
SHAPES = [(1, 1), (2, 2), (3, 5), (3, 17), (6, 8), (12, 3), (12, 16), (8, 32)]


def make_cores(n, D, seed=0, spread=0.3):
    gen = torch.Generator().manual_seed(7000 * n + 13 * D + seed)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    return ((eye + spread * torch.randn(n, 2, D, D, dtype=torch.float64, generator=gen)) / math.sqrt(2.0)).contiguous().numpy()


def svd_constant(n):
    return 8.0 * math.sqrt(2.0 ** (n // 2))


@pytest.mark.parametrize("n,D", SHAPES)
def test_mirror_schmidt_values_equal_the_unfolded_svd(n, D):
    cores = make_cores(n, D)
    r64 = cm.canonicalise(cores)
    rld = cm.canonicalise(cores, dtype=cm.LD)
    assert r64["status"] == 0 and rld["status"] == 0
    assert r64["sweeps"] < cm.MAX_SWEEPS and rld["sweeps"] < cm.MAX_SWEEPS
    if n == 1:
        assert r64["schmidt"].shape == (0, D)
        return
    svd = cm.unfolded_schmidt(cores)
    e64 = float(np.abs(r64["schmidt"] - svd).max()) / EPS
    eld = float(np.abs(hp.to_f64(rld["schmidt"]) - svd).max()) / EPS
    print(f"n={n} D={D}: sweeps {r64['sweeps']} / {rld['sweeps']}; |float64 mirror - svd| = {e64:.1f} EPS64, |extended mirror - svd| = {eld:.1f} EPS64")
    assert eld <= svd_constant(n)
    assert e64 <= cm.derived_constant(n, D) + svd_constant(n)
    # the squares of a bond sum to 1, the values descend, a bond holds at most min(2^k, 2^(n-k)) non-zero ones: exact zeros
    assert np.all(np.abs((r64["schmidt"] ** 2).sum(axis=1) - 1.0) <= 4 * D * EPS)
    assert np.all(np.diff(r64["schmidt"], axis=1) <= 0)
    for k in range(1, n):
        cap = min(2 ** k, 2 ** (n - k))
        assert np.all(r64["schmidt"][k - 1, cap:] == 0.0)
        assert r64["rank"][k - 1] <= cap


@pytest.mark.parametrize("n,D", SHAPES)
def test_mirror_keeps_psi_and_the_gauge(n, D):
    cores = make_cores(n, D)
    r = cm.canonicalise(cores)
    psi, Z = cm.psi_of(cores)
    out = hp.to_f64(r["cores_out"])
    psi_out, Z_out = cm.psi_of(out)
    C = cm.derived_constant(n, D)
    err = float(np.abs(psi_out - psi / np.sqrt(Z)).max()) / EPS
    print(f"n={n} D={D}: max |psi_out - psi / sqrt(Z)| = {err:.1f} EPS64 (C = {C:.0f}); Z_out - 1 = {float(Z_out - 1):.2e}")
    assert err <= C                                             # the sign is kept: + psi, not - psi
    assert abs(float(Z_out - 1)) <= 2 * C * EPS
    assert abs(float(r["log_norm"] - np.log(Z))) <= C * EPS * (1.0 + float(r["log_abs"]))
    assert np.all(out[0, :, 1:, :] == 0.0) and np.all(out[n - 1, :, :, 1:] == 0.0)
    for k in range(2, n + 1):
        rk = int(r["rank"][k - 2])
        gram = out[k - 1, 0] @ out[k - 1, 0].T + out[k - 1, 1] @ out[k - 1, 1].T
        assert np.abs(gram[:rk, :rk] - np.eye(rk)).max() <= C * EPS
        assert np.all(out[k - 1, :, rk:, :] == 0.0)


def test_mirror_truncates_where_it_says():
    """(10, 4 -> 2): the discarded weight is neither 0 nor of order 1, and the cut state is as far from the input as the
    discarded weights say: |psi_out - psi / sqrt(Z)|^2 <= 2 sum_k discarded_k (equality to first order)."""
    gen = torch.Generator().manual_seed(11)
    n, D = 10, 4
    cores = ((torch.eye(D, dtype=torch.float64) + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64, generator=gen)) / math.sqrt(2.0)).numpy()
    r = cm.canonicalise(cores, D_out=2)
    assert r["gap"] > 1e-6
    total = float(r["discarded"].sum())
    assert 1e-5 < total < 1e-1
    assert np.all(r["rank"] <= 2)
    psi, Z = cm.psi_of(cores)
    psi_out, _ = cm.psi_of(hp.to_f64(r["cores_out"]))
    d2 = float(((psi_out - psi / np.sqrt(Z)) ** 2).sum())
    print(f"discarded {total:.4e}, |psi_out - psi|^2 = {d2:.4e}")
    assert d2 <= 2 * total + cm.derived_constant(n, D) * EPS
    assert d2 >= 0.5 * total


@pytest.mark.parametrize("cls", [MPSBornMachine, SampledMPSBornMachine])
def test_expand_with_zero_noise_leaves_psi_bit_for_bit(cls):
    torch.manual_seed(3)
    bm = cls(6, bond_dim=3, init_method="random")
    before = bm.cores.detach().numpy().copy()
    old = bm.cores
    bm.expand_(7)
    assert bm.bond_dim == 7 and bm.cores is not old and isinstance(bm.cores, torch.nn.Parameter)
    assert tuple(bm.cores.shape) == (6, 2, 7, 7) and bm.cores.dtype == torch.float64
    after = bm.cores.detach().numpy()
    assert np.array_equal(after, cm.expand(before, 7))
    assert np.array_equal(hp.to_f64(cm.psi_of(after)[0]), hp.to_f64(cm.psi_of(before)[0]))
    assert list(bm.parameters())[0] is bm.cores and len(list(bm.parameters())) == 1


def test_expand_noise_fills_the_new_entries_only():
    torch.manual_seed(4)
    bm = SampledMPSBornMachine(5, bond_dim=2, init_method="random")
    before = bm.cores.detach().numpy().copy()
    bm.expand_(4, noise=1e-2, seed=9)
    after = bm.cores.detach().numpy()
    assert np.array_equal(after[:, :, :2, :2], before)
    assert np.array_equal(after, cm.expand(before, 4, 1e-2, 9))
    # the new entries of the first core's rows >= 1 and of the last core's columns >= 1 stay 0 (the old block is the model's own)
    assert np.all(after[0, :, 2:, :] == 0.0) and np.all(after[0, :, 1:, 2:] == 0.0) and np.all(after[0, :, 0, 2:] != 0.0)
    assert np.all(after[4, :, :, 2:] == 0.0) and np.all(after[4, :, 2:, 1:] == 0.0) and np.all(after[4, :, 2:, 0] != 0.0)
    assert np.all(after[1, :, 2:, :] != 0.0) and np.all(after[1, :, :, 2:] != 0.0)
    again = SampledMPSBornMachine(5, bond_dim=2, init_method="random")
    with torch.no_grad():
        again.cores.copy_(torch.from_numpy(before))
    again.expand_(4, noise=1e-2, seed=10)
    assert not np.array_equal(again.cores.detach().numpy(), after)


@pytest.mark.parametrize("cls", [MPSBornMachine, SampledMPSBornMachine])
def test_argument_errors_are_raised_on_the_host(cls, monkeypatch):
    from tensornetworks_amd import backend

    def no_gpu(*a, **k):
        raise AssertionError("an argument error must be raised before any GPU call")
    monkeypatch.setattr(backend, "mps_canonicalise", no_gpu)
    bm = cls(4, bond_dim=4)
    for bad in (0, 5, -1, True, 2.0, "2"):
        with pytest.raises(ValueError, match="bond_dim"):
            bm.canonical_cores(bond_dim=bad)
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError, match="bond_dim"):
            bm.compress_(bond_dim=bad)
    with pytest.raises(ValueError, match="current bond dimension"):
        bm.compress_(bond_dim=5)                                   # above the current D: not a compression (D itself is allowed)
    for bad in (-1e-9, float("nan"), float("inf"), True, "0", None):
        with pytest.raises(ValueError, match="cutoff"):
            bm.canonical_cores(cutoff=bad)
        with pytest.raises(ValueError, match="cutoff"):
            bm.compress_(cutoff=bad)
    for bad in (4, 3, 0, 33, True, 8.0, None):
        with pytest.raises(ValueError, match="bond_dim"):
            bm.expand_(bad)
    for bad in (-1.0, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="noise"):
            bm.expand_(8, noise=bad)
    for bad in (True, 1.5, None):
        with pytest.raises(ValueError, match="seed"):
            bm.expand_(8, seed=bad)
    assert bm.bond_dim == 4                                        # nothing was changed by a refused call


def test_tournament_meets_every_pair_once():
    for D in range(1, 33):
        rounds = cm.tournament(D)
        assert len(rounds) == (D - 1 if D % 2 == 0 else D)
        seen = [p for pr in rounds for p in pr]
        assert sorted(seen) == [(i, j) for i in range(D) for j in range(i + 1, D)]
        for pr in rounds:
            cols = [c for p in pr for c in p]
            assert len(cols) == len(set(cols)) and len(pr) <= D // 2
