"""Host checks of the MMD objective, no device: the fourth header and its binding, the spectral identity
of the mixture kernel, the algebra of the sampled estimator on the mirror (tests/mmd_mirror.py), and the argument errors of the
kernel class, the objective, the backend calls and the three trainers, all raised before any GPU call."""
import math
import os

import numpy as np
import pytest
import torch

import mmd_mirror as mm
from conftest import REPO


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_parses_into_tables_of_its_own():
    from tensornetworks_amd import _ext, backend
    C = _ext.C
    with open(os.path.join(REPO, "include", "bornvi_mmd.h")) as f:
        limits, enums, protos = _ext.parse_header(f.read())
    assert _ext.MMD_LIMITS == limits and enums == {} and _ext.MMD_PROTOTYPES == protos
    assert limits["BORNVI_HAMMING_PAIRS_MAX_A"] == 1 << 17 and limits["BORNVI_HAMMING_PAIRS_MAX_B"] == 1 << 20
    assert set(limits) == {"BORNVI_HAMMING_PAIRS_MAX_A", "BORNVI_HAMMING_PAIRS_MAX_B", "BORNVI_MMD_MAX_SCALES", "BORNVI_MMD_TILE_BITS",
                           "BORNVI_MMD_HIGH_BITS"}
    assert list(protos) == ["bornvi_mmd_passes", "bornvi_mmd_workspace_bytes", "bornvi_mmd_weights",
                            "bornvi_hamming_pairs_workspace_bytes", "bornvi_hamming_pairs_rowsum"]
    assert backend.HAMMING_PAIRS_MAX_A == 1 << 17 and backend.HAMMING_PAIRS_MAX_B == 1 << 20
    assert backend.MMD_TILE_BITS == limits["BORNVI_MMD_TILE_BITS"] and backend.MMD_HIGH_BITS == limits["BORNVI_MMD_HIGH_BITS"]
    # the other three headers' tables do not know the family
    others = (list(_ext.LIMITS) + list(_ext.PROTOTYPES) + list(_ext.TWOSITE_LIMITS) + list(_ext.TWOSITE_PROTOTYPES)
              + list(_ext.CMPS_LIMITS) + list(_ext.CMPS_PROTOTYPES))
    assert not any("mmd" in k.lower() or "hamming_pairs" in k.lower() for k in others)
    p = C.c_void_p
    assert protos["bornvi_mmd_passes"] == (C.c_int, [C.c_int])
    assert protos["bornvi_mmd_workspace_bytes"] == (C.c_size_t, [p, C.c_int])
    assert protos["bornvi_mmd_weights"] == (C.c_int, [p, C.c_int, p, p, p, p, p, p, C.c_size_t, p])
    assert protos["bornvi_hamming_pairs_workspace_bytes"] == (C.c_size_t, [p, C.c_int, C.c_longlong, C.c_longlong])
    assert protos["bornvi_hamming_pairs_rowsum"] == (C.c_int, [p, C.c_int, C.c_longlong, p, C.c_longlong, p, C.c_int, p, p, p, p, p,
                                                               C.c_size_t, p])
    lib = _ext.lib()
    for name, (res, args) in protos.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype is res


def test_pass_geometry_follows_the_tile_constants():
    """1, 3, 5 tile passes: one bit group of at most TILE_BITS low bits, then groups of at most HIGH_BITS."""
    from tensornetworks_amd import backend
    t, hb = backend.MMD_TILE_BITS, backend.MMD_HIGH_BITS
    for n in range(1, 31):
        groups = 1 + (max(0, n - t) + hb - 1) // hb
        assert backend.mmd_passes(n) == 2 * groups - 1, n
    assert _lib_passes(0) == 0 and _lib_passes(31) == 0
    for bad in (0, 31, 2.0):
        with pytest.raises(backend.BornviError):
            backend.mmd_passes(bad)


def _lib_passes(n):
    from tensornetworks_amd import _ext
    return _ext.lib().bornvi_mmd_passes(n)


# ---- the kernel and its spectrum -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 8])
@pytest.mark.parametrize("scales", [(1.0,), (0.25, 1.0, 4.0)])
def test_spectrum_identity(n, scales):
    """H K H / 2^n = diag(lam[popcount k]) to 1e-13 relative; the tables equal the mirror's longdouble ones rounded."""
    from tensornetworks_amd.hamming_kernel import HammingMixtureKernel
    k = HammingMixtureKernel(n, scales)
    assert k.kappa.dtype == np.float64 and k.kappa.shape == (n + 1,) and k.spectrum.shape == (n + 1,)
    kap_m, lam_m = mm.tables(n, scales)
    np.testing.assert_allclose(k.kappa, kap_m.astype(np.float64), rtol=4e-16)
    np.testing.assert_allclose(k.spectrum, lam_m.astype(np.float64), rtol=4e-16)
    assert np.all(k.spectrum > 0) and k.kappa[0] == 1.0
    K = k.dense().numpy()
    np.testing.assert_allclose(K, mm.dense_K(n, k.kappa), rtol=1e-14)
    H = mm.hadamard(n)
    D = H @ K @ H / 2.0 ** n
    want = np.diag(k.spectrum[mm.popcounts(n)])
    assert np.abs(D - want).max() <= 1e-13 * np.abs(want).max()
    assert math.isclose(k.spectrum[mm.popcounts(n)].sum() / 2.0 ** n, k.kappa[0], rel_tol=1e-14)


def test_one_length_scale_is_the_base_kernel():
    from tensornetworks_amd.hamming_kernel import HammingMixtureKernel
    from tensornetworks_amd.stein_utils import base_hamming_kernel_torch
    n = 6
    rng = np.random.default_rng(0)
    z1 = torch.from_numpy(rng.integers(0, 2, (9, n)).astype(np.float64))
    z2 = torch.from_numpy(rng.integers(0, 2, (9, n)).astype(np.float64))
    for l in (0.05, 1.0, 3.5):
        k = HammingMixtureKernel(n, (l,))
        assert torch.equal(k(z1, z2), base_hamming_kernel_torch(z1, z2, n, l))
        d = (z1 != z2).sum(dim=-1).numpy()
        np.testing.assert_allclose(k(z1, z2).numpy(), k.kappa[d], rtol=1e-14)      # (rho^d against exp(-d / (n l)): an exponent of up to 20)


def test_walsh_route_is_the_dense_product():
    """The mirror's two routes: w = 2 K d and L = d^T K d by the dense K and by two transforms."""
    from tensornetworks_amd.hamming_kernel import HammingMixtureKernel
    for n in (1, 5, 10):
        k = HammingMixtureKernel(n, (0.05, 1.0, 4.0))
        rng = np.random.default_rng(n)
        q = rng.random(1 << n)
        q /= q.sum()
        t = np.bincount(rng.integers(0, 1 << n, 50), minlength=1 << n) / 50.0
        K = mm.dense_K(n, k.kappa)
        d = q - t
        L, w = mm.weights(q, t, k.spectrum)
        np.testing.assert_allclose(w, 2.0 * K @ d, rtol=0, atol=1e-13 * np.abs(d).sum())
        assert math.isclose(L, d @ K @ d, rel_tol=1e-11)
        L0, w0 = mm.weights(q, None, k.spectrum)
        np.testing.assert_allclose(w0, 2.0 * K @ q, rtol=1e-12)


# ---- estimator algebra -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 7])
@pytest.mark.parametrize("N", [1, 5])
def test_estimator_algebra(B, N):
    from tensornetworks_amd.hamming_kernel import HammingMixtureKernel
    from tensornetworks_amd.mmd_objective import mmd_u_and_weights
    n = 5
    k = HammingMixtureKernel(n)
    rng = np.random.default_rng([B, N])
    z = rng.integers(0, 1 << n, B)
    z[-1] = z[0]                                   # duplicates on both sides
    y = rng.integers(0, 1 << n, N)
    if N > 1:
        y[-1] = y[0]
    assert np.array_equal(mm.pair_counts(z, y, n), mm.pair_counts_fast(z, y, n))
    assert np.array_equal(mm.pair_counts(z, z, n, True), mm.pair_counts_fast(z, z, n, True))
    U, w, rxx, rxy, Tyy = mm.sampled(z, y, n, k.kappa)
    assert abs(w.sum()) <= 16 * mm.EPS64 * np.abs(w).sum() + 1e-300
    assert math.isclose(U, mm.u_double_loop(z, y, n, k.kappa), rel_tol=1e-13, abs_tol=1e-15)
    perm = rng.permutation(N)
    U2, w2, _, rxy2, _ = mm.sampled(z, y[perm], n, k.kappa)
    assert np.array_equal(rxy2, rxy) and np.array_equal(w2, w) and math.isclose(U2, U, rel_tol=1e-14, abs_tol=1e-16)
    # the trainers' own expression on torch tensors is the mirror's
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    Ut, wt = mmd_u_and_weights(t(rxx), t(math.fsum(rxx)), t(rxy), t(math.fsum(rxy)), t(Tyy), B, N)
    np.testing.assert_allclose(wt.numpy(), w, rtol=1e-14, atol=1e-17)
    assert math.isclose(float(Ut), U, rel_tol=1e-14, abs_tol=1e-16)


def test_estimator_is_unbiased_for_the_enumerated_loss():
    """The mean of U over ALL B-tuples drawn from q (n = 2, B = 3: 64 tuples, weighted) is d^T K d."""
    from tensornetworks_amd.hamming_kernel import HammingMixtureKernel
    n, B = 2, 3
    k = HammingMixtureKernel(n)
    q = np.array([0.1, 0.4, 0.3, 0.2])
    y = np.array([0, 3, 3, 1, 2])
    p = np.bincount(y, minlength=4) / y.size
    L = (q - p) @ mm.dense_K(n, k.kappa) @ (q - p)
    mean = 0.0
    for a in range(4):
        for b in range(4):
            for c in range(4):
                mean += q[a] * q[b] * q[c] * mm.u_double_loop([a, b, c], y, n, k.kappa)
    assert math.isclose(mean, L, rel_tol=1e-12)


# ---- argument errors, before any GPU call --------------------------------------------------------------------------------
def test_kernel_and_objective_argument_errors():
    from tensornetworks_amd import HammingMixtureKernel, MMDObjective
    for kw in (dict(num_vars=0), dict(num_vars=64), dict(num_vars=True), dict(num_vars=2.0), dict(length_scales=()),
               dict(length_scales=(1.0,) * 9), dict(length_scales=(0.0,)), dict(length_scales=(-1.0,)), dict(length_scales=(float("inf"),)),
               dict(length_scales=(float("nan"),)), dict(length_scales=(True,)), dict(length_scales="ab")):
        with pytest.raises(ValueError):
            HammingMixtureKernel(**{**dict(num_vars=4), **kw})
        with pytest.raises(ValueError):
            MMDObjective(**{**dict(num_vars=4), **kw})
    k = HammingMixtureKernel(4, 2.0)
    assert k.length_scales == (2.0,)
    with pytest.raises(ValueError):
        k(torch.zeros(3, 5), torch.zeros(3, 5))
    obj = MMDObjective(4)
    for bad in (torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64), torch.tensor([16]), torch.tensor([-1]), torch.full((3, 4), 2),
                torch.zeros(3, 5, dtype=torch.int64), torch.full((3, 4), 0.5), torch.zeros(8), torch.full((16,), -1.0),
                torch.full((16,), float("nan")), torch.zeros(2, 2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            obj.prepare(bad)
    with pytest.raises(ValueError):
        MMDObjective(31).prepare(torch.zeros(8))          # a table beyond the enumerated limit
    with pytest.raises(ValueError):
        obj.weights(torch.zeros(16, dtype=torch.float64))
    with pytest.raises(ValueError):
        obj.sample_weights(torch.zeros(4, dtype=torch.int64))


def test_backend_argument_errors():
    from tensornetworks_amd import backend
    E = backend.BornviError
    q, lam = torch.zeros(16, dtype=torch.float64), torch.ones(5, dtype=torch.float64)
    for args, kw in (((q[:12], None, lam), {}), ((q, None, lam[:4]), {}), ((q.reshape(4, 4), None, lam), {}), ((q, q[:8], lam), {}),
                     ((q, None, lam), dict(want_w=False, out=q)), ((q[:1], None, lam[:1]), {}), (([0.0] * 16, None, lam), {}),
                     ((q, q.reshape(4, 4), lam), {}), ((q, None, lam), {})):        # (the last: not on a GPU)
        with pytest.raises(E):
            backend.mmd_weights(*args, **kw)
    z, kap = torch.zeros(4, dtype=torch.int64), torch.ones(5, dtype=torch.float64)
    for args in ((z[:0], z, kap), (z, z[:0], kap), (z, z, kap[:1]), (z, z, torch.ones(65, dtype=torch.float64)), (z.reshape(2, 2), z, kap),
                 (z, z.reshape(2, 2), kap), ([0, 1], z, kap), (z, z, kap)):
        with pytest.raises(E):
            backend.hamming_pairs_rowsum(*args)


def test_trainer_argument_errors():
    from tensornetworks_amd import ClassicalMMDTrainer, QuantumMMDTrainer, SampledMMDTrainer
    for kw in (dict(qbm_shots=100), dict(natural_gradient="diag"), dict(natural_gradient="quantum"), dict(length_scales=()),
               dict(length_scales=(0.0,)), dict(num_vars=0), dict(num_vars=31)):
        with pytest.raises(ValueError):
            QuantumMMDTrainer(**{**dict(num_vars=4, qbm_ansatz_layers=1), **kw})
    vi = QuantumMMDTrainer(4, 2, "basic")
    assert vi.observed_vars_names == [] and vi._loss_key == 'loss_mmd2' and vi.num_latent_vars == 4
    for bad in (torch.zeros(0, dtype=torch.int64), torch.tensor([16]), torch.full((3, 4), 2)):
        with pytest.raises(ValueError):
            vi.train(bad, 1, 0.1, verbose=False)
    for cfg in ({}, {'use_logits': False}, {'family': 'mps', 'bond_dim': 2}):
        cv = ClassicalMMDTrainer(4, cfg)
        assert cv._loss_key == 'loss_mmd2'
        with pytest.raises(ValueError):
            cv.train(torch.tensor([-1]), 1, 0.1, verbose=False)
    for bad in (dict(num_vars=0), dict(num_vars=31), dict(length_scales=(-1.0,)), dict(born_machine_config={'family': 'tree'}),
                dict(born_machine_config={'conditioning_dim': 1}), dict(born_machine_config={}, condition=[1.0])):
        with pytest.raises(ValueError):
            ClassicalMMDTrainer(**{**dict(num_vars=4, born_machine_config={}), **bad})
    for cfg in ({'num_samples': 2}, {'num_samples': (1 << 17) + 1}, {'num_samples': 64, 'cores': 'quaternion'}, {'num_samples': 64, 'rank': 2}):
        with pytest.raises(ValueError):
            SampledMMDTrainer(6, {'bond_dim': 2, **cfg})
    with pytest.raises(ValueError):
        SampledMMDTrainer(6, {'bond_dim': 2, 'num_samples': 64, 'cores': 'complex'}, natural_gradient='site')
    with pytest.raises(ValueError):
        SampledMMDTrainer(64, {'bond_dim': 2, 'num_samples': 64})
    sv = SampledMMDTrainer(6, {'bond_dim': 2, 'num_samples': 64})
    assert sv.LOSS_KEYS == ('loss_mmd2',) and sv.MIN_SAMPLES == 3 and sv.MAX_SAMPLES == 1 << 17
    for bad in (torch.zeros(0, dtype=torch.int64), torch.tensor([64]), torch.tensor([-3]), torch.full((3, 6), 2)):
        with pytest.raises(ValueError):
            sv.train(bad, 1, 0.1, verbose=False)
