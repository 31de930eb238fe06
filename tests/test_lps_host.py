"""Host checks of the locally purified sampled MPS, no device: the fifth header and its binding, the
Python argument checks, the matrix-core lane maps the score kernel relies on (a NumPy model of v_mfma_f64_16x16x4_f64), and the
mirror's mathematics (tests/lps_mirror.py): brute force over (z, mu), central differences, the real family at m = 1, from_real
and from_complex through the other mirrors, and the joint-draw rule's marginal."""
import os

import numpy as np
import pytest
import torch

import cmps_mirror as cx
import hp_reference as hp
import lps_mirror as lp
import mps_sampled_mirror as sm
from conftest import REPO
from tensornetworks_amd._ext import LPS_LIMITS          # the fifth header's table: every test of this module needs the new family

# the mirror's geometry (its derived counts use it) is the header's and the kernel file's
assert (lp.TILE, lp.MAX_WG_SMALL, lp.MAX_WG_LARGE) == (LPS_LIMITS["BORNVI_LPS_SCORE_TILE"], LPS_LIMITS["BORNVI_LPS_MAX_WG_SMALL"],
                                                       LPS_LIMITS["BORNVI_LPS_MAX_WG_LARGE"])


random_cores = lp.random_cores
FREQ_SEED = lp.FREQ_SEED


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_parses_into_tables_of_its_own():
    from tensornetworks_amd import _ext, backend
    C = _ext.C
    with open(os.path.join(REPO, "include", "bornvi_lps.h")) as f:
        limits, enums, protos = _ext.parse_header(f.read())
    assert _ext.LPS_LIMITS == limits and enums == {}
    assert limits == {"BORNVI_LPS_MAX_BOND": 16, "BORNVI_LPS_MAX_PURIFICATION": 4, "BORNVI_LPS_SCORE_TILE": 16,
                      "BORNVI_LPS_MAX_WG_SMALL": 1024, "BORNVI_LPS_MAX_WG_LARGE": 256}
    assert (lp.TILE, lp.MAX_WG_SMALL, lp.MAX_WG_LARGE) == (16, 1024, 256)
    with open(os.path.join(REPO, "tensornetworks_amd", "csrc", "kernels_lps.hip")) as f:
        assert f"constexpr int LP_WAVES = {lp.WAVES};" in f.read()
    assert _ext.LPS_PROTOTYPES == protos
    assert list(protos) == ["bornvi_lps_workspace_bytes", "bornvi_lps_environments", "bornvi_lps_sample", "bornvi_lps_score_vjp"]
    assert backend.LPS_MAX_BOND == 16 and backend.LPS_MAX_PURIFICATION == 4
    # the other four headers' tables do not know the family
    others = (_ext.LIMITS, _ext.PROTOTYPES, _ext.TWOSITE_LIMITS, _ext.TWOSITE_PROTOTYPES, _ext.CMPS_LIMITS, _ext.CMPS_PROTOTYPES,
              _ext.MMD_LIMITS, _ext.MMD_PROTOTYPES)
    assert not any("lps" in k.lower() for table in others for k in table)
    p = C.c_void_p
    assert protos["bornvi_lps_workspace_bytes"] == (C.c_size_t, [p, C.c_int, C.c_int, C.c_int, C.c_longlong])
    assert protos["bornvi_lps_environments"] == (C.c_int, [p, C.c_int, C.c_int, C.c_int, C.c_longlong, p, p, p, C.c_size_t, p])
    assert protos["bornvi_lps_sample"] == (C.c_int, [p, C.c_int, C.c_int, C.c_int, C.c_longlong, p, C.c_ulonglong, p, p, p, p, p, C.c_size_t, p])
    assert protos["bornvi_lps_score_vjp"] == (C.c_int, [p, C.c_int, C.c_int, C.c_int, C.c_longlong, p, p, p, p, p, p, p, C.c_size_t, p])
    lib = _ext.lib()
    for name, (res, args) in protos.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype is res


def test_conventions_are_stated_in_the_same_words():
    """The parameter layout, the definitions, the rescaling rule and the gradient: the same lines in the header, the kernel
    file and the mirror (comment markers and indentation aside)."""
    def words(path, strip):
        with open(path) as f:
            return " ".join(" ".join(line.strip().lstrip(strip).split()) for line in f)
    texts = [words(os.path.join(REPO, "include", "bornvi_lps.h"), "*/ "),
             words(os.path.join(REPO, "tensornetworks_amd", "csrc", "kernels_lps.hip"), "/ "),
             words(os.path.join(REPO, "tests", "lps_mirror.py"), " ")]
    for phrase in ("psi(z, mu) = e0^T A_1[z_1, mu_1] ... A_n[z_n, mu_n] e0.",
                   "T(z) = sum_{mu_1 .. mu_n} psi(z, mu)^2.",
                   "rho_k = sum_mu A_k[z_k, mu]^T rho_{k-1} A_k[z_k, mu]",
                   "R_{k-1} = sum_mu A_k[z_k, mu] R_k A_k[z_k, mu]^T.",
                   "E_{k-1} = sum_{s,mu} A_k[s, mu] E_k A_k[s, mu]^T;",
                   "(2 w_b / T_b) rho_{b,k-1} A_k[z_{b,k}, mu] R_{b,k}.",
                   "(sum_b w_b) 2 L_{k-1} A_k[s, mu] E_k / Z."):
        assert all(phrase in t for t in texts), phrase
    for phrase in ("e the ilogb of its largest magnitude",):
        assert all(phrase in t for t in texts[:2]), phrase


# ---- argument errors, before any GPU call --------------------------------------------------------------------------------
def test_constructor_and_refused_methods():
    from tensornetworks_amd import ComplexSampledMPSBornMachine, PurifiedSampledMPSBornMachine
    from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine
    for kw in (dict(bond_dim=17), dict(bond_dim=0), dict(bond_dim=True), dict(bond_dim=2.0), dict(purification_dim=0), dict(purification_dim=5),
               dict(purification_dim=True), dict(purification_dim=2.0), dict(num_latent_vars=0), dict(num_latent_vars=64),
               dict(num_latent_vars=True), dict(num_latent_vars=4.0), dict(init_method="ones"), dict(conditioning_dim=1), dict(seed=1.5),
               dict(seed=True)):
        with pytest.raises(ValueError):
            PurifiedSampledMPSBornMachine(**{**dict(num_latent_vars=4, bond_dim=2), **kw})
    bm = PurifiedSampledMPSBornMachine(4, bond_dim=3, purification_dim=2, init_method="zero")
    assert tuple(bm.cores.shape) == (4, 2, 2, 3, 3) and bm.cores.dtype == torch.float64
    assert bm.num_parameters == 4 * 2 * 2 * 3 * 3 and bm.bond_dim == 3 and bm.purification_dim == 2
    assert PurifiedSampledMPSBornMachine(3).purification_dim == 2 and PurifiedSampledMPSBornMachine(3).bond_dim == 4
    idx = torch.zeros(5, dtype=torch.int64)
    calls = {"bond_spectrum": (), "bond_entropies": (), "canonical_cores": (), "canonicalise_": (), "compress_": (2,), "expand_": (4,),
             "two_site_sweep_": (idx,), "fit_two_site": (idx, 2), "marginals": (), "pair_marginals": (), "log_marginal": ({0: 1},),
             "log_marginal_vjp": ({0: 1}, torch.ones(1)), "sample_given": ({0: 1}, 4)}
    assert set(calls) == set(PurifiedSampledMPSBornMachine.REFUSED) == set(ComplexSampledMPSBornMachine.REFUSED)
    for name, args in calls.items():
        with pytest.raises(ValueError, match="SampledMPSBornMachine"):
            getattr(bm, name)(*args)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError):
            bm.sample_indices(bad)
    with pytest.raises(ValueError):
        bm.sample(4, x_condition=torch.zeros(1))
    with pytest.raises(ValueError):
        PurifiedSampledMPSBornMachine(21, bond_dim=2, init_method="zero").probabilities64()
    # the three initialisations: 'zero' is the exactly uniform q, 'small_random' draws the real family's cores first
    T, q = lp.brute_force(bm.cores.detach().numpy())
    assert np.all(hp.to_f64(q) == 1.0 / 16)
    torch.manual_seed(11)
    real = SampledMPSBornMachine(5, bond_dim=3)
    torch.manual_seed(11)
    pur = PurifiedSampledMPSBornMachine(5, bond_dim=3, purification_dim=3)
    c = pur.cores.detach()
    assert torch.equal(c[:, :, 0], real.cores.detach()) and float(c[:, :, 1:].abs().max()) > 0
    assert abs(float(c[:, :, 1:].std()) - 0.1 / np.sqrt(2.0)) < 0.02
    torch.manual_seed(3)
    rnd = PurifiedSampledMPSBornMachine(20, bond_dim=8, purification_dim=4, init_method="random")
    assert abs(float((rnd.cores.detach() ** 2).sum(2).mean()) - 1.0 / 16) < 0.003          # sum_mu E A^2 = 1 / (2 D)
    with pytest.raises(ValueError):
        PurifiedSampledMPSBornMachine.from_real(SampledMPSBornMachine(3, bond_dim=17, init_method="zero"))
    with pytest.raises(ValueError):
        PurifiedSampledMPSBornMachine.from_real(bm)
    with pytest.raises(ValueError):
        PurifiedSampledMPSBornMachine.from_real(real, purification_dim=5)
    with pytest.raises(ValueError):
        PurifiedSampledMPSBornMachine.from_complex(ComplexSampledMPSBornMachine(3, bond_dim=9, init_method="zero"))
    with pytest.raises(ValueError):
        PurifiedSampledMPSBornMachine.from_complex(real)


def test_backend_argument_errors():
    from tensornetworks_amd import backend
    from tensornetworks_amd._ext import BornviError
    c = torch.as_tensor(random_cores(4, 2, 2, 0))
    ep = torch.zeros(1, dtype=torch.int64)
    idx = torch.zeros(5, dtype=torch.int64)
    w = torch.ones(5, dtype=torch.float64)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    bad_cores = (z(4, 2, 2, 17, 17), z(4, 2, 2, 0, 0), z(4, 2, 0, 2, 2), z(4, 2, 5, 2, 2), z(64, 2, 2, 2, 2), z(0, 2, 2, 2, 2), z(4, 2, 2, 2),
                 z(4, 2, 2, 2, 3), z(4, 3, 2, 2, 2), c.to(torch.float32), c[..., :1].expand(4, 2, 2, 2, 2), c.numpy())
    for cores in bad_cores:
        with pytest.raises(BornviError):
            backend.lps_environments(cores, 8)
        with pytest.raises(BornviError):
            backend.lps_sample(cores, 8, 0, ep)
        with pytest.raises(BornviError):
            backend.lps_score_vjp(cores, idx, w)
        with pytest.raises(BornviError):
            backend.lps_score_vjp(cores, idx, out=False)
    for B in (0, -1, (1 << 24) + 1, True, 2.0):
        with pytest.raises(BornviError):
            backend.lps_environments(c, B)
        with pytest.raises(BornviError):
            backend.lps_sample(c, B, 0, ep)
    for seed, epoch in ((1.5, ep), (True, ep), (0, 3), (0, torch.zeros(2, dtype=torch.int64)), (0, torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(BornviError):
            backend.lps_sample(c, 8, seed, epoch)
    for i, ww in ((idx.to(torch.int32), w), (torch.zeros(2, 3, dtype=torch.int64), w), (torch.zeros(0, dtype=torch.int64), w[:0]),
                  (idx, w[:4]), (idx, w.to(torch.float32)), (idx, [1.0] * 5), (idx.numpy(), w), (idx, None)):
        with pytest.raises(BornviError):
            backend.lps_score_vjp(c, i, ww)
    for kw in (dict(out=z(4, 2, 2, 2)), dict(out_logq=z(4)), dict(status=torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(BornviError):
            backend.lps_score_vjp(c, idx, w, **kw)
    with pytest.raises(BornviError):
        backend.lps_sample(c, 8, 0, ep, out_aux=torch.zeros(8, dtype=torch.int64))


def test_trainer_configuration_errors():
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference, SampledMMDTrainer, PurifiedSampledMPSBornMachine
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(4, 0)
    for cfg in ({'purification_dim': 2}, {'cores': 'real', 'purification_dim': 2}, {'cores': 'complex', 'purification_dim': 1},
                {'cores': 'purified', 'purification_dim': 0}, {'cores': 'purified', 'purification_dim': 5},
                {'cores': 'purified', 'purification_dim': True}, {'cores': 'purified', 'purification_dim': 2.0},
                {'cores': 'purified', 'bond_dim': 17}, {'cores': 'purified', 'bond_dim': 0}, {'cores': 'purest'}):
        for make in (lambda c: SampledELBOVariationalInference(bn, lat, obs, c), lambda c: SampledKSDVariationalInference(bn, lat, obs, c),
                     lambda c: SampledMMDTrainer(4, c)):
            with pytest.raises(ValueError):
                make(dict(cfg))
    for ng in ('block', 'sample', 'cg'):
        with pytest.raises(ValueError, match="purified"):
            SampledELBOVariationalInference(bn, lat, obs, {'cores': 'purified'}, natural_gradient=ng)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'cores': 'purified', 'purification_dim': 3, 'bond_dim': 2})
    assert type(vi.born_machine) is PurifiedSampledMPSBornMachine and tuple(vi.born_machine.cores.shape) == (4, 2, 3, 2, 2)
    assert SampledMMDTrainer(4, {'cores': 'purified'}).born_machine.purification_dim == 2


# ---- the matrix-core lane maps --------------------------------------------------------------------------------------------
def mfma_16x16x4(a, b, c):
    """v_mfma_f64_16x16x4_f64 on lane values: a [64] is A[l & 15][l >> 4] (16 x 4), b [64] is B[l >> 4][l & 15] (4 x 16), c
    [4, 64] holds D[(l >> 4) + 4 reg][l & 15] in register reg.  Returns the new accumulator registers [4, 64]."""
    l = np.arange(64)
    A = np.zeros((16, 4)); A[l & 15, l >> 4] = a
    B = np.zeros((4, 16)); B[l >> 4, l & 15] = b
    Cm = np.zeros((16, 16))
    for reg in range(4):
        Cm[(l >> 4) + 4 * reg, l & 15] = c[reg]
    Dm = A @ B + Cm
    return np.stack([Dm[(l >> 4) + 4 * reg, l & 15] for reg in range(4)])


def tile_of(X):
    l = np.arange(64)
    return np.stack([X[4 * j + (l >> 4), l & 15] for j in range(4)])


def matrix_of(t):
    l = np.arange(64)
    X = np.zeros((16, 16))
    for j in range(4):
        X[4 * j + (l >> 4), l & 15] = t[j]
    return X


def mma(a, b, c):
    for j in range(4):
        c = mfma_16x16x4(a[j], b[j], c)
    return c


def test_lane_maps_of_the_density_steps():
    """The score kernel's three uses of an accumulator tile as an operand, on a NumPy model of the instruction's lane maps:
    register j of a tile is the B operand of K-step j, and for a symmetric tile also the A operand; the values a[j], aT[j] read
    from LDS serve the products the kernel's head comment lists."""
    rng = np.random.default_rng(5)
    D = 16
    A = rng.standard_normal((D, D))
    S = rng.standard_normal((D, D)); rho = S @ S.T
    S = rng.standard_normal((D, D)); R = S @ S.T
    l = np.arange(64)
    a = np.stack([A[4 * j + (l >> 4), l & 15] for j in range(4)])
    aT = np.stack([A[l & 15, 4 * j + (l >> 4)] for j in range(4)])
    zero = np.zeros((4, 64))
    Y = mma(tile_of(rho), a, zero)                       # rho A
    np.testing.assert_allclose(matrix_of(Y), rho @ A, rtol=0, atol=1e-12)
    nxt = mma(a, Y, zero)                                # A^T (rho A)
    np.testing.assert_allclose(matrix_of(nxt), A.T @ rho @ A, rtol=0, atol=1e-11)
    V = mma(tile_of(R), aT, zero)                        # R A^T
    np.testing.assert_allclose(matrix_of(V), R @ A.T, rtol=0, atol=1e-12)
    Rn = mma(aT, V, zero)                                # A (R A^T)
    np.testing.assert_allclose(matrix_of(Rn), A @ R @ A.T, rtol=0, atol=1e-11)
    W = mma(aT, tile_of(R), zero)                        # A R
    np.testing.assert_allclose(matrix_of(W), A @ R, rtol=0, atol=1e-12)
    G = mma(0.37 * tile_of(rho), W, zero)                # c rho (A R)
    np.testing.assert_allclose(matrix_of(G), 0.37 * rho @ A @ R, rtol=0, atol=1e-10)
    # with an unsymmetric tile the A-operand use computes with the transpose: the recursion the kernel states
    X = rng.standard_normal((D, D))
    np.testing.assert_allclose(matrix_of(mma(tile_of(X), a, zero)), X.T @ A, rtol=0, atol=1e-12)


# ---- the mirror's mathematics ----------------------------------------------------------------------------------------------
def test_brute_force_normalisation_and_densities():
    """sum_z q = 1 by brute force over (z, mu); the density sweep and the environments give the same T and Z."""
    for n, m, D in ((3, 2, 2), (4, 2, 3), (2, 4, 2), (3, 3, 1)):
        cores = random_cores(n, m, D, 7 * n + m)
        T, q = lp.brute_force(cores)
        assert abs(float(q.sum()) - 1.0) <= 4 * hp.EPS64
        env = lp.environments(cores)
        d = lp.densities(cores, lp.all_bits(n))
        assert np.all(np.abs(d["T"] - T) <= 64 * hp.EPS64 * d["T_abs"])
        assert abs(float(env["Z"] - T.sum())) <= 64 * hp.EPS64 * float(env["Z_abs"])
        assert np.all(np.abs(d["R"][0][:, 0, 0] - T) <= 64 * hp.EPS64 * d["T_abs"])           # the right sweep ends at the same T
        assert abs(float(env["L"][n][0, 0] - env["Z"])) <= 64 * hp.EPS64 * float(env["Z_abs"])
        lq = lp.logq_of(cores, lp.all_bits(n), env)["logq"]
        assert np.all(np.abs(hp.to_f64(np.exp(lq) - q)) <= 1e-15)


def test_gradient_against_central_differences():
    """Every entry at (n, m, D) = (4, 2, 3): the mirror's gradient, float64 torch autograd of its restatement, and central
    differences of sum_b w_b log q(z_b) in extended precision."""
    n, m, D = 4, 2, 3
    cores = random_cores(n, m, D, 4)
    rng = np.random.default_rng(9)
    bits = lp.all_bits(n)[rng.permutation(16)[:11]]
    w = rng.standard_normal(len(bits))
    ref = lp.score_gradient(cores, bits, w)
    auto = lp.autograd_score(cores, bits, w)
    assert np.all(np.abs(auto - hp.to_f64(ref["grad"])) <= 1e-12 * (1 + np.abs(auto)))

    def f(c):
        return float((lp.logq_of(c, bits)["logq"] * w.astype(lp.LD)).sum())
    h = 1e-6
    worst = 0.0
    for i in np.ndindex(cores.shape):
        up, dn = cores.copy(), cores.copy()
        up[i] += h
        dn[i] -= h
        fd = (f(up) - f(dn)) / (2 * h)
        worst = max(worst, abs(fd - float(ref["grad"][i])))
    print(f"worst |central difference - mirror| over {cores.size} entries: {worst:.2e}")
    assert worst <= 5e-8
    # entries of the first and last core that do not enter psi
    g = hp.to_f64(ref["grad"])
    assert np.all(g[0][:, :, 1:] == 0.0) and np.all(g[n - 1][:, :, :, 1:] == 0.0)


def test_m_equal_one_is_the_real_family():
    n, D, B = 6, 3, 40
    rng = np.random.default_rng(3)
    real = (np.eye(D) + 0.3 * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0)
    cores = real[:, :, None]
    bits = rng.integers(0, 2, size=(B, n))
    w = rng.standard_normal(B)
    a, b = sm.score_gradient(real, bits, w), lp.score_gradient(cores, bits, w)
    assert np.all(np.abs(hp.to_f64(a["logq"] - b["logq"])) <= 1e-15)
    assert np.all(np.abs(hp.to_f64(a["grad"] - b["grad"][:, :, 0])) <= 64 * hp.EPS64 * hp.to_f64(a["grad_abs"]))
    # the density majorant is the vector one times psi_abs / |psi| >= 1 per sample: never below it
    assert np.all(hp.to_f64(b["grad_abs"][:, :, 0]) >= (1 - 1e-12) * hp.to_f64(a["grad_abs"]))
    sa, sb = sm.sample(real, 5, 2, 300), lp.sample(cores, 5, 2, 300)
    assert sa["undecided"] == 0 and sb["undecided"] == 0 and np.array_equal(sa["idx"], sb["idx"]) and not sb["mus"].any()


def test_from_real_and_from_complex_keep_q():
    from tensornetworks_amd import ComplexSampledMPSBornMachine, PurifiedSampledMPSBornMachine
    from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine
    n, D = 5, 3
    torch.manual_seed(2)
    comp = ComplexSampledMPSBornMachine(n, bond_dim=D, init_method="random", seed=9)
    pur = PurifiedSampledMPSBornMachine.from_complex(comp)
    assert tuple(pur.cores.shape) == (n, 2, 2, 2 * D, 2 * D) and pur.seed == 9
    c = pur.cores.detach().numpy()
    assert not c[:n - 1, :, 1].any() and c[n - 1, :, 1].any() and not c[n - 1, :, 1, :, 1:].any()
    bits = lp.all_bits(n)
    want = cx.conditionals(comp.cores.detach().numpy(), bits)["logq"]
    res = lp.logq_of(c, bits)
    got, tol = res["logq"], 1e-16 * hp.to_f64(res["kappa"])      # (a state reached through cancellation carries kappa rounding errors)
    print(f"from_complex: worst |log q difference| {float(np.abs(got - want).max()):.2e}")
    assert np.all(np.abs(hp.to_f64(got - want)) <= tol)
    T, q = lp.brute_force(c)
    assert np.all(np.abs(hp.to_f64(np.log(q) - want)) <= tol)
    torch.manual_seed(4)
    real = SampledMPSBornMachine(n, bond_dim=D, init_method="random", seed=6)
    for m in (1, 3):
        pr = PurifiedSampledMPSBornMachine.from_real(real, purification_dim=m)
        cr = pr.cores.detach()
        assert tuple(cr.shape) == (n, 2, m, D, D) and torch.equal(cr[:, :, 0], real.cores.detach()) and not bool(cr[:, :, 1:].any()) and pr.seed == 6
        want = sm.conditionals(real.cores.detach().numpy(), bits)["logq"]
        got = lp.logq_of(cr.numpy(), bits)                 # (a state reached through cancellation carries kappa = T_abs / T rounding errors)
        assert np.all(np.abs(hp.to_f64(got["logq"] - want)) <= 1e-16 * hp.to_f64(got["kappa"]))


def test_joint_draw_rule_sums_to_the_marginal():
    """sum_mu P(z, mu) = q(z) at n = 3: the pure-state conditionals m_{s,mu} / M chain to psi(z, mu)^2 / Z."""
    for m, D in ((2, 3), (3, 2)):
        cores = random_cores(3, m, D, 11 + m)
        P = lp.joint_probabilities(cores)
        _, q = lp.brute_force(cores)
        assert np.all(np.abs(hp.to_f64(P.sum(axis=1) - q)) <= 1e-15)
        assert abs(float(P.sum()) - 1.0) <= 1e-15


def test_mirror_sampler_frequencies():
    """The GPU frequency test's CPU half: at (4, 2, 3, 2^16) the mirror's own sampler, with the seed the GPU test uses, lies
    within 5 standard errors of the exact q on each of the 16 outcomes; decide() follows the rule's words on a hand case."""
    z, mu, und = lp.decide(np.array([[[1.0, 2.0, 1.0], [3.0, 0.5, 0.5]]] * 4), np.array([0.1, 0.45, 0.5, 0.95]))
    assert list(z) == [0, 0, 1, 1] and list(mu) == [0, 2, 0, 2] and und == 1            # U M = 0.8, 3.6, 4.0 (on M0 = 4), 7.6
    n, m, D, B = 4, 2, 3, 1 << 16
    cores = random_cores(n, m, D, 21)
    s = lp.sample(cores, FREQ_SEED, 0, B, dtype=np.float64)
    _, q = lp.brute_force(cores)
    q = hp.to_f64(q)
    freq = np.bincount(s["idx"], minlength=16) / B
    zs = np.abs(freq - q) / np.sqrt(q * (1 - q) / B)
    print(f"mirror sampler: worst |freq - q| / standard error = {zs.max():.2f}")
    assert zs.max() <= 5.0
    assert np.array_equal(lp.mus_of_aux(s["aux"], n), s["mus"]) and s["mus"].max() == 1



def test_mirror_gradient_estimate_is_unbiased():
    """The GPU estimator test's CPU half: the mean of 64 epochs' estimates from the mirror's sampler lies within 5 standard
    errors of the exact reverse-KL gradient (n = 3, D = 2, m = 2, B = 1024)."""
    from tensornetworks_amd.bayesian_network import pack_network, synthetic_network
    n, m, D, B = 3, 2, 2, 1024
    bn, lat, obs, x = synthetic_network(n, 0)
    packed = pack_network(bn, lat, x)
    cores = random_cores(n, m, D, 31)
    weights = lp.elbo_weights(packed)
    est = []
    for e in range(64):
        s = lp.sample(cores, 21, e, B, dtype=np.float64)
        lq = hp.to_f64(lp.logq_of(cores, s["bits"], dtype=np.float64)["logq"])
        _, w = weights(s["idx"], s["bits"], lq)
        est.append(hp.to_f64(lp.score_gradient(cores, s["bits"], w, dtype=np.float64)["grad"]))
    est = np.stack(est)
    mean, se = est.mean(axis=0), est.std(axis=0, ddof=1) / np.sqrt(64)
    exact = hp.to_f64(lp.exact_elbo_gradient(cores, lp.log_joint(packed, lp.all_bits(n))))
    zs = np.abs(mean - exact) / np.where(se > 0, se, 1)
    print(f"mirror estimator: worst |mean - exact| / standard error = {zs.max():.2f}")
    assert np.all(np.abs(mean - exact) <= 5 * se + 1e-15)
