"""Host checks of the complex sampled MPS, no device: the third header and its binding, the Python
argument checks, the mirror's mathematics (tests/cmps_mirror.py) against central differences, against the real family's mirror
at zero imaginary parts, and from_statevector through the mirror."""
import os

import numpy as np
import pytest
import torch

import cmps_mirror as cx
import hp_reference as hp
import mps_sampled_mirror as sm
from conftest import REPO


def random_cores(n, D, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    c = spread * rng.standard_normal((n, 2, D, D, 2))
    c[..., 0] += np.eye(D)
    return c / np.sqrt(2.0)


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_parses_into_tables_of_its_own():
    from tensornetworks_amd import _ext, backend
    C = _ext.C
    with open(os.path.join(REPO, "include", "bornvi_cmps.h")) as f:
        limits, enums, protos = _ext.parse_header(f.read())
    assert _ext.CMPS_LIMITS == limits == {"BORNVI_CMPS_MAX_BOND": 16} and enums == {}
    assert _ext.CMPS_PROTOTYPES == protos
    assert list(protos) == ["bornvi_cmps_workspace_bytes", "bornvi_cmps_environments", "bornvi_cmps_sample", "bornvi_cmps_score_vjp"]
    assert backend.CMPS_MAX_BOND == 16
    # bornvi.h's and bornvi_twosite.h's tables do not know the family
    assert not any("cmps" in k.lower() for k in list(_ext.LIMITS) + list(_ext.PROTOTYPES) + list(_ext.TWOSITE_LIMITS) + list(_ext.TWOSITE_PROTOTYPES))
    p = C.c_void_p
    assert protos["bornvi_cmps_workspace_bytes"] == (C.c_size_t, [p, C.c_int, C.c_int, C.c_longlong])
    assert protos["bornvi_cmps_environments"] == (C.c_int, [p, C.c_int, C.c_int, C.c_longlong, p, p, p, C.c_size_t, p])
    assert protos["bornvi_cmps_sample"] == (C.c_int, [p, C.c_int, C.c_int, C.c_longlong, p, C.c_ulonglong, p, p, p, p, p, C.c_size_t, p])
    assert protos["bornvi_cmps_score_vjp"] == (C.c_int, [p, C.c_int, C.c_int, C.c_longlong, p, p, p, p, p, p, p, C.c_size_t, p])
    lib = _ext.lib()
    for name, (res, args) in protos.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype is res


# ---- argument errors, before any GPU call --------------------------------------------------------------------------------
def test_constructor_and_refused_methods():
    from tensornetworks_amd import ComplexSampledMPSBornMachine
    from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine
    for kw in (dict(bond_dim=17), dict(bond_dim=0), dict(bond_dim=True), dict(bond_dim=2.0), dict(num_latent_vars=0), dict(num_latent_vars=64),
               dict(num_latent_vars=True), dict(init_method="ones"), dict(conditioning_dim=1), dict(seed=1.5), dict(seed=True)):
        with pytest.raises(ValueError):
            ComplexSampledMPSBornMachine(**{**dict(num_latent_vars=4, bond_dim=2), **kw})
    bm = ComplexSampledMPSBornMachine(4, bond_dim=3, init_method="zero")
    assert tuple(bm.cores.shape) == (4, 2, 3, 3, 2) and bm.cores.dtype == torch.float64
    assert bm.num_parameters == 4 * 2 * 3 * 3 * 2 and bm.bond_dim == 3
    assert bm.complex_cores.dtype == torch.complex128 and tuple(bm.complex_cores.shape) == (4, 2, 3, 3)
    assert not isinstance(bm, __import__("tensornetworks_amd.born_machine_base", fromlist=["MPSCores"]).MPSCores)
    idx = torch.zeros(5, dtype=torch.int64)
    calls = {"bond_spectrum": (), "bond_entropies": (), "canonical_cores": (), "canonicalise_": (), "compress_": (2,), "expand_": (4,),
             "two_site_sweep_": (idx,), "fit_two_site": (idx, 2), "marginals": (), "pair_marginals": (), "log_marginal": ({0: 1},),
             "log_marginal_vjp": ({0: 1}, torch.ones(1)), "sample_given": ({0: 1}, 4)}
    assert set(calls) == set(ComplexSampledMPSBornMachine.REFUSED)
    for name, args in calls.items():
        with pytest.raises(ValueError, match="SampledMPSBornMachine"):
            getattr(bm, name)(*args)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError):
            bm.sample_indices(bad)
    with pytest.raises(ValueError):
        bm.sample(4, x_condition=torch.zeros(1))
    with pytest.raises(ValueError):
        ComplexSampledMPSBornMachine(21, bond_dim=2, init_method="zero").probabilities64()
    # the three initialisations: 'zero' is the uniform q, 'small_random' draws the real family's real parts first
    q = np.exp(hp.to_f64(cx.conditionals(bm.cores.detach().numpy(), cx.all_bits(4))["logq"]))
    assert np.all(q == 1.0 / 16)
    torch.manual_seed(11)
    real = SampledMPSBornMachine(5, bond_dim=3)
    torch.manual_seed(11)
    comp = ComplexSampledMPSBornMachine(5, bond_dim=3)
    assert torch.equal(comp.cores.detach()[..., 0], real.cores.detach()) and float(comp.cores.detach()[..., 1].abs().max()) > 0
    assert abs(float(comp.cores.detach()[..., 1].std()) - 0.1 / np.sqrt(2.0)) < 0.02
    torch.manual_seed(3)
    rnd = ComplexSampledMPSBornMachine(20, bond_dim=8, init_method="random")
    assert abs(float((rnd.cores.detach() ** 2).sum(-1).mean()) - 1.0 / 16) < 0.003          # E|A|^2 = 1 / (2 D), split between the parts
    # from_real
    back = ComplexSampledMPSBornMachine.from_real(real)
    assert torch.equal(back.cores.detach()[..., 0], real.cores.detach()) and bool((back.cores.detach()[..., 1] == 0).all()) and back.seed == real.seed
    with pytest.raises(ValueError):
        ComplexSampledMPSBornMachine.from_real(SampledMPSBornMachine(3, bond_dim=17, init_method="zero"))
    with pytest.raises(ValueError):
        ComplexSampledMPSBornMachine.from_real(bm)


def test_backend_argument_errors():
    from tensornetworks_amd import backend
    from tensornetworks_amd._ext import BornviError
    c = torch.as_tensor(random_cores(4, 2, 0))
    ep = torch.zeros(1, dtype=torch.int64)
    idx = torch.zeros(5, dtype=torch.int64)
    w = torch.ones(5, dtype=torch.float64)
    bad_cores = (torch.zeros(4, 2, 17, 17, 2, dtype=torch.float64), torch.zeros(64, 2, 2, 2, 2, dtype=torch.float64),
                 torch.zeros(0, 2, 2, 2, 2, dtype=torch.float64), torch.zeros(4, 2, 2, 2, dtype=torch.float64),
                 torch.zeros(4, 2, 2, 3, 2, dtype=torch.float64), torch.zeros(4, 3, 2, 2, 2, dtype=torch.float64),
                 torch.zeros(4, 2, 2, 2, 3, dtype=torch.float64), c.to(torch.float32), c[..., :1].expand(4, 2, 2, 2, 2), c.numpy(),
                 torch.view_as_complex(c))
    for cores in bad_cores:
        with pytest.raises(BornviError):
            backend.cmps_environments(cores, 8)
        with pytest.raises(BornviError):
            backend.cmps_sample(cores, 8, 0, ep)
        with pytest.raises(BornviError):
            backend.cmps_score_vjp(cores, idx, w)
    for B in (0, -1, (1 << 24) + 1, True, 2.0):
        with pytest.raises(BornviError):
            backend.cmps_environments(c, B)
        with pytest.raises(BornviError):
            backend.cmps_sample(c, B, 0, ep)
    for seed, epoch in ((1.5, ep), (True, ep), (0, 3), (0, torch.zeros(2, dtype=torch.int64)), (0, torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(BornviError):
            backend.cmps_sample(c, 8, seed, epoch)
    for i, ww in ((idx.to(torch.int32), w), (torch.zeros(2, 3, dtype=torch.int64), w), (torch.zeros(0, dtype=torch.int64), w[:0]),
                  (idx, w[:4]), (idx, w.to(torch.float32)), (idx, [1.0] * 5), (idx.numpy(), w)):
        with pytest.raises(BornviError):
            backend.cmps_score_vjp(c, i, ww)
    for kw in (dict(out=torch.zeros(4, 2, 2, 2, dtype=torch.float64)), dict(out_logq=torch.zeros(4, dtype=torch.float64)),
               dict(status=torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(BornviError):
            backend.cmps_score_vjp(c, idx, w, **kw)


def test_trainer_argument_errors():
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    from tensornetworks_amd.born_machine_cmps_sampled import ComplexSampledMPSBornMachine
    from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine
    bn = get_sprinkler_network(False)
    lat, obs = ['C', 'S', 'R'], ['W']
    for cls in (SampledELBOVariationalInference, SampledKSDVariationalInference):
        cfg = {'bond_dim': 2, 'num_samples': 64, 'seed': 1}
        assert type(cls(bn, lat, obs, cfg).born_machine) is SampledMPSBornMachine
        assert type(cls(bn, lat, obs, {**cfg, 'cores': 'real'}).born_machine) is SampledMPSBornMachine
        vi = cls(bn, lat, obs, {**cfg, 'cores': 'complex'})
        assert type(vi.born_machine) is ComplexSampledMPSBornMachine and tuple(vi.born_machine.cores.shape) == (3, 2, 2, 2, 2)
        for kind in ('imaginary', 'Complex', None, 1):
            with pytest.raises(ValueError):
                cls(bn, lat, obs, {**cfg, 'cores': kind})
        for ng in ('site', 'sample', 'cg'):
            with pytest.raises(ValueError, match="complex"):
                cls(bn, lat, obs, {**cfg, 'cores': 'complex'}, natural_gradient=ng)
        with pytest.raises(ValueError):
            cls(bn, lat, obs, {**cfg, 'cores': 'complex', 'bond_dim': 17})


# ---- the mirror's mathematics --------------------------------------------------------------------------------------------
def test_gradient_against_central_differences_and_normalisation():
    n, D, B = 4, 3, 24
    cores = random_cores(n, D, 5)
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2, size=(B, n))
    w = rng.standard_normal(B)
    allb = cx.all_bits(n)
    q = np.exp(cx.conditionals(cores, allb)["logq"])
    assert abs(float(q.sum()) - 1.0) <= 1e-15
    got = hp.to_f64(cx.score_gradient(cores, bits, w)["grad"])

    def f(c):
        return float((cx.conditionals(c, bits)["logq"] * w).sum())
    h = 1e-5 if hp.HAVE_LONGDOUBLE else 1e-6
    fd = np.zeros_like(cores)
    for i in np.ndindex(cores.shape):
        cp, cm_ = cores.copy(), cores.copy()
        cp[i] += h
        cm_[i] -= h
        fd[i] = (f(cp) - f(cm_)) / (2 * h)
    err = float(np.abs(got - fd).max())
    print(f"central differences (n, D) = ({n}, {D}): worst error {err:.2e}")
    assert err <= 1e-7
    # torch autograd on the real view takes the same gradient
    assert np.abs(got - cx.autograd_score(cores, bits, w)).max() <= 1e-12
    # entries of the first and last core that do not enter psi
    assert np.all(got[0][:, 1:] == 0.0) and np.all(got[n - 1][:, :, 1:] == 0.0)
    # the exact ELBO gradient is the derivative of sum_z q (log q - log p)
    logp = np.log(rng.dirichlet(np.ones(1 << n)))
    ge = hp.to_f64(cx.exact_elbo_gradient(cores, logp))

    def F(c):
        lq = cx.conditionals(c, allb)["logq"]
        return float((np.exp(lq) * (lq - logp)).sum())
    for i in [(0, 0, 0, 1, 0), (1, 1, 2, 0, 1), (3, 0, 1, 0, 1), (2, 1, 1, 1, 0)]:
        cp, cm_ = cores.copy(), cores.copy()
        cp[i] += h
        cm_[i] -= h
        assert abs((F(cp) - F(cm_)) / (2 * h) - ge[i]) <= 1e-7


def test_zero_imaginary_parts_are_the_real_family():
    n, D, B = 5, 3, 40
    rng = np.random.default_rng(8)
    real = (np.eye(D) + 0.3 * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0)
    cores = np.stack((real, np.zeros_like(real)), axis=-1)
    bits = rng.integers(0, 2, size=(B, n))
    w = rng.standard_normal(B)
    cr, cc = sm.conditionals(real, bits), cx.conditionals(cores, bits)
    assert np.all(cc["psi"].imag == 0) and np.array_equal(cc["psi"].real, cr["psi"])
    assert np.array_equal(cc["logq"], cr["logq"]) and np.array_equal(cc["p1"], cr["p1"])
    gr, gc = sm.score_gradient(real, bits, w), cx.score_gradient(cores, bits, w)
    assert np.all(gc["grad"][..., 1] == 0.0)
    # the real half: the same sums with E_k^T for E_k (equal as matrices, other bits): a few roundings of the mirror's arithmetic
    unit = float(np.finfo(cx.LD).eps)
    assert np.all(np.abs(gc["grad"][..., 0] - gr["grad"]) <= 64 * unit * gr["grad_abs"])
    assert np.array_equal(cx.sample(cores, 3, 1, 64)["idx"], sm.sample(real, 3, 1, 64)["idx"])


# ---- from_statevector ------------------------------------------------------------------------------------------------------
def random_state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)


def amplitudes(machine):
    n = machine.num_latent_vars
    return cx.conditionals(machine.cores.detach().numpy(), cx.all_bits(n))["psi"]


@pytest.mark.parametrize("n,D", [(8, 16), (3, 2), (1, 1)])
def test_from_statevector_is_exact_at_full_bond(n, D):
    from tensornetworks_amd import ComplexSampledMPSBornMachine
    psi = random_state(n, 40 + n)
    bm, discarded = ComplexSampledMPSBornMachine.from_statevector(torch.as_tensor(psi), D)
    assert tuple(bm.cores.shape) == (n, 2, D, D, 2) and tuple(discarded.shape) == (n - 1,) and bool((discarded <= 1e-28).all())
    got = amplitudes(bm)
    err = float(np.abs(got - psi).max())
    print(f"from_statevector n={n} D={D}: worst amplitude error {err:.2e}")
    assert err <= 1e-13
    # a real vector is taken too
    bm2, _ = ComplexSampledMPSBornMachine.from_statevector(torch.as_tensor(psi.real.copy()), D)
    assert float(np.abs(amplitudes(bm2) - psi.real).max()) <= 1e-13


def test_from_statevector_truncated_reports_the_tail_sums():
    from tensornetworks_amd import ComplexSampledMPSBornMachine
    n, D = 8, 4
    psi = random_state(n, 77)
    bm, discarded = ComplexSampledMPSBornMachine.from_statevector(torch.as_tensor(psi), D)
    # the same sequence of SVDs in NumPy: the tail sums past the D largest values
    rest = psi.reshape(1, -1)
    tails = []
    for k in range(n - 1):
        U, S, Vh = np.linalg.svd(rest.reshape(rest.shape[0] * 2, -1), full_matrices=False)
        tails.append(float((S[D:] ** 2).sum()))
        rest = S[:D, None] * Vh[:D]
    assert np.abs(discarded.numpy() - np.array(tails)).max() <= 1e-14
    assert discarded[0] == 0 and discarded[1] == 0 and float(discarded[3]) > 1e-3
    # the truncated state is that of the kept factors, and its squared distance is at most the sum of the tails
    err2 = float((np.abs(amplitudes(bm) - psi) ** 2).sum())
    assert 0 < err2 <= sum(tails) * (1 + 1e-12)
    # cutoff: more goes from the small end, from the first bond on (its two values are both kept without a cutoff)
    _, more = ComplexSampledMPSBornMachine.from_statevector(torch.as_tensor(psi), D, cutoff=0.6)
    assert 0 < float(more[0]) <= 0.6 and float(more.sum()) > float(discarded.sum())
    for args in ((torch.zeros(6), 2), (torch.zeros(1 << 17), 2), (torch.as_tensor(psi), 17), (torch.as_tensor(psi), 0), (torch.as_tensor(psi), True),
                 (torch.zeros(2, 4), 2), (torch.full((4,), float("nan")), 2), (torch.zeros(4, dtype=torch.int64), 2)):
        with pytest.raises(ValueError):
            ComplexSampledMPSBornMachine.from_statevector(*args)
    for cutoff in (-0.1, 1.0, True, "0"):
        with pytest.raises(ValueError):
            ComplexSampledMPSBornMachine.from_statevector(torch.as_tensor(psi), 4, cutoff=cutoff)
