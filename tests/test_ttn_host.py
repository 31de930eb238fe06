"""Host checks of the tree-tensor-network sampled Born machine, no device: the sixth header and its
binding, the Python argument checks, and the mirror's mathematics (tests/ttn_mirror.py): brute force, central differences, the
environments' Z, the sampler's conditionals and frequencies."""
import os

import numpy as np
import pytest
import torch

import hp_reference as hp
import ttn_mirror as tt
from conftest import REPO
from tensornetworks_amd._ext import TTN_LIMITS          # the sixth header's table: every test of this module needs the new family

assert tt.MAX_WG == TTN_LIMITS["BORNVI_TTN_MAX_WG"]

SHAPES = [(1, 2), (2, 2), (3, 2), (5, 3), (7, 3), (9, 2)]


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_parses_into_tables_of_its_own():
    from tensornetworks_amd import _ext, backend
    C = _ext.C
    with open(os.path.join(REPO, "include", "bornvi_ttn.h")) as f:
        limits, enums, protos = _ext.parse_header(f.read())
    assert _ext.TTN_LIMITS == limits and enums == {}
    assert limits == {"BORNVI_TTN_MAX_BOND": 8, "BORNVI_TTN_MAX_WG": 1024}
    with open(os.path.join(REPO, "tensornetworks_amd", "csrc", "ttn_dev.hpp")) as f:
        assert f"constexpr int TT_LANES = {tt.LANES};" in f.read()
    assert _ext.TTN_PROTOTYPES == protos and _ext.TTN_HEADER_PATH.endswith("bornvi_ttn.h")
    assert list(protos) == ["bornvi_ttn_workspace_bytes", "bornvi_ttn_environments", "bornvi_ttn_sample", "bornvi_ttn_score_vjp"]
    assert backend.TTN_MAX_BOND == 8
    others = (_ext.LIMITS, _ext.PROTOTYPES, _ext.TWOSITE_LIMITS, _ext.TWOSITE_PROTOTYPES, _ext.CMPS_LIMITS, _ext.CMPS_PROTOTYPES,
              _ext.MMD_LIMITS, _ext.MMD_PROTOTYPES, _ext.LPS_LIMITS, _ext.LPS_PROTOTYPES)
    assert not any("ttn" in k.lower() for table in others for k in table)
    p = C.c_void_p
    assert protos["bornvi_ttn_workspace_bytes"] == (C.c_size_t, [p, C.c_int, C.c_int, C.c_longlong])
    assert protos["bornvi_ttn_environments"] == (C.c_int, [p, C.c_int, C.c_int, C.c_longlong, p, p, p, C.c_size_t, p])
    assert protos["bornvi_ttn_sample"] == (C.c_int, [p, C.c_int, C.c_int, C.c_longlong, p, C.c_ulonglong, p, p, p, p, p, C.c_size_t, p])
    assert protos["bornvi_ttn_score_vjp"] == (C.c_int, [p, C.c_int, C.c_int, C.c_longlong, p, p, p, p, p, p, p, C.c_size_t, p])
    lib = _ext.lib()
    for name, (res, args) in protos.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype is res


def test_conventions_are_stated_in_the_same_words():
    """The tree, the parameter, the dead entries, the amplitude, the environments, the down vectors, the gradient and the sampler:
    the same lines in the header, the kernel file and the mirror (comment markers and indentation aside)."""
    def words(path, strip):
        with open(path) as f:
            return " ".join(" ".join(line.strip().lstrip(strip).split()) for line in f)
    texts = [words(os.path.join(REPO, "include", "bornvi_ttn.h"), "*/ "),
             words(os.path.join(REPO, "tensornetworks_amd", "csrc", "kernels_ttn.hip"), "/ "),
             words(os.path.join(REPO, "tests", "ttn_mirror.py"), " ")]
    for phrase in ("h = max(1, ceil(log2 n)), L = 2^h leaf positions, 1 <= n <= 63, so L <= 64.",
                   "z_{j+1}, bit n - 1 - j of the int64 outcome index, the real family's bit order.",
                   "Positions j >= n are padding and carry the fixed value 0.",
                   "Nodes are heap-numbered v = 1 .. L - 1, their children are 2 v and 2 v + 1; nodes v >= L / 2 are bottom nodes, "
                   "their children are the positions 2 (v - L / 2) and 2 (v - L / 2) + 1.",
                   "cores[v - 1] = T_v[p, a, b], p the parent bond, a, b the left and right child bonds.",
                   "Never read, and their gradient is exactly 0.0: the root at p >= 1; a bottom node at a >= 2 or b >= 2; a bottom "
                   "node at the value 1 of a padding child.",
                   "x_v[p] = sum_{a,b} T_v[p, a, b] x_{2v}[a] x_{2v+1}[b], contracted as M = T x_{2v} over a, then M x_{2v+1} over b;",
                   "psi(z) = x_1[0]; Z = sum_z psi(z)^2; q = psi^2 / Z.",
                   "V_{2v}[a, a'] = sum V_v[p, p'] T[p, a, b] T[p', a', b'] U_{2v+1}[b, b'], V_{2v+1} the same with U_{2v}.",
                   "dZ/dT_v[p, a, b] = 2 sum V_v[p, p'] T_v[p', a', b'] U_{2v}[a, a'] U_{2v+1}[b, b'].",
                   "y_1 = e0, y_{2v}[a] = sum y_v[p] T[p, a, b] x_{2v+1}[b], y_{2v+1}[b] = sum y_v[p] T[p, a, b] x_{2v}[a].",
                   "Block v receives sum_b (2 w_b / psi_b) y_{b,v} (x) x_{b,2v} (x) x_{b,2v+1} and loses (sum_b w_b) dZ/dT_v / Z.",
                   "P_{2v+1} = M^T P_v M; descend right; return x_v = M x_{2v+1}.",
                   "m_1 = P[1, 1] and draws z = [U (m_0 + m_1) >= m_0]; a padding position draws nothing and is 0.",
                   "bornvi_mps_sample's Philox4x32-10 uniform at (seed, epoch, b, k = j + 1)."):
        assert all(phrase in t for t in texts), phrase
    for phrase in ("e the ilogb of its largest magnitude", "a node's exponent is its own plus its children's"):
        assert all(phrase in t for t in texts[:2]), phrase


# ---- the mirror's mathematics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", SHAPES)
def test_q_sums_to_one_and_z_of_the_environments_is_brute_force(n, D):
    cores = tt.random_cores(n, D, 100 * n + D)
    T, q = tt.brute_force(cores, n)
    env = tt.environments(cores, n)
    assert abs(float(q.sum()) - 1.0) <= 4e-16
    assert abs(float(env["Z"] / T.sum()) - 1.0) <= 64 * float(np.finfo(tt.LD).eps)
    lq = tt.logq_of(cores, n, tt.all_bits(n), env)["logq"]
    assert np.all(np.abs(hp.to_f64(np.exp(lq) - q)) <= 1e-15)
    # dead entries are never read: any value there changes nothing
    noisy = np.where(tt.live_mask(n, D), cores, 7.5)
    assert np.array_equal(tt.brute_force(noisy, n)[0], T)


def test_gradient_agrees_with_central_differences_on_every_live_entry():
    n, D, B = 5, 3, 9
    cores = tt.random_cores(n, D, 41)
    rng = np.random.default_rng(8)
    bits = tt.bits_of_idx(rng.integers(0, 1 << n, B), n)
    w = rng.standard_normal(B)
    g = hp.to_f64(tt.score_gradient(cores, n, bits, w)["grad"])
    live = tt.live_mask(n, D)
    assert np.all(g[~live] == 0.0)

    def f(c):
        return (tt.logq_of(c, n, bits)["logq"] * w).sum()      # kept in the mirror's arithmetic: the difference below is of nearby numbers
    # the truncation error is eps^2 times a third derivative over 6, which is large where a sample's psi is small (here |psi| >= 6e-3)
    eps, worst = 1e-7, 0.0
    for at in zip(*np.nonzero(live)):
        cp, cm = cores.copy(), cores.copy()
        cp[at] += eps
        cm[at] -= eps
        worst = max(worst, abs(float((f(cp) - f(cm)) / (2 * eps)) - g[at]))
    print(f"central differences: worst error {worst:.2e}")
    assert worst <= 1e-7
    assert np.abs(tt.autograd_score(cores, n, bits, w) - g).max() <= 1e-12


def test_product_of_the_samplers_conditionals_is_q_for_every_z():
    n, D = 5, 3
    cores = tt.random_cores(n, D, 43)
    _, q = tt.brute_force(cores, n)
    p = tt.chain_probability(cores, n, tt.all_bits(n))
    assert np.abs(hp.to_f64(p / q - 1)).max() <= 4e-16 * 64


def test_mirror_sampler_frequencies_and_no_undecided_draw():
    """(5, 3, 2^16): the mirror's own sampler with FREQ_SEED lies within 3 standard errors of the exact q on every outcome."""
    n, D, B = 5, 3, 1 << 16
    cores = tt.random_cores(n, D, 21)
    _, q = tt.brute_force(cores, n)
    q = hp.to_f64(q)
    s = tt.sample(cores, n, tt.FREQ_SEED, 0, B, dtype=np.float64)
    assert s["undecided"] == 0
    freq = np.bincount(s["idx"], minlength=32) / B
    zs = np.abs(freq - q) / np.sqrt(q * (1 - q) / B)
    print(f"mirror sampler frequencies: worst |freq - q| / standard error = {zs.max():.2f}")
    assert zs.max() < 3.0
    assert np.abs(np.exp(s["logq"]) - q[s["idx"]]).max() <= 1e-13


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_zero_init_is_exactly_uniform(n):
    from tensornetworks_amd import TreeSampledBornMachine
    for D in (2, 3):
        bm = TreeSampledBornMachine(n, bond_dim=D, init_method="zero")
        c = bm.cores.detach().numpy()
        assert np.array_equal(c, tt.uniform_cores(n, D))
        T, q = tt.brute_force(c, n)
        assert np.all(hp.to_f64(q) == 1.0 / (1 << n))
        assert np.array_equal(bm.live_mask().numpy(), tt.live_mask(n, D)) and bm.num_parameters == int(tt.live_mask(n, D).sum())
        assert bm.tree_shape == tt.tree_shape(n) and tuple(bm.cores.shape) == (bm.tree_shape[1] - 1, D, D, D)


# ---- argument errors, before any GPU call --------------------------------------------------------------------------------
def test_constructor_and_refused_methods():
    from tensornetworks_amd import ComplexSampledMPSBornMachine, TreeSampledBornMachine
    for kw in (dict(bond_dim=1), dict(bond_dim=9), dict(bond_dim=True), dict(bond_dim=2.0), dict(num_latent_vars=0), dict(num_latent_vars=64),
               dict(num_latent_vars=True), dict(num_latent_vars=4.0), dict(init_method="ones"), dict(conditioning_dim=1), dict(seed=1.5),
               dict(seed=True)):
        with pytest.raises(ValueError):
            TreeSampledBornMachine(**{**dict(num_latent_vars=4, bond_dim=2), **kw})
    bm = TreeSampledBornMachine(5, bond_dim=3)
    assert tuple(bm.cores.shape) == (7, 3, 3, 3) and bm.cores.dtype == torch.float64 and bm.bond_dim == 3
    assert TreeSampledBornMachine(3).bond_dim == 4
    live = bm.live_mask()
    for method in ("small_random", "random"):
        c = TreeSampledBornMachine(5, bond_dim=3, init_method=method).cores.detach()
        assert torch.all(c[~live] == 0.0) and torch.all(c[live] != 0.0)
    idx = torch.zeros(5, dtype=torch.int64)
    calls = {"bond_spectrum": (), "bond_entropies": (), "canonical_cores": (), "canonicalise_": (), "compress_": (2,), "expand_": (4,),
             "two_site_sweep_": (idx,), "fit_two_site": (idx, 2), "marginals": (), "pair_marginals": (), "log_marginal": ({0: 1},),
             "log_marginal_vjp": ({0: 1}, torch.ones(1)), "sample_given": ({0: 1}, 4)}
    assert set(calls) == set(TreeSampledBornMachine.REFUSED) == set(ComplexSampledMPSBornMachine.REFUSED) and len(calls) == 13
    for name, args in calls.items():
        with pytest.raises(ValueError, match="SampledMPSBornMachine") as e:
            getattr(bm, name)(*args)
        assert "tree cores" in str(e.value)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError):
            bm.sample_indices(bad)
    with pytest.raises(ValueError):
        bm.sample(4, x_condition=torch.zeros(1))
    with pytest.raises(ValueError):
        TreeSampledBornMachine(21, bond_dim=2, init_method="zero").probabilities64()
    other = TreeSampledBornMachine._with_cores(bm.cores.detach(), seed=4, num_latent_vars=5)
    assert torch.equal(other.cores, bm.cores) and other.seed == 4 and other.num_latent_vars == 5
    with pytest.raises(ValueError):
        TreeSampledBornMachine._with_cores(bm.cores.detach(), num_latent_vars=9)


def test_backend_argument_errors():
    from tensornetworks_amd import backend
    from tensornetworks_amd._ext import BornviError
    good = torch.zeros(7, 3, 3, 3, dtype=torch.float64)
    ep = torch.zeros(1, dtype=torch.int64)
    for cores, n, B in ((good, 4, 8), (good, 9, 8), (torch.zeros(7, 9, 9, 9, dtype=torch.float64), 5, 8), (torch.zeros(7, 1, 1, 1, dtype=torch.float64), 5, 8),
                        (good, 0, 8), (good, 64, 8), (good, True, 8), (good, 5, 0), (good, 5, (1 << 24) + 1), (good[:, :, :, :2], 5, 8), (None, 5, 8)):
        with pytest.raises(BornviError):
            backend.ttn_environments(cores, n, B)
        with pytest.raises(BornviError):
            backend.ttn_sample(cores, n, B, 0, ep)
    with pytest.raises(BornviError):
        backend.ttn_score_vjp(good, 5, torch.zeros((2, 2), dtype=torch.int64), None, out=False)
    assert backend.ttn_tree_shape(1) == (1, 2) and backend.ttn_tree_shape(33) == (6, 64) and backend.ttn_tree_shape(63) == (6, 64)


def test_trainer_configuration():
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference, SampledMMDTrainer, sampled_trainer
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    from tensornetworks_amd.born_machine_ttn_sampled import TreeSampledBornMachine
    bn = get_sprinkler_network(False)
    lat, obs = ['C', 'S', 'R'], ['W']
    assert sampled_trainer.TREE_FAMILIES == {"tree": (TreeSampledBornMachine, ())} and sampled_trainer.ALL_FAMILIES["tree"][0] is TreeSampledBornMachine
    for cls in (SampledELBOVariationalInference, SampledKSDVariationalInference):
        vi = cls(bn, lat, obs, {"cores": "tree", "bond_dim": 2, "num_samples": 64, "seed": 3})
        assert isinstance(vi.born_machine, TreeSampledBornMachine) and vi.born_machine.bond_dim == 2 and vi.born_machine.seed == 3
        with pytest.raises(ValueError, match="tree cores"):
            cls(bn, lat, obs, {"cores": "tree", "bond_dim": 2}, natural_gradient="block")
        with pytest.raises(ValueError, match="'tree'"):
            cls(bn, lat, obs, {"cores": "forest"})
        for bad in (1, 9, True, 2.0):
            with pytest.raises(ValueError):
                cls(bn, lat, obs, {"cores": "tree", "bond_dim": bad})
        with pytest.raises(ValueError, match="purified"):
            cls(bn, lat, obs, {"cores": "tree", "purification_dim": 2})
    assert isinstance(SampledMMDTrainer(3, {"cores": "tree", "bond_dim": 2, "num_samples": 64}).born_machine, TreeSampledBornMachine)
