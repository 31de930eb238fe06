"""bornvi_bn_sample and bornvi_mps_log_marginals_vjp against the mirror (amortised_mirror.py) and their contract (DESIGN.md
section 6m).

bn_sample: idx is the mirror's for EVERY sample: the decision U (t0 + t1) >= t0 is one add, one multiply and one compare in
float64 on both sides, so no draw is left out.  logp: V logs of at most a unit each (relative to |log f|; two are allowed) and
V - 1 additions, against the sum of |log f|:  (V + 1) EPS logp_abs.

log_marginals_vjp, per entry, units of EPS64 (the rule of test_gpu_mps_sampled_kernel.py: every rounding a whole unit, the
power-of-two rescalings add none, first order in EPS), t_abs_j = 2 |c_j| (L_abs |A| E_abs)[entry] / m_j the term's magnitudes:
  C_ENV(n - 1) for L^_{k-1} and E^_k together (k - 1 and n - k clamped environment steps, C_ENV(j) = j (3 D + 1));
  2 D for the chains T_s = A_s E^_k and M_s = L^ T_s;  3 for c_j / m^_j, the product with it and the subnormal end of ldexp;
  C_ENV(n) kappa_c for the quotient's divisor m_j, kappa_c = m_abs / m the evidence's condition number;
  Q / G + G + 1 for the additions: the workgroup's queries in order, the G partials in order, the final subtraction;
  the normaliser's term the same with kappa_Z and sum_j |c_j|, its additions those of W (Q / G, then 12 for sum_partials) and
  the product with W:  Q / G + 14.
Q in {1, 3, G, G + 1, 2 G + 3} with G the geometry's cap (its value at Q = 2^16): one query per workgroup, then workgroups with
one and with two, then with two and with three.  The grid is min(Q, G) + 1, so no workgroup of it is without a query except
the last, which takes the empty mask alone.
amortised_mirror.log_marginal_gradient evaluates exactly this sum.  The constants are not fitted: each test prints the worst
ratio beside 1."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import amortised_mirror as am
import hp_reference as hp
import mps_query_mirror as qm
import mps_sampled_mirror as sm
from tensornetworks_amd import _ext, backend
from tensornetworks_amd.bayesian_network import (BayesianNetwork, get_sprinkler_network, pack_network, pack_network_for_sampling,
                                                synthetic_network)
from test_gpu_mps_sampled_kernel import c_score, make_cores

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
SEED = 20260
UNSUPPORTED = -4


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def t64(x):
    return torch.tensor(x, dtype=torch.int64, device=dev())


def row(p1):
    return {0: 1.0 - p1, 1: p1}


def six_node_network():
    """A -> H -> {B, C}, B -> D, {C, D} -> E; H is dropped and has two children."""
    rng = np.random.default_rng(61)
    bn = BayesianNetwork()
    tab = lambda k: {cfg: row(float(rng.uniform(0.05, 0.95))) for cfg in np.ndindex(*(2,) * k)}
    bn.add_node('A', cpt=tab(0))
    bn.add_node('H', cpt=tab(1), parent_names=['A'])
    bn.add_node('B', cpt=tab(1), parent_names=['H'])
    bn.add_node('C', cpt=tab(1), parent_names=['H'])
    bn.add_node('D', cpt=tab(1), parent_names=['B'])
    bn.add_node('E', cpt=tab(2), parent_names=['C', 'D'])
    return bn, ['E', 'A', 'B', 'C', 'D']


def deterministic_network():
    """Rows (0, 1) and (1, 0): B copies A, C negates B; the zero-probability value must never be drawn."""
    bn = BayesianNetwork()
    bn.add_node('A', cpt={(): {0: 0.3, 1: 0.7}})
    bn.add_node('B', cpt={(0,): {0: 1.0, 1: 0.0}, (1,): {0: 0.0, 1: 1.0}}, parent_names=['A'])
    bn.add_node('C', cpt={(0,): {0: 0.0, 1: 1.0}, (1,): {0: 1.0, 1: 0.0}}, parent_names=['B'])
    return bn, ['A', 'B', 'C']


def chain64():
    """64 nodes in a chain, the first dropped: n = 63, tuple position 0 is bit 62."""
    rng = np.random.default_rng(64)
    bn = BayesianNetwork()
    bn.add_node('N0', cpt={(): row(0.5)})
    for v in range(1, 64):
        bn.add_node(f'N{v}', cpt={(0,): row(float(rng.uniform(0.1, 0.9))), (1,): row(float(rng.uniform(0.1, 0.9)))},
                    parent_names=[f'N{v - 1}'])
    return bn, [f'N{v}' for v in range(1, 64)]


def networks():
    syn, zs, xs, _ = synthetic_network(5)
    return {"sprinkler": (get_sprinkler_network(False), ['C', 'S', 'R', 'W']), "synthetic5": (syn, zs + xs),
            "dropped": six_node_network(), "deterministic": deterministic_network(), "chain64": chain64()}


def draw(desc, n, B, epoch, seed=SEED):
    idx, logp, st = backend.bn_sample(desc, n, B, seed, t64([epoch]))
    return idx, logp, st


@pytest.mark.parametrize("name", ["sprinkler", "synthetic5", "dropped", "deterministic", "chain64"])
def test_bn_sample_against_the_mirror(name):
    bn, sites = networks()[name]
    n = len(sites)
    packed = pack_network_for_sampling(bn, sites)
    V = len(packed["role"])
    keep, desc = backend.bn_descriptor(packed, dev())
    ref = am.bn_sample(packed, n, SEED, 0, 1000)
    got = {}
    for B in (1, 64, 65, 1000):
        idx, logp, st = draw(desc, n, B, 0)
        assert int(st.item()) == 0
        gi, gl = idx.cpu().numpy(), logp.cpu().numpy()
        assert np.array_equal(gi, ref["idx"][:B].astype(np.int64)), B                  # every sample
        err = np.abs(hp.to_f64(gl.astype(sm.LD) - ref["logp"][:B]))
        assert np.all(err <= EPS * (V + 1) * hp.to_f64(ref["logp_abs"][:B])), B
        got[B] = (idx, logp)
    assert torch.equal(got[1000][0][:64], got[64][0]) and torch.equal(got[1000][1][:64], got[64][1])      # not a function of B
    again = draw(desc, n, 1000, 0)
    assert torch.equal(again[0], got[1000][0]) and torch.equal(again[1], got[1000][1])                    # two calls
    other = draw(desc, n, 1000, 1)
    assert not torch.equal(other[0], got[1000][0])                                                        # epoch 1 differs
    assert np.array_equal(other[0].cpu().numpy(), am.bn_sample(packed, n, SEED, 1, 1000)["idx"].astype(np.int64))
    bits = sm.bits_of_idx(got[1000][0].cpu().numpy(), n)
    if name == "deterministic":
        assert np.all(bits[:, 1] == bits[:, 0]) and np.all(bits[:, 2] == 1 - bits[:, 1])
        assert bool(torch.isfinite(got[1000][1]).all())
    if name == "chain64":
        assert 0 < int(bits[:, 0].sum()) < 1000 and np.all(got[1000][0].cpu().numpy() >= 0)               # bit 62 is used


def test_bn_sample_logp_is_the_log_joint_bit_for_bit():
    bn, sites = networks()["sprinkler"]
    keep, desc = backend.bn_descriptor(pack_network_for_sampling(bn, sites), dev())
    keep2, desc2 = backend.bn_descriptor(pack_network(bn, sites, {}), dev())
    idx, logp, _ = draw(desc, 4, 1000, 2)
    assert torch.equal(backend.bn_logjoint_samples(desc2, 4, idx), logp)


def test_bn_sample_dead_row():
    """A row whose two entries sum to 0 kills the sample that meets it: status 1, logp NaN; the others are untouched."""
    bn = BayesianNetwork()
    bn.add_node('A', cpt={(): row(0.5)})
    bn.add_node('B', cpt={(0,): row(0.25), (1,): {0: 0.0, 1: 0.0}}, parent_names=['A'])
    packed = pack_network_for_sampling(bn, ['A', 'B'])
    keep, desc = backend.bn_descriptor(packed, dev())
    idx, logp, st = draw(desc, 2, 257, 0)
    ref = am.bn_sample(packed, 2, SEED, 0, 257)
    assert int(st.item()) == 1 and ref["dead"].any() and not ref["dead"].all()
    assert np.array_equal(idx.cpu().numpy(), ref["idx"].astype(np.int64))
    assert np.array_equal(np.isnan(logp.cpu().numpy()), ref["dead"])


def test_bn_sample_refusals():
    lib = _ext.lib()
    h = _ext.handle_for(dev())
    bn, sites = networks()["sprinkler"]
    good = pack_network_for_sampling(bn, sites)
    observed = pack_network(bn, sites[:3], {'W': 1})
    unordered = {k: v.copy() for k, v in good.items()}
    unordered["parents"][1, 0] = 2                       # S's parent index above its own
    idx = torch.full((8,), 7, dtype=torch.int64, device=dev())
    logp = torch.full((8,), 7.0, dtype=torch.float64, device=dev())
    st = torch.full((1,), 7, dtype=torch.int32, device=dev())
    ep = t64([0])
    p = lambda t: t.data_ptr()
    keep = []
    for packed, n, B in ((good, 0, 8), (good, 64, 8), (good, 4, 0), (good, 4, (1 << 24) + 1), (observed, 3, 8), (unordered, 4, 8)):
        arrays, desc = backend.bn_descriptor(packed, dev())
        keep.append(arrays)
        rc = lib.bornvi_bn_sample(h.h, C.byref(desc), n, B, 1, p(ep), p(idx), p(logp), p(st), None)
        assert rc == UNSUPPORTED, (n, B)
    torch.cuda.synchronize()
    assert bool((idx == 7).all()) and bool((logp == 7.0).all()) and int(st.item()) == 7
    with pytest.raises(_ext.BornviError):
        backend.bn_sample(backend.bn_descriptor(good, dev())[1], 4, 0, 1, ep)


# ---- the gradient of weighted log-marginals -------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 3), (2, 2), (5, 3), (6, 8), (3, 32), (63, 2)]


@functools.lru_cache(maxsize=None)
def shape(n, D):
    """cores and the evidence kinds of a shape: empty, one site, half the sites, all sites (two states), shared and unchanged."""
    cores = make_cores(n, D, seed=2)
    c = cores.numpy()
    states = sm.sample(c, SEED, 0, 2)["bits"]
    rng = np.random.default_rng([n, D, 31])
    kinds = [{}, {0: 1}, {n - 1: int(states[0][n - 1])}, {p: int(states[0][p]) for p in range(0, n, 2)},
             {p: int(rng.integers(0, 2)) for p in range(n) if p % 2 == 1 or n == 1}, {p: int(states[0][p]) for p in range(n)},
             {p: int(states[1][p]) for p in range(n)}]
    return dict(cores=cores, c=c, kinds=kinds)


def words_dev(evs, n):
    w = [qm.words(ev, n) for ev in evs]
    return t64([m for m, _ in w]), t64([v for _, v in w])


def run_vjp(S, evs, c):
    n = S["c"].shape[0]
    m, v = words_dev(evs, n)
    return backend.mps_log_marginals_vjp(S["cores"].to(dev()), m, v, torch.tensor(c, dtype=torch.float64, device=dev()))


@pytest.mark.parametrize("n,D", SHAPES)
def test_log_marginals_vjp_against_the_mirror(n, D):
    S = shape(n, D)
    G = backend.mps_log_marginals_vjp_groups(1 << 16)
    assert G == am.MAX_WG and backend.mps_log_marginals_vjp_groups(3) == 3
    cd = S["cores"].to(dev())
    worst = 0.0
    for Q in (1, 3, G, G + 1, 2 * G + 3):
        rng = np.random.default_rng([n, D, Q])
        evs = [S["kinds"][(3 * j + Q) % len(S["kinds"])] for j in range(Q)]
        for c in (rng.standard_normal(Q), np.zeros(Q)):
            grad, logm, st = run_vjp(S, evs, c)
            grad2, logm2, _ = run_vjp(S, evs, c)
            assert torch.equal(grad, grad2) and torch.equal(logm, logm2)              # two calls are bitwise equal
            assert int(st.item()) == 0
            m, v = words_dev(evs, n)
            want, _ = backend.mps_log_marginals(cd, m, v)
            assert torch.equal(logm, want)                                            # bornvi_mps_log_marginals' bits
            ref = am.log_marginal_gradient(S["c"], evs, c)
            g = grad.cpu().numpy()
            r, at = hp.worst(hp.ratio(g, ref["grad"], ref["bound"], X=hp._LongDouble))
            worst = max(worst, r)
            assert r <= 1.0, (Q, r, at)
            if not c.any():
                assert np.all(g == 0.0)
            if D > 1:
                assert np.all(g[0][:, 1:, :] == 0.0) and np.all(g[n - 1][:, :, 1:] == 0.0)
    print(f"n={n} D={D}: worst gradient error / bound = {worst:.2e}")


@pytest.mark.parametrize("n,D", [(5, 3), (63, 2)])
def test_log_marginals_vjp_identities(n, D):
    S = shape(n, D)
    cd = S["cores"].to(dev())
    # an all-clamped query with weight c is the score gradient of that state with weight c
    full = S["kinds"][5]
    c = -0.75
    grad, logm, st = run_vjp(S, [full], [c])
    idx = t64([qm.words(full, n)[1]])
    backend.mps_environments(cd, 1)
    sgrad, slogq, _ = backend.mps_score_vjp(cd, idx, torch.tensor([c], dtype=torch.float64, device=dev()))
    ref = am.log_marginal_gradient(S["c"], [full], [c])
    env = sm.environments(S["c"])
    sref = sm.score_gradient(S["c"], np.array([[full[p] for p in range(n)]]), [c], env)
    cs = c_score(n, D, 1, float(sref["kappa"].max()), float(env["Z_abs"] / env["Z"]))
    lim = EPS * hp.to_f64(ref["bound"] + cs * sref["grad_abs"])
    assert np.all(np.abs(grad.cpu().numpy() - sgrad.cpu().numpy()) <= lim)
    # all-empty evidences: the gradient of log 1
    evs, cc = [{}] * 5, [0.5, -1.25, 2.0, 0.125, -3.0]
    grad, logm, st = run_vjp(S, evs, cc)
    ref = am.log_marginal_gradient(S["c"], evs, cc)
    assert bool((logm == 0.0).all()) and np.all(np.abs(grad.cpu().numpy()) <= EPS * hp.to_f64(ref["bound"]))


def test_log_marginals_vjp_impossible_evidence():
    """A core slice set to zero: status 1 and logm -inf for the evidence that needs it; the other queries' contribution is
    unchanged (the impossible query adds a partial of zeros and its weight stays out of the normaliser's)."""
    n, D = 6, 3
    cores = make_cores(n, D, seed=2).clone()
    cores[3, 1] = 0.0
    S = dict(cores=cores, c=cores.numpy())
    evs = [{0: 1}, {3: 1, 5: 0}, {1: 0, 3: 0}, {}]
    c = [0.5, 4.0, -1.5, 0.25]
    grad, logm, st = run_vjp(S, evs, c)
    keep = [0, 2, 3]
    grad_k, logm_k, st_k = run_vjp(S, [evs[j] for j in keep], [c[j] for j in keep])
    lm = logm.cpu().numpy()
    assert int(st.item()) == 1 and int(st_k.item()) == 0 and lm[1] == -math.inf
    assert np.array_equal(lm[keep], logm_k.cpu().numpy()) and torch.equal(grad, grad_k)
    ref = am.log_marginal_gradient(S["c"], evs, c)
    r, at = hp.worst(hp.ratio(grad.cpu().numpy(), ref["grad"], ref["bound"], X=hp._LongDouble))
    assert r <= 1.0, (r, at)


def test_log_marginals_vjp_refusals():
    lib = _ext.lib()
    h = _ext.handle_for(dev())
    size = lib.bornvi_mps_log_marginals_vjp_workspace_bytes
    for n, D, Q in ((0, 4, 1), (64, 4, 1), (8, 33, 1), (8, 0, 1), (8, 4, 0), (8, 4, (1 << 16) + 1)):
        assert size(h.h, n, D, Q) == 0
    need = size(h.h, 8, 4, 3)
    assert need > 0
    G = C.c_int(-1)
    assert lib.bornvi_mps_log_marginals_vjp_geometry(0, C.byref(G)) == UNSUPPORTED
    assert lib.bornvi_mps_log_marginals_vjp_geometry((1 << 16) + 1, C.byref(G)) == UNSUPPORTED and G.value == -1
    buf = torch.zeros(1 << 22, dtype=torch.uint8, device=dev())
    words = torch.zeros(8, dtype=torch.int64, device=dev())
    out = torch.full((8 * 2 * 33 * 33,), 7.0, dtype=torch.float64, device=dev())
    st = torch.full((1,), 7, dtype=torch.int32, device=dev())
    p = lambda t: t.data_ptr()
    for n, D, Q, nbytes in ((64, 4, 3, buf.numel()), (8, 0, 3, buf.numel()), (8, 33, 3, buf.numel()), (8, 4, 0, buf.numel()),
                            (8, 4, (1 << 16) + 1, buf.numel()), (8, 4, 3, need - 1)):
        rc = lib.bornvi_mps_log_marginals_vjp(h.h, n, D, Q, p(buf), p(words), p(words), p(out), p(out), p(out), p(st), p(buf),
                                              nbytes, None)
        assert rc == UNSUPPORTED, (n, D, Q)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(st.item()) == 7                           # nothing was launched


def test_capture_and_replay():
    """One graph of both calls; the epoch and the evidence words change between the replays; equal to the eager calls.  Under
    capture the descriptor cannot be read back: an observed role then gives NaN and status 1 from the kernel itself."""
    bn, sites = networks()["dropped"]
    n, B, Q, D = len(sites), 257, 5, 3
    keep, desc = backend.bn_descriptor(pack_network_for_sampling(bn, sites), dev())
    spr, spr_sites = networks()["sprinkler"]
    keep_bad, bad = backend.bn_descriptor(pack_network(spr, spr_sites[:3], {'W': 1}), dev())
    cores = make_cores(n, D, seed=3).to(dev())
    ep = torch.zeros(1, dtype=torch.int64, device=dev())
    rng = np.random.default_rng(8)
    cases = {e: (words_dev([{p: int(rng.integers(0, 2)) for p in range(n) if rng.random() < 0.5} for _ in range(Q)], n),
                 torch.from_numpy(rng.standard_normal(Q)).to(dev())) for e in (0, 1, 2)}
    eager = {}
    for e, ((m, v), c) in cases.items():
        ep.fill_(e)
        idx, logp, _ = backend.bn_sample(desc, n, B, SEED, ep)
        grad, logm, _ = backend.mps_log_marginals_vjp(cores, m, v, c)
        eager[e] = tuple(t.clone() for t in (idx, logp, grad, logm))
    mask, value = torch.zeros(Q, dtype=torch.int64, device=dev()), torch.zeros(Q, dtype=torch.int64, device=dev())
    w = torch.zeros(Q, dtype=torch.float64, device=dev())
    idx, logp = torch.empty(B, dtype=torch.int64, device=dev()), torch.empty(B, dtype=torch.float64, device=dev())
    bidx, blogp = torch.empty(B, dtype=torch.int64, device=dev()), torch.empty(B, dtype=torch.float64, device=dev())
    grad, logm = torch.empty_like(cores), torch.empty(Q, dtype=torch.float64, device=dev())
    st = [torch.empty(1, dtype=torch.int32, device=dev()) for _ in range(3)]

    def calls(with_bad):
        backend.bn_sample(desc, n, B, SEED, ep, out_idx=idx, out_logp=logp, status=st[0])
        backend.mps_log_marginals_vjp(cores, mask, value, w, out=grad, out_logm=logm, status=st[1])
        if with_bad:
            backend.bn_sample(bad, 3, B, SEED, ep, out_idx=bidx, out_logp=blogp, status=st[2])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls(False)                                      # the side stream's workspaces exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls(True)
    for e in (2, 0, 1, 2):
        (m, v), c = cases[e]
        ep.fill_(e)
        mask.copy_(m), value.copy_(v), w.copy_(c)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((idx, logp, grad, logm), eager[e]):
            assert torch.equal(got, want), e
        assert int(st[0].item()) == 0 and int(st[1].item()) == 0
        assert int(st[2].item()) == 1 and bool(torch.isnan(blogp).all())
