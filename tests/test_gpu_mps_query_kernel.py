"""bornvi_mps_log_marginals / _sample_clamped / _marginals against the extended-precision mirror (mps_query_mirror.py) and their
contract: the empty-mask identities bit for bit, results that depend on neither the slot, the number of queries nor the
batch, exact power-of-two rescaling, impossible evidence, refused sizes, capturable.

Shapes: SHAPES below (one site with both boundaries, the odd pads and DP template edges, an index past 32 bits, bit 62);
evidence per shape: empty, all n sites (a state the mirror samples), the first site, the last site, alternating sites, a
seeded random mask (at n = 63 the first site is bit 62).

Error bounds, by the rule of test_gpu_mps_sampled_kernel.py (units of EPS64, every rounding a whole unit, the power-of-two
rescalings add none, first order in EPS):
  clamped environments: a clamped step has one D-term and one D-term chain instead of D and 2 D: C_ENV(j) = j (3 D + 1) holds.
  logm = (log E^^(j)_0 - log E^_0) + (e_j - e) ln 2:  C_ENV(n) kappa_c + C_ENV(n) kappa_Z, kappa_c = Zc_abs / Zc, and the
    assembly: two logs, the difference, the product with ln 2, the sum, each at most a unit of the largest partial result,
    which |log Zc| + |log Z| + 4 bounds:  8 (|log Zc| + |log Z| + 4).
  m1[i], m2[i][j] against the same sums of magnitudes (|cores| throughout, over the true Z):  L_{i-1}, the carried M and E_j
    are n - 1 environment steps together (M's first step, s = 1 alone, has the shorter chains): C_ENV(n - 1); mq_inner is
    four D-term chains (T, G, the rows, their sum): 4 D; the quotient and one unit for the subnormal end of ldexp: 2; and
    1 / Z: C_ENV(n) kappa_Z.   C_M = C_ENV(n - 1) + 4 D + 2 + C_ENV(n) kappa_Z.
  logq_cond: logq_bound of the sampler with Z replaced by the clamped normaliser (kappa_Z by kappa_c, log Z by log Zc).
  exp of a log with absolute error e eps: relative error (e + 2) eps.
  q64 of mps_probs (test_gpu_mps_kernel.py): relative (2 C_PSI + 1)(kappa_z + kappa_Z) + 2 + T_Z, T_Z <= 29 for n <= 12.
The constants are not fitted: each test prints the worst ratio beside its bound."""
import functools
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_query_mirror as qm
import mps_sampled_mirror as sm
from tensornetworks_amd import backend
from test_gpu_mps_sampled_kernel import c_env, logq_bound, make_cores

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
SEED = 20250
EPOCH = 3
SHAPES = [(1, 1), (2, 2), (3, 5), (3, 17), (12, 3), (12, 16), (33, 32), (63, 4), (63, 16), (63, 1)]
B_EV = 65                                  # samples per evidence: more than one workgroup, a ragged tail


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def t64(x):
    return torch.tensor(x, dtype=torch.int64, device=dev())


def words_dev(evs, n):
    w = [qm.words(ev, n) for ev in evs]
    return t64([m for m, _ in w]), t64([v for _, v in w])


def f64(x):
    return hp.to_f64(x)


@functools.lru_cache(maxsize=None)
def shape(n, D):
    """cores, the mirror's environments and the evidence list of a shape, shared by the tests and left unchanged."""
    cores = make_cores(n, D)
    c = cores.numpy()
    env = sm.environments(c)
    rng = np.random.default_rng([n, D, 9])
    state = sm.sample(c, SEED, 0, 1)["bits"][0]
    evs = {"empty": {}, "full": {p: int(state[p]) for p in range(n)}, "first": {0: 1}, "last": {n - 1: int(state[n - 1])},
           "alternating": {p: int(state[p]) for p in range(0, n, 2)},
           "random": {p: int(rng.integers(0, 2)) for p in range(n) if rng.random() < 0.5}}
    return dict(cores=cores, c=c, env=env, evs=evs, kZ=float(env["Z_abs"] / env["Z"]), logZ=float(np.log(env["Z"])))


def logm_bound(n, D, ref, shift=0.0):
    """In units of EPS, from mps_query_mirror.log_marginal's dict; shift: what cores times 2^p add to both logs."""
    lc, lz = float(np.log(ref["Zc"])), float(np.log(ref["Z"]))
    return c_env(n, D) * (float(ref["kappa_c"]) + float(ref["kappa_Z"])) + 8 * (abs(lc + shift) + abs(lz + shift) + 4)


def c_marg(n, D, kZ):
    return c_env(n - 1, D) + 4 * D + 2 + c_env(n, D) * kZ


@functools.lru_cache(maxsize=None)
def single_logm(n, D):
    """{evidence name: (logm as a float64 scalar from a Q = 1 call, status)}"""
    S = shape(n, D)
    c = S["cores"].to(dev())
    out = {}
    for name, ev in S["evs"].items():
        m, v = words_dev([ev], n)
        lm, st = backend.mps_log_marginals(c, m, v)
        out[name] = (lm.cpu().numpy()[0], int(st.item()))
    return out


@functools.lru_cache(maxsize=None)
def enumerated(n, D):
    """n <= 12: (q64 of mps_probs as long double, bits, the per-state relative bound of q64 in units of EPS times q64)."""
    S = shape(n, D)
    _, q64, _, _ = backend.mps_probs(S["cores"].to(dev()), want_q32=False)
    q = q64.cpu().numpy().astype(sm.LD)
    bits = sm.bits_of_idx(np.arange(1 << n), n)
    cond = sm.conditionals(S["c"], bits, S["env"])
    with np.errstate(divide="ignore", invalid="ignore"):
        kz = np.where(cond["psi"] != 0, cond["psi_abs"] / np.abs(cond["psi"]), 0)
    werr = q * ((2 * (n * D + 2) + 1) * (kz + S["kZ"]) + 2 + 29)
    return q, bits, werr


@pytest.mark.parametrize("n,D", SHAPES)
def test_log_marginals(n, D):
    S = shape(n, D)
    single = single_logm(n, D)
    c = S["cores"].to(dev())
    assert single["empty"][0] == 0.0 and math.copysign(1.0, single["empty"][0]) == 1.0        # exactly 0.0
    worst = 0.0
    for name, ev in S["evs"].items():
        got, st = single[name]
        assert st == 0
        if name == "empty":
            continue
        ref = qm.log_marginal(S["c"], ev, S["env"])
        bound = EPS * logm_bound(n, D, ref)
        err = abs(float(f64(sm.LD(got) - ref["logm"])))
        worst = max(worst, err / bound)
        assert err <= bound, (name, err, bound)
        if n <= 12:
            q, bits, werr = enumerated(n, D)
            ok = qm.consistent(bits, ev)
            want = q[ok].sum()
            lim = EPS * (want * (logm_bound(n, D, ref) + 2) + werr[ok].sum())
            assert abs(float(f64(np.exp(sm.LD(got)) - want))) <= float(f64(lim)), name
    print(f"n={n} D={D}: worst |logm err| / bound = {worst:.3f}")
    # all n sites clamped: log q of that state, against mps_score_vjp's
    full = S["evs"]["full"]
    idx = t64([qm.words(full, n)[1]])
    backend.mps_environments(c, 1)
    _, lq, st = backend.mps_score_vjp(c, idx, torch.zeros(1, dtype=torch.float64, device=dev()))
    cond = sm.conditionals(S["c"], np.array([[full[p] for p in range(n)]]), S["env"])
    kb = f64(cond["psi_abs"] / np.abs(cond["psi"]))
    b_score = logq_bound(n, D, kb, S["kZ"], f64(cond["logq"]), S["logZ"])[0]
    b_logm = logm_bound(n, D, qm.log_marginal(S["c"], full, S["env"]))
    assert int(st.item()) == 0 and abs(float(lq.item()) - single["full"][0]) <= EPS * (b_score + b_logm)
    # a query's bits depend neither on Q nor on its slot
    names = list(S["evs"])
    for Q in (2, 65, 257):
        order = [names[(5 * s + Q) % len(names)] for s in range(Q)]       # 5 and the 6 names are coprime: every name
        m, v = words_dev([S["evs"][k] for k in order], n)
        lm, st = backend.mps_log_marginals(c, m, v)
        lm = lm.cpu().numpy()
        assert int(st.item()) == 0
        want = np.array([single[k][0] for k in order])
        assert np.array_equal(lm, want), Q


@pytest.mark.parametrize("n,D", SHAPES)
def test_marginals(n, D):
    S = shape(n, D)
    c = S["cores"].to(dev())
    m1, m2 = backend.mps_marginals(c, want_pairs=True)
    only1, none = backend.mps_marginals(c)
    assert none is None and torch.equal(only1, m1)
    assert torch.equal(m2, m2.T) and torch.equal(torch.diagonal(m2), m1)
    again1, again2 = backend.mps_marginals(c, want_pairs=True)
    assert torch.equal(again1, m1) and torch.equal(again2, m2)
    m1, m2 = m1.cpu().numpy(), m2.cpu().numpy()
    ref = qm.marginals(S["c"], S["env"])
    C = c_marg(n, D, S["kZ"])
    r1, at1 = hp.worst(hp.ratio(m1, ref["m1"], ref["m1_abs"], X=hp._LongDouble))
    r2, at2 = hp.worst(hp.ratio(m2, ref["m2"], ref["m2_abs"], X=hp._LongDouble))
    print(f"n={n} D={D}: worst m1 ratio {r1:.2f} at {at1}, m2 ratio {r2:.2f} at {at2}, C_M = {C:.0f} (kappa_Z {S['kZ']:.2f})")
    assert r1 <= C and r2 <= C
    assert np.all(np.isfinite(m1)) and np.all(np.isfinite(m2))
    # exp(log_marginals of {i: 1, j: 1}) against m2[i, j]
    rng = np.random.default_rng([n, D, 21])
    pairs = {(0, n - 1), (0, min(1, n - 1)), tuple(sorted(int(x) for x in rng.integers(0, n, 2))), (n // 2, n // 2)}
    pairs = sorted(pairs)
    evs = [{i: 1, j: 1} for i, j in pairs]
    m, v = words_dev(evs, n)
    lm, st = backend.mps_log_marginals(c, m, v)
    lm = lm.cpu().numpy()
    assert int(st.item()) == 0
    for (i, j), ev, got in zip(pairs, evs, lm):
        r = qm.log_marginal(S["c"], ev, S["env"])
        lim = EPS * (float(f64(ref["m2"][i, j])) * (logm_bound(n, D, r) + 2) + C * float(f64(ref["m2_abs"][i, j])))
        assert abs(math.exp(got) - m2[i, j]) <= lim, (i, j)
    if n <= 12:
        q, bits, werr = enumerated(n, D)
        one = bits.astype(bool)
        for i in range(n):
            for j in range(i, n):
                ok = one[:, i] & one[:, j]
                lim = EPS * (C * ref["m2_abs"][i, j] + werr[ok].sum())
                assert abs(float(f64(sm.LD(m2[i, j]) - q[ok].sum()))) <= float(f64(lim)), (i, j)
    if D == 1:             # mean field: the sites are independent
        a1, ab1 = f64(ref["m1"]), f64(ref["m1_abs"])
        lim = EPS * (C * f64(ref["m2_abs"]) + C * (np.outer(ab1, a1) + np.outer(a1, ab1)) + np.outer(a1, a1))
        off = ~np.eye(n, dtype=bool)
        assert np.all(np.abs(m2 - np.outer(m1, m1))[off] <= lim[off])


@pytest.mark.parametrize("n,D", SHAPES)
def test_sample_clamped_empty_mask_is_the_sampler(n, D):
    c = shape(n, D)["cores"].to(dev())
    ep = t64([EPOCH])
    zero = t64([0])
    junk = t64([(1 << n) - 1])                           # value bits outside the mask are ignored
    for B in (63, 65, 4099):
        backend.mps_environments(c, B)
        idx, logq, st = backend.mps_sample(c, B, SEED, ep)
        for value in (zero, junk):
            cidx, clogq, logm, cst = backend.mps_sample_clamped(c, B, zero, value, SEED, ep)
            assert torch.equal(cidx, idx) and torch.equal(clogq, logq) and int(cst.item()) == int(st.item()) == 0
            assert float(logm.item()) == 0.0


@functools.lru_cache(maxsize=None)
def decided_seed(n, D, name):
    """The first seed from SEED on at which the mirror leaves no draw of this evidence undecided, and the mirror's run."""
    S = shape(n, D)
    for seed in range(SEED, SEED + 16):
        s = qm.sample_clamped(S["c"], S["evs"][name], seed, EPOCH, B_EV)
        if s["undecided"] == 0:
            return seed, s
    raise AssertionError("no decided seed among 16")


@pytest.mark.parametrize("n,D", SHAPES)
def test_sample_clamped_against_the_mirror(n, D):
    S = shape(n, D)
    c = S["cores"].to(dev())
    ep = t64([EPOCH])
    single = single_logm(n, D)
    worst = 0.0
    for name, ev in S["evs"].items():
        seed, mir = decided_seed(n, D, name)
        assert mir["undecided"] == 0                     # no draw is left out
        m, v = words_dev([ev], n)
        idx, logq, logm, st = backend.mps_sample_clamped(c, B_EV, m, v, seed, ep)
        idx2, logq2, logm2, _ = backend.mps_sample_clamped(c, B_EV, m, v, seed, ep)
        assert torch.equal(idx, idx2) and torch.equal(logq, logq2) and torch.equal(logm, logm2)      # two calls are bitwise equal
        big_idx, big_logq, _, _ = backend.mps_sample_clamped(c, 257, m, v, seed, ep)                  # draws do not depend on B
        assert torch.equal(big_idx[:B_EV], idx) and torch.equal(big_logq[:B_EV], logq)
        assert int(st.item()) == 0
        assert logm.cpu().numpy()[0] == single[name][0]                                               # the log-marginal call's bits
        gi, gl = idx.cpu().numpy(), logq.cpu().numpy()
        bits = sm.bits_of_idx(gi, n)
        assert np.all(qm.consistent(bits, ev))                                                        # the evidence bits
        assert np.array_equal(bits, mir["bits"])                                                      # the mirror's decisions
        assert np.all(gi >= 0)
        if name == "full":
            assert np.all(gl == 0.0) and np.all(gi == qm.words(ev, n)[1])
            continue
        kc = float(mir["Zc_abs"] / mir["Zc"])
        kb = f64(mir["psi_abs"] / np.abs(mir["psi"]))
        lZc = float(np.log(mir["Zc"]))
        bound = logq_bound(n, D, kb, kc, f64(mir["logq"]), lZc)
        ratio = np.abs(f64(gl.astype(sm.LD) - mir["logq"])) / (EPS * bound)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, name
        # log q(z | evidence) + log q(evidence) = log q(z), against mps_score_vjp's
        backend.mps_environments(c, B_EV)
        _, lq, st2 = backend.mps_score_vjp(c, idx, torch.zeros(B_EV, dtype=torch.float64, device=dev()))
        lq = lq.cpu().numpy()
        full_logq = f64(mir["logq"] + np.log(mir["Zc"]) - np.log(S["env"]["Z"]))
        b_score = logq_bound(n, D, kb, S["kZ"], full_logq, S["logZ"])
        b_logm = logm_bound(n, D, qm.log_marginal(S["c"], ev, S["env"]))
        assert int(st2.item()) == 0
        assert np.all(np.abs((gl + single[name][0]) - lq) <= EPS * (bound + b_logm + b_score + np.abs(lq)))
    print(f"n={n} D={D}: worst logq_cond ratio = {worst:.3f}")


def test_power_of_two_scaling():
    """n = 63, D = 4: cores times 2^+-12 move psi^2 by 2^+-1512.  Every query is a ratio: logm, m1, m2 stay within their
    bounds (the assembly's with the shifted logs) and the clamped draws are bitwise the same."""
    n, D = 63, 4
    S = shape(n, D)
    ep = t64([EPOCH])
    names = [k for k in S["evs"] if k != "empty"]
    m, v = words_dev([S["evs"][k] for k in names], n)
    ref = qm.marginals(S["c"], S["env"])
    C = c_marg(n, D, S["kZ"])
    base = {}
    for p in (0, 12, -12):
        c = (S["cores"] * 2.0 ** p).to(dev())
        shift = 2 * n * p * math.log(2.0)
        lm, st = backend.mps_log_marginals(c, m, v)
        assert int(st.item()) == 0
        for k, got in zip(names, lm.cpu().numpy()):
            r = qm.log_marginal(S["c"], S["evs"][k], S["env"])
            assert abs(float(f64(sm.LD(got) - r["logm"]))) <= EPS * logm_bound(n, D, r, shift), (p, k)
        m1, m2 = backend.mps_marginals(c, want_pairs=True)
        r1, _ = hp.worst(hp.ratio(m1.cpu().numpy(), ref["m1"], ref["m1_abs"], X=hp._LongDouble))
        r2, _ = hp.worst(hp.ratio(m2.cpu().numpy(), ref["m2"], ref["m2_abs"], X=hp._LongDouble))
        assert r1 <= C and r2 <= C, (p, r1, r2)
        for k in ("alternating", "random"):
            seed, _ = decided_seed(n, D, k)
            em, evv = words_dev([S["evs"][k]], n)
            idx, _, _, st = backend.mps_sample_clamped(c, B_EV, em, evv, seed, ep)
            assert int(st.item()) == 0
            if p == 0:
                base[k] = idx
            else:
                assert torch.equal(idx, base[k]), (p, k)


def test_zero_probability_evidence():
    """A_k[s] = 0 at a clamped site: logm -inf and the status word; the sampler reports status 1, NaN logq and keeps the
    evidence's bits, its free bits from the dead site on 0; the machine itself is valid: m1, m2 finite."""
    n, D = 12, 3
    cores = make_cores(n, D).clone()
    cores[5, 1] = 0.0                                    # q(z_5 = 1) = 0
    c = cores.to(dev())
    evs = [{5: 1}, {5: 1, 0: 1, 11: 1}, {5: 0}, {}]
    m, v = words_dev(evs, n)
    lm, st = backend.mps_log_marginals(c, m, v)
    lm = lm.cpu().numpy()
    assert int(st.item()) == 1 and lm[0] == -math.inf and lm[1] == -math.inf and np.isfinite(lm[2]) and lm[3] == 0.0
    ok, st = backend.mps_log_marginals(c, m[2:], v[2:])
    assert int(st.item()) == 0 and np.array_equal(ok.cpu().numpy(), lm[2:])
    ep = t64([EPOCH])
    for ev in evs[:2]:
        em, evv = words_dev([ev], n)
        idx, logq, logm, st = backend.mps_sample_clamped(c, B_EV, em, evv, SEED, ep)
        assert int(st.item()) == 1 and float(logm.item()) == -math.inf and bool(torch.isnan(logq).all())
        bits = sm.bits_of_idx(idx.cpu().numpy(), n)
        assert np.all(qm.consistent(bits, ev))
        free = [p for p in range(n) if p not in ev]
        assert np.all(bits[:, free] == 0)                # the evidence's environment is 0 from the first site on
    m1, m2 = backend.mps_marginals(c, want_pairs=True)
    assert bool(torch.isfinite(m1).all()) and bool(torch.isfinite(m2).all())
    assert float(m1[5].item()) == 0.0 and bool((m2[5] == 0).all())
    # a non-finite environment: NaN and the status word
    bad = make_cores(n, D).clone()
    bad[7, 0, 0, 0] = math.inf
    lm, st = backend.mps_log_marginals(bad.to(dev()), m[:1], v[:1])
    assert int(st.item()) == 1 and bool(torch.isnan(lm).all())


def test_refused_sizes():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    UNSUPPORTED = -4
    size = lib.bornvi_mps_query_workspace_bytes
    for n, D, Q in ((0, 4, 1), (64, 4, 1), (8, 33, 1), (8, 0, 1), (8, 4, 0), (8, 4, (1 << 16) + 1)):
        assert size(h.h, n, D, Q) == 0
    need = size(h.h, 8, 4, 3)
    assert need > 0 and size(h.h, 8, 4, 1 << 16) > need
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    words = torch.zeros(8, dtype=torch.int64, device=dev())
    out = torch.full((8,), 7.0, dtype=torch.float64, device=dev())
    idx = torch.full((8,), 7, dtype=torch.int64, device=dev())
    st = torch.full((1,), 7, dtype=torch.int32, device=dev())
    p = lambda t: t.data_ptr()
    for n, D, Q, nbytes in ((0, 4, 3, buf.numel()), (64, 4, 3, buf.numel()), (8, 33, 3, buf.numel()), (8, 4, 0, buf.numel()),
                            (8, 4, (1 << 16) + 1, buf.numel()), (8, 4, 3, need - 1)):
        rc = lib.bornvi_mps_log_marginals(h.h, n, D, Q, p(buf), p(words), p(words), p(out), p(st), p(buf), nbytes, None)
        assert rc == UNSUPPORTED, (n, D, Q)
    need1 = size(h.h, 8, 4, 1)
    for n, D, B, nbytes in ((0, 4, 8, buf.numel()), (64, 4, 8, buf.numel()), (8, 33, 8, buf.numel()), (8, 4, 0, buf.numel()),
                            (8, 4, (1 << 24) + 1, buf.numel()), (8, 4, 8, need1 - 1)):
        rc = lib.bornvi_mps_sample_clamped(h.h, n, D, B, p(buf), p(words), p(words), 1, p(words), p(idx), p(out), p(out), p(st),
                                           p(buf), nbytes, None)
        assert rc == UNSUPPORTED, (n, D, B)
    for n, D, nbytes in ((0, 4, buf.numel()), (64, 4, buf.numel()), (8, 33, buf.numel()), (8, 4, need1 - 1)):
        rc = lib.bornvi_mps_marginals(h.h, n, D, p(buf), p(out), None, p(buf), nbytes, None)
        assert rc == UNSUPPORTED, (n, D)
    torch.cuda.synchronize()
    # nothing was launched: no output was touched
    assert bool((out == 7.0).all()) and bool((idx == 7).all()) and int(st.item()) == 7
    with pytest.raises(_ext.BornviError, match="queries"):
        backend.mps_log_marginals(make_cores(4, 2).to(dev()), torch.zeros(0, dtype=torch.int64, device=dev()),
                                  torch.zeros(0, dtype=torch.int64, device=dev()))


def test_capture_and_replay():
    """One graph of the three calls; epoch_dev and the evidence words change between the replays; equal to the eager calls."""
    n, D, B, Q = 12, 5, 257, 5
    c = make_cores(n, D, seed=3).to(dev())
    ep = torch.zeros(1, dtype=torch.int64, device=dev())
    rng = np.random.default_rng(4)
    cases = {}
    for e in (0, 1, 2):
        qs = [{p: int(rng.integers(0, 2)) for p in range(n) if rng.random() < 0.4} for _ in range(Q)]
        cases[e] = (words_dev(qs, n), words_dev([qs[0]], n))
    eager = {}
    for e, ((qm_, qv_), (sm_, sv_)) in cases.items():
        ep.fill_(e)
        lm, _ = backend.mps_log_marginals(c, qm_, qv_)
        idx, logq, logm, _ = backend.mps_sample_clamped(c, B, sm_, sv_, SEED, ep)
        m1, m2 = backend.mps_marginals(c, want_pairs=True)
        eager[e] = tuple(t.clone() for t in (lm, idx, logq, logm, m1, m2))
    qmask, qvalue = torch.zeros(Q, dtype=torch.int64, device=dev()), torch.zeros(Q, dtype=torch.int64, device=dev())
    smask, svalue = torch.zeros(1, dtype=torch.int64, device=dev()), torch.zeros(1, dtype=torch.int64, device=dev())
    lm = torch.empty(Q, dtype=torch.float64, device=dev())
    idx = torch.empty(B, dtype=torch.int64, device=dev())
    logq = torch.empty(B, dtype=torch.float64, device=dev())
    logm = torch.empty(1, dtype=torch.float64, device=dev())
    m1 = torch.empty(n, dtype=torch.float64, device=dev())
    m2 = torch.empty(n, n, dtype=torch.float64, device=dev())
    st1 = torch.empty(1, dtype=torch.int32, device=dev())
    st2 = torch.empty(1, dtype=torch.int32, device=dev())

    def calls():
        backend.mps_log_marginals(c, qmask, qvalue, out=lm, status=st1)
        backend.mps_sample_clamped(c, B, smask, svalue, SEED, ep, out_idx=idx, out_logq=logq, out_logm=logm, status=st2)
        backend.mps_marginals(c, want_pairs=True, out_m1=m1, out_m2=m2)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()                                           # the side stream's workspaces exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls()
    for e in (2, 0, 1, 2):
        (qm_, qv_), (sm_, sv_) = cases[e]
        ep.fill_(e)
        qmask.copy_(qm_), qvalue.copy_(qv_), smask.copy_(sm_), svalue.copy_(sv_)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((lm, idx, logq, logm, m1, m2), eager[e]):
            assert torch.equal(got, want), e
        assert int(st1.item()) == 0 and int(st2.item()) == 0
