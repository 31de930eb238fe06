"""Pins tests/hp_reference.py (the extended-precision reference of the Stein path) and shows that its per-entry bounds
are attainable: the fp64 oracle (oracle/stein.py, NumPy) lies inside every bound on every input family, and four
deliberately wrong copies of it do not -- while the max|K|-scaled comparisons of the older tests accept two of them
(the other two they catch as well, which the test records).
The printed table of oracle ratios (pytest -s) is where the measured constants of test_gpu_stein_precision.py come from.
"""
import math

import numpy as np
import pytest

import hp_reference as hp
from conftest import golden
from oracle import stein as os_
from tensornetworks_amd.bayesian_network import BayesianNetwork, pack_network, synthetic_network

EPS_LD_IN_EPS64 = float(np.finfo(np.longdouble).eps) / hp.EPS64
GOLDENS = ["sprinkler_w1", "sprinkler_w0", "sprinkler_rand0", "sprinkler_rand1", "sprinkler_rand2", "synthetic_n4_s0",
           "synthetic_n5_s0", "synthetic_n5_s1", "synthetic_n6_s0", "synthetic_n8_s0", "two_node"]


def two_node():
    bn = BayesianNetwork()
    bn.add_node('A', cpt={(): {0: 0.8, 1: 0.2}})
    bn.add_node('B', cpt={(0,): {0: 0.7, 1: 0.3}, (1,): {0: 0.4, 1: 0.6}}, parent_names=['A'])
    return bn


def test_long_double_is_extended():
    assert hp.HAVE_LONGDOUBLE, "x86 hosts have an 80-bit long double; elsewhere the helper falls back to mpmath"
    assert hp.arithmetic().name == "longdouble" and hp.unavailable(16) is None
    assert "long double unavailable" in hp.unavailable(9, hp.arithmetic("mpmath"))


@pytest.mark.parametrize("name", GOLDENS)
def test_helper_against_golden(name):
    """Scores, p(x, z) and K_p captured from the reference (fp64) lie inside the derived bounds around the helper."""
    g = golden(name + ".npz")
    n = g["S"].shape[1]
    packed = pack_network(two_node(), ['A'], {'B': 1}) if name == "two_node" else \
        {k[5:]: g[k] for k in g.files if k.startswith("pack_")}
    S, pxz, Sb, zeroed = hp.score_packed(packed, n)
    Cp, Cs = hp.score_constants(packed)
    assert hp.worst(hp.ratio(g["pxz"], pxz, pxz))[0] <= Cp
    assert hp.worst(hp.ratio(g["S"], S, Sb))[0] <= Cs
    assert np.array_equal(zeroed, np.all(g["S"] == 0, axis=1) & (np.abs(g["pxz"]) < 1e-12))
    rows = g["rows"] if "rows" in g.files else None
    K, B, d = hp.gram_bound(g["S"], n, 1.0, rows=rows)
    if n <= 6:
        K = hp.gram_four_terms(g["S"], n, 1.0, rows=rows)
    r, at = hp.worst(hp.ratio(g["K"], K, B) / hp.gram_constant(n, d))
    assert r <= 1.0, (name, r, at)


def test_reference_known_answers():
    """The reference's own assertions (stein_utils.py:205-251) that concern numbers: p(x, z), both scores, both kernel
    values, the base kernel exp(-2/4) and the Hamming distance behind it."""
    bn = two_node()
    S, pxz, _, _ = hp.score(bn, {'B': 1}, ['A'])
    assert abs(float(pxz[1]) - 0.12) < 1e-17                                              # :229-230
    assert abs(float(S[1, 0]) + 1.0) < 1e-15 and abs(float(S[0, 0]) - 0.5) < 1e-15         # :233-236
    K, _ = hp.gram_terms(hp.to_f64(S), 1, 1.0)
    e1 = np.exp(np.longdouble(-1))
    assert abs(K[0, 1] - (2 * e1 - np.longdouble(2.5))) < 1e-15                            # :245-247
    assert abs(K[0, 0] - (np.longdouble(1.25) - e1)) < 1e-15                               # :249-251
    assert hp.popcount(np.array([0b0011 ^ 0b1001]))[0] == 2                                # :208-211
    # base kernel at distance 2 of 4 (:214-217): K_p of all-zero scores is the trace term 2 sum_b (k - k_b)
    K4 = hp.gram_four_terms(np.zeros((16, 4)), 4, 1.0)
    k = lambda dd: np.exp(np.longdouble(-dd) / 4)
    assert abs(K4[0b0011, 0b1001] - 2 * (2 * (k(2) - k(1)) + 2 * (k(2) - k(3)))) < 1e-17


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("ls", [0.3, 1.0, 3.0])
def test_long_double_against_mpmath(n, ls):
    """Every long-double routine against the same routine run in mpmath at 40 digits: a few hundred long-double units."""
    M = hp.arithmetic("mpmath")
    tol = 200 * EPS_LD_IN_EPS64                    # in units of EPS64 * bound
    for fam in ("mild", "wide", "spiky"):
        S = hp.scores(fam, n, 3)
        K, B, _ = hp.gram_bound(S, n, ls)
        Km, Bm, _ = hp.gram_bound(S, n, ls, X=M)
        K4m = hp.gram_four_terms(S, n, ls, X=M)
        for got in (K, hp.gram_four_terms(S, n, ls)):
            for ref in (Km, K4m):
                assert np.all(np.abs(M.arr(hp.to_f64(got)) - ref) <= (tol + 1) * hp.EPS64 * Bm)
        K64 = hp.to_f64(K)
        for qf in ("dirichlet", "signed", "onehot"):
            q = hp.qvec(qf, n, 1)
            y, Yb, k2, K2b = hp.matvec(K64, q)
            ym, Ybm, k2m, K2bm = hp.matvec(K64, q, X=M)
            assert np.all(np.abs(M.arr(hp.to_f64(y)) - ym) <= 2 * hp.EPS64 * Ybm)      # (to_f64 itself rounds once)
            assert abs(M.num(float(k2)) - k2m) <= 2 * hp.EPS64 * K2bm
            yk, Ykb, kk2, _ = hp.kron(S, q, n, ls)
            ykm, Ykbm, kk2m, _ = hp.kron(S, q, n, ls, X=M)
            assert np.all(np.abs(M.arr(hp.to_f64(yk)) - ykm) <= 2 * hp.EPS64 * Ykbm)
            # and the recipe is the matrix: kron == dense in 40 digits, to the long-double rounding of K64
            ymm = Km @ M.arr(q)
            assert np.all(np.abs(ykm - ymm) <= 1e-30 * Ykbm)
    bn, lat, obs, x = hp.sharp_network(n, 1)
    S, pxz, Sb, z = hp.score(bn, x, lat)
    Sm, pm, Sbm, zm = hp.score(bn, x, lat, X=M)
    assert np.array_equal(z, zm)
    assert np.all(np.abs(M.arr(hp.to_f64(S)) - Sm) <= 2 * hp.EPS64 * Sbm)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("ls", [0.3, 1.0, 3.0])
def test_four_term_form_equals_closed_form(n, ls):
    """Extended precision, every score family: the closed form used above n = 6 is the definition used below."""
    for fam in hp.SCORE_FAMILIES:
        S = hp.scores(fam, n, 2)
        K, B, _ = hp.gram_bound(S, n, ls)
        K4 = hp.gram_four_terms(S, n, ls)
        # k - k_b loses log2(n l) bits to cancellation, in long double: 64 n l long-double units, 0.2 EPS64 at most
        r, at = hp.worst(np.abs(K4 - K) / (hp.EPS64 * B))
        assert r <= 64 * max(1.0, n * ls) * EPS_LD_IN_EPS64 <= 0.7, (fam, r, at)


# ------------------------------------------------------------------------------------------------ the oracle is inside
def _oracle_finish(shifted, y, k2):
    loss = math.sqrt(max(k2, 1e-12))
    inv = 0.0 if k2 < 1e-12 else 1.0 / loss
    return loss, y * inv, ((shifted[0::2] - shifted[1::2]) @ y) * (0.5 * inv)


@pytest.mark.parametrize("n", [2, 5, 8])
@pytest.mark.parametrize("ls", [0.3, 1.0, 3.0])
def test_fp64_oracle_inside_every_bound(n, ls):
    N = 1 << n
    Cy_max, Ck_max = hp.dense_constants(N)
    Cky_max, Ckk_max = hp.kron_constant(n)
    lines = []
    for fam in hp.SCORE_FAMILIES:
        S = hp.scores(fam, n, 1)
        Ko = os_.gram_closed_form(S, n, ls)
        K, B = hp.gram_terms(S, n, ls)
        d = hp.popcount(np.arange(N)[:, None] ^ np.arange(N)[None, :])
        rg = hp.ratio(Ko, K, B)
        w, at = hp.worst(rg / hp.gram_constant(n, d))
        assert w <= 1.0, ("gram", fam, n, ls, hp.worst(rg), at)
        lines.append(f"gram    n={n} l={ls} S={fam:9s} oracle ratio {hp.worst(rg)[0]:8.2f} (C = 3n + d + 12)")
        for qf in hp.Q_FAMILIES:
            q = hp.qvec(qf, n, 1)
            fl = hp.underflow_floor(qf, N)
            y, Yb, k2, K2b = hp.matvec(Ko, q)
            yo = Ko @ q
            ry, rk = hp.worst(hp.ratio(yo, y, Yb, fl)), hp.worst(hp.ratio(q @ yo, k2, K2b, fl * N))
            assert ry[0] <= Cy_max and rk[0] <= Ck_max, ("dense", fam, qf, n, ry, rk)
            yk, Ykb, kk2, Kk2b = hp.kron(S, q, n, ls)
            yko = os_.stein_matvec_kron(S, q, n, ls)
            rky = hp.worst(hp.ratio(yko, yk, Ykb, fl * n))
            rkk = hp.worst(hp.ratio(q @ yko, kk2, Kk2b, fl * n * N))
            assert rky[0] <= Cky_max and rkk[0] <= Ckk_max, ("kron", fam, qf, n, rky, rkk)
            lines.append(f"matvec  n={n} l={ls} S={fam:9s} q={qf:9s} dense y {ry[0]:6.2f} ksd2 {rk[0]:6.2f} | "
                         f"kron y {rky[0]:6.2f} ksd2 {rkk[0]:6.2f}")
    print("\n".join(lines))


@pytest.mark.parametrize("n,n_shift", [(4, 1), (4, 7), (8, 7)])
def test_fp64_finish_inside_bounds(n, n_shift):
    N = 1 << n
    rng = np.random.default_rng(n * 10 + n_shift)
    y = hp.scores("wide", n, 5)[:, 0].copy()
    shifted = rng.dirichlet(np.full(N, 0.3), 2 * n_shift)
    for k2 in hp.KSD2_EDGE_VALUES:
        ref = hp.finish(shifted, y, np.array([k2]))
        loss, dldq, grad = _oracle_finish(shifted, y, k2)
        assert ref["clamped"] == (k2 < 1e-12)
        assert hp.worst(hp.ratio(loss, ref["loss"], ref["loss"]))[0] <= hp.FINISH_DERIVED_C
        assert hp.worst(hp.ratio(dldq, ref["dldq"], ref["dldq_bound"]))[0] <= hp.FINISH_DERIVED_C
        rg = hp.worst(hp.ratio(grad, ref["grad"], ref["grad_bound"]))[0]
        assert rg <= N + 2 + hp.FINISH_DERIVED_C
        print(f"finish  n={n} n_shift={n_shift} ksd2={k2:.3e} oracle dot ratio {rg:.2f}")
        if k2 < 1e-12:
            assert float(ref["loss"]) == 1e-6 and not np.any(hp.to_f64(ref["dldq"])) and not np.any(hp.to_f64(ref["grad"]))


@pytest.mark.parametrize("n", [3, 6])
def test_fp64_score_inside_bounds(n):
    for bn, lat, obs, x in (hp.sharp_network(n, 0), hp.sharp_network(n, 1), hp.cut_network()):
        packed = pack_network(bn, lat, x)
        S, pxz, Sb, zeroed = hp.score_packed(packed, len(lat))
        Cp, Cs = hp.score_constants(packed)
        So, po = os_.score_matrix(bn, x, lat), os_.joint_vector(bn, x, lat)
        assert hp.worst(hp.ratio(po, pxz, pxz))[0] <= Cp
        assert hp.worst(hp.ratio(So, S, Sb))[0] <= Cs
        assert np.array_equal(zeroed, np.abs(po) < 1e-12)
    bn, lat, obs, x = hp.cut_network()
    _, pxz, _, zeroed = hp.score(bn, x, lat)
    assert not zeroed[0b110] and zeroed[0b111]
    assert abs(float(pxz[0b110]) / 1e-12 - 1.001) < 1e-6 and abs(float(pxz[0b111]) / 1e-12 - 0.999) < 1e-6


# ------------------------------------------------------------------------------------------------ mutation check
def _gram_mutant(S, n, ls, drop_2c_bit=None, wrong_c_above=None):
    """oracle.stein.gram_closed_form with one of two planted errors."""
    N = 2 ** n
    a = math.exp(-1.0 / (n * ls))
    idx = np.arange(N)
    x = idx[:, None] ^ idx[None, :]
    bits = ((x[:, :, None] >> (n - 1 - np.arange(n))[None, None, :]) & 1).astype(np.float64)
    c = np.where(bits > 0, 1.0 - 1.0 / a, 1.0 - a)
    two_c = 2.0 * c
    if drop_2c_bit is not None:
        two_c[:, :, drop_2c_bit] = 0.0
    if wrong_c_above is not None:
        big = np.maximum(np.abs(S[:, None, :]), np.abs(S[None, :, :])) > wrong_c_above
        c = np.where(big & (bits > 0), 1.0 - a, c)
        two_c = 2.0 * c
    T = S[:, None, :] * S[None, :, :] - c * (S[:, None, :] + S[None, :, :]) + two_c
    return (a ** bits.sum(-1)) * T.sum(-1)


def test_mutations_are_caught_per_entry_and_missed_globally():
    """(a) 2 c_b dropped for one bit; (b) c_b = 1 - a on differing bits where |S| > 1e6; (c) one 32-row strip of the
    contraction accumulated in float32; (d) one column block of the transposed partials skipped under a strip-sparse q.
    (a) and (c) pass the max|K|-scaled comparison the suite used so far.  (b) and (d) do not on this family: (b)'s error,
    c_b times a score of 1e9 ... 1e11, is still above 3e-15 max|K| ~ 1e8, and (d)'s dropped block (about 0.5) is above
    1e-13 of the strip-sparse q's own scale; both outcomes are recorded, not required.  All four fail the per-entry ratio
    by seven orders of magnitude or more."""
    n, ls = 8, 1.0
    N = 1 << n
    S = hp.scores("spiky", n, 1)
    Ko = os_.gram_closed_form(S, n, ls)
    K, B = hp.gram_terms(S, n, ls)
    d = hp.popcount(np.arange(N)[:, None] ^ np.arange(N)[None, :])
    C = hp.gram_constant(n, d)
    report = []
    for tag, Km in (("a", _gram_mutant(S, n, ls, drop_2c_bit=3)), ("b", _gram_mutant(S, n, ls, wrong_c_above=1e6))):
        old_ok = bool(np.all(np.abs(Km - Ko) <= 3e-15 * np.abs(Ko).max()))
        new = hp.worst(hp.ratio(Km, K, B) / C)[0]
        report.append((tag, old_ok, new))
    big = np.abs(S).max(axis=1) > 1e6
    strips = [s for s in range(N // 32) if not big[32 * s:32 * s + 32].any()]
    q = hp.qvec("dirichlet", n, 1)
    y, Yb, k2, K2b = hp.matvec(Ko, q)
    Cy = hp.measured_constant(hp.worst(hp.ratio(Ko @ q, y, Yb))[0], hp.dense_constants(N)[0])
    s = strips[1]
    yc = Ko @ q
    yc[32 * s:32 * s + 32] = (Ko[32 * s:32 * s + 32].astype(np.float32) * q.astype(np.float32)).sum(axis=1, dtype=np.float32)
    scale = (np.abs(Ko) @ np.abs(q)).max()
    report.append(("c", bool(np.all(np.abs(yc - Ko @ q) <= 1e-13 * scale)), hp.worst(hp.ratio(yc, y, Yb))[0] / Cy))
    qs = np.zeros(N)
    qs[32 * strips[0]:32 * strips[0] + 32] = 1.0 / 32                       # strip-sparse q on a mild strip
    y, Yb, k2, K2b = hp.matvec(Ko, qs)
    Cy = hp.measured_constant(hp.worst(hp.ratio(Ko @ qs, y, Yb))[0], hp.dense_constants(N)[0])
    yd = Ko @ qs
    s = strips[2]                                                            # a later block: fed by transposed partials
    yd[32 * s:32 * s + 32] -= Ko[32 * s:32 * s + 32, 32 * strips[0]:32 * strips[0] + 32] @ qs[32 * strips[0]:32 * strips[0] + 32]
    scale = (np.abs(Ko) @ np.abs(qs)).max()                                  # (the suite's scale, from the q contracted)
    report.append(("d", bool(np.all(np.abs(yd - Ko @ qs) <= 1e-13 * scale)), hp.worst(hp.ratio(yd, y, Yb))[0] / Cy))
    for tag, old_ok, new in report:
        print(f"mutation ({tag}): max|K|-scaled check {'accepts' if old_ok else 'rejects'}; per-entry ratio / C = {new:.3g}")
    assert all(old_ok for tag, old_ok, _ in report if tag in "ac"), report
    assert all(new > 1e3 for _, _, new in report), report


@pytest.mark.parametrize("n,sharp", [(5, False), (5, True), (8, False), (8, True)])
def test_fp64_oracle_inside_bounds_on_networks(n, sharp):
    """The chain CPT -> S -> K_p -> y in fp64 (oracle) on a mild and a near-deterministic network (bn-sharp), with the
    exact posterior q = p(x, z) / sum p(x, z) among the vectors.  Where no row is zeroed by the 1e-12 cut the posterior
    is the cancellation case: K_p q and q^T K_p q are rounding, and |ksd2| itself lies within the smallest measured
    constant (16) of EPS64 * K2b, for the dense and the matrix-free form -- the bound the GPU test asserts there.  On the
    sharp network zero-score rows carry posterior mass, K_p q does not cancel, and only the forms' own bounds hold."""
    N = 1 << n
    bn, lat, obs, x = hp.sharp_network(n, 5) if sharp else synthetic_network(n, 5)
    S = os_.score_matrix(bn, x, lat)
    pxz = os_.joint_vector(bn, x, lat)
    Sr, pr, Sb, zeroed = hp.score(bn, x, lat)
    kept, big = hp.surviving_rows(zeroed, Sr)
    print(f"network n={n} sharp={sharp}: {kept} of {N} rows keep a score, {big} of them with |s| > 1e4")
    assert kept >= N // 4 and (big >= 1) == sharp
    Ko = os_.gram_closed_form(S, n, 1.0)
    K, B = hp.gram_terms(S, n, 1.0)
    d = hp.popcount(np.arange(N)[:, None] ^ np.arange(N)[None, :])
    rg = hp.ratio(Ko, K, B)
    assert hp.worst(rg / hp.gram_constant(n, d))[0] <= 1.0
    print(f"gram    n={n} S={'bn-sharp' if sharp else 'bn-mild'} oracle ratio {hp.worst(rg)[0]:.2f}")
    Cy_max, Ck_max = hp.dense_constants(N)
    Cky_max, Ckk_max = hp.kron_constant(n)
    for qf, q in [("posterior", pxz / pxz.sum()), ("dirichlet", hp.qvec("dirichlet", n, 1)), ("signed", hp.qvec("signed", n, 1))]:
        y, Yb, k2, K2b = hp.matvec(Ko, q)
        yo = Ko @ q
        ry, rk = hp.worst(hp.ratio(yo, y, Yb))[0], hp.worst(hp.ratio(q @ yo, k2, K2b))[0]
        yk, Ykb, kk2, Kk2b = hp.kron(S, q, n, 1.0)
        yko = os_.stein_matvec_kron(S, q, n, 1.0)
        rky, rkk = hp.worst(hp.ratio(yko, yk, Ykb))[0], hp.worst(hp.ratio(q @ yko, kk2, Kk2b))[0]
        assert ry <= Cy_max and rk <= Ck_max and rky <= Cky_max and rkk <= Ckk_max
        print(f"matvec  n={n} sharp={sharp} q={qf:9s} dense y {ry:6.2f} ksd2 {rk:6.2f} | kron y {rky:6.2f} ksd2 {rkk:6.2f}")
        if qf == "posterior":
            a_d, a_k = abs(q @ yo) / (hp.EPS64 * float(K2b)), abs(q @ yko) / (hp.EPS64 * float(Kk2b))
            print(f"posterior n={n} sharp={sharp}: |ksd2| / (EPS64 K2b) dense {a_d:.3g} (reference {abs(float(k2)) / (hp.EPS64 * float(K2b)):.3g}), kron {a_k:.3g}")
            if not zeroed.any():
                assert a_d <= 16.0 and a_k <= 16.0
