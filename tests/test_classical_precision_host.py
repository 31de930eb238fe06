"""The per-entry bounds of classical_hp.py, checked on the CPU: a plain float64 NumPy evaluation of every formula of the
table-family kernels lies inside its bound on every shape and input family of test_gpu_classical_precision.py with
n <= 16 (the bounds are real); seven seeded mutants of that evaluation -- the mistakes the earlier, looser comparisons
could not see -- each leave theirs (the bounds bite); and the tie exception of the q32 check excuses at most one entry
in 10^4 of any case."""
import numpy as np
import pytest

import classical_hp as chp
from classical_hp import CLAMP32

if chp.unavailable():
    pytest.skip(chp.unavailable(), allow_module_level=True)

HOST_TABLE_SHAPES = [s for s in chp.TABLE_SHAPES if s[0] <= 16]
HOST_REINFORCE_SHAPES = [s for s in chp.REINFORCE_SHAPES if s[0] <= 16]


# ---- the float64 mirrors (mutate: one of the seeded mistakes) -------------------------------------------------------
def forward_mirror(w, mode, mutate=None):
    w64 = w.astype(np.float64)
    if mode == 0:
        with np.errstate(all="ignore"):
            x = w64 - w64.max(axis=1, keepdims=True)
            e = np.exp(x.astype(np.float32)).astype(np.float64) if mutate == "exp32" else np.exp(x)
    else:
        e = np.abs(w64)
    q32 = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    H = -(q32.astype(np.float64) * np.log(np.maximum(q32, CLAMP32).astype(np.float64))).sum(axis=1)
    return q32, q32.astype(np.float64), H.astype(np.float32)


def vjp_mirror(w, q64, y, ksd2, lam, mode, mutate=None):
    rows, N = w.shape
    g = np.zeros((rows, N))
    if y is not None:
        g = (y * chp.ksd_scale(ksd2, rows)[:, None]).astype(np.float32).astype(np.float64)
    if lam != 0.0:
        qf = q64.astype(np.float32)
        ind = {"no-indicator": np.ones_like(qf, dtype=bool), "strict": qf > CLAMP32}.get(mutate, qf >= CLAMP32)
        g = g + lam * (np.log(np.maximum(qf, CLAMP32).astype(np.float64)) + ind)
    qg = q64 * g
    if mutate == "short-c":
        chunk, G = chp.bt_geom(N)
        qg = qg[:, :(G - 1) * chunk] if G > 1 else qg
    c = qg.sum(axis=1, keepdims=True)
    if mode == 0:
        out = q64 * (g - c)
    else:
        w64 = w.astype(np.float64)
        sg = np.where(w64 == 0.0, 1.0, np.sign(w64)) if mutate == "sign0" else np.sign(w64)
        out = sg * (g - c) / np.abs(w64).sum(axis=1, keepdims=True)
    loss = None if ksd2 is None else np.sqrt(np.where(ksd2 < 1e-12, 1e-12, ksd2))
    return out.astype(np.float32), loss


def reinforce_mirror(idx, logit, log_p, q32, baseline, first, decay, coef=chp.COEF, mutate=None):
    """The kernel's recipe in float64 and 64-bit integers: weights rounded once to u = 2^-e, summed as int64."""
    B, N = idx.shape[0], q32.shape[0]
    raw = logit.astype(np.float64) - log_p.astype(np.float64)[idx]
    mean = raw.sum() / B
    base = mean if first else decay * baseline + (1.0 - decay) * mean
    W = np.abs(raw).max() + abs(base) + abs(coef)
    e = 60 - (B - 1).bit_length() - (int(np.frexp(W)[1]) - 1)
    f = np.rint((raw - base + coef) * 2.0 ** e)
    if mutate == "coarse":
        f = np.rint(f / 1024.0) * 1024.0
    f = f.astype(np.int64)
    if mutate == "drop":
        f[int(np.flatnonzero(q32[idx] > 0.1)[0])] = 0
    S = np.zeros(N, dtype=np.int64)
    np.add.at(S, idx, f)
    s = S.astype(np.float64) * 2.0 ** -e
    q = q32.astype(np.float64)
    live = (q32 >= CLAMP32) & (S != 0)
    d = np.where(live, s / (B * np.where(live, q, 1.0)), 0.0)
    loss = np.float32((np.log(np.maximum(q32, CLAMP32).astype(np.float64)) * s).sum() / B)
    return d, loss, base


# ---- drivers -----------------------------------------------------------------------------------------------------
def table_ratios(n, rows, mode, family, fwd=None, vjp=None):
    """Worst ratios of the mirror over the forward and every VJP configuration: {'q', 'H', 'g'}."""
    w, ref = chp.forward_case(n, rows, mode, family)
    q32, q64, H = forward_mirror(w, mode, fwd)
    out = {k: v[0] for k, v in chp.forward_check(w, mode, q32, q64, H, ref).items()}
    y, ksd2 = chp.vjp_inputs(n, rows)
    out["g"] = 0.0
    for has_y, has_k, lam in chp.VJP_CONFIGS:
        yy, kk = (y if has_y else None), (ksd2 if has_k else None)
        grad, loss = vjp_mirror(w, q64, yy, kk, lam, mode, vjp)
        out["g"] = max(out["g"], chp.vjp_check(w, q64, yy, kk, lam, mode, grad, loss)["g"][0])
    return out


def reinforce_ratios(n, B, kind, first, mutate=None):
    inp = chp.step_inputs(n, B, kind, chp.step_seed(n, B, kind, first))
    ref = chp.reinforce_reference(*inp, chp.BASELINE, first, chp.DECAY)
    return {k: v[0] for k, v in chp.reinforce_check(ref, *reinforce_mirror(*inp, chp.BASELINE, first, chp.DECAY,
                                                                           mutate=mutate)).items()}


# ---- the bounds are real -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,family", chp.TABLE_FAMILIES)
@pytest.mark.parametrize("n,rows", HOST_TABLE_SHAPES)
def test_table_mirror_is_inside_the_bounds(n, rows, mode, family):
    r = table_ratios(n, rows, mode, family)
    C = chp.table_constants(n, mode)
    print(f"mirror n={n} mode={mode} {family}: q {r['q']:.3g} (C_Q {C['q']:g}) H {r['H']:.3g} (C_H {C['H']:g}) "
          f"g {r['g']:.3g} (C_1 {C['g1']:g}, C_c {C['gc']:g})")
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("kind", chp.REINFORCE_KINDS)
@pytest.mark.parametrize("n,B", HOST_REINFORCE_SHAPES)
def test_reinforce_mirror_is_inside_the_bounds(n, B, kind, first):
    r = reinforce_ratios(n, B, kind, first)
    C = chp.reinforce_constants(n, B)
    print(f"mirror n={n} B={B} {kind} first={first}: dLdq {r['d']:.3g} loss {r['loss']:.3g} baseline {r['base']:.3g} "
          f"(T_mean {C['T_mean']:g}, T_loss {C['T_loss']:g})")
    assert max(r.values()) <= 1.0, r


def test_inputs_hold_what_they_are_for():
    """The edge rows' q are the float32 clamp and its two neighbours exactly; the spread rows hold normal float32 q below
    the clamp (the entries an error proportional to q hides in); the peaked samples sit on outcomes with q > 0.1."""
    for n in (12, 13, 14, 21):
        w, (q_star, _) = chp.forward_case(n, 1 if n == 21 else 3, 1, "edge")
        assert np.array_equal(q_star.astype(np.float32)[:, chp.EDGE_AT], np.tile(chp.EDGE_TARGETS, (w.shape[0], 1)))
        assert (w < 0).any()
    w, (q_star, _) = chp.forward_case(12, 3, 0, "edge")
    assert np.isneginf(w).sum() == 9 and (chp.to_f64(q_star) == 0).sum() == 9
    q = chp.to_f64(q_star)
    assert ((q > 1e-11) & (q < 1e-10)).any() and ((q > 1e-10) & (q < 1e-9)).any()
    q = chp.to_f64(chp.forward_case(12, 3, 0, "spread")[1][0])
    assert ((q > chp.F32_MIN_NORMAL) & (q < 1e-20)).sum() > 100 and (q < 2.0 ** -150).any()
    for n, B in chp.REINFORCE_SHAPES:
        idx, _, _, q32 = chp.step_inputs(n, B, "peaked", chp.step_seed(n, B, "peaked", True))
        assert (q32 > 0.1).sum() == min(3, 1 << n) and (q32[idx] > 0.1).mean() >= (0.85 if B >= 64 else 0.0)
        assert abs(float(q32.astype(np.float64).sum()) - 1.0) < 1e-5


# ---- the bounds bite ------------------------------------------------------------------------------------------------
def worst_over(cases, key):
    seen = {c: r[key] for c, r in cases}
    print({c: f"{v:.3g}" for c, v in seen.items()})
    return max(seen.values())


def test_mutant_a_entropy_indicator_dropped():
    """lambda (log c + 1) on every entry: wrong by lambda where q < 1e-10 only."""
    assert worst_over([((n, m, f), table_ratios(n, 3, m, f, vjp="no-indicator"))
                       for n in (3, 12, 13) for m, f in ((0, "spread"), (1, "edge"))], "g") > 1.0


def test_mutant_b_indicator_strict_at_the_clamp():
    """[q > 1e-10] differs from [q >= 1e-10] on the one entry per edge row that equals the float32 1e-10."""
    assert worst_over([((n, 1, "edge"), table_ratios(n, 3, 1, "edge", vjp="strict")) for n in (12, 13, 14)], "g") > 1.0


def test_mutant_c_float32_exp():
    assert worst_over([((n, 0, f), table_ratios(n, 3, 0, f, fwd="exp32"))
                       for n in (3, 12) for f in ("random", "spread")], "q") > 1.0


def test_mutant_d_c_without_the_last_chunk():
    assert worst_over([((n, m, "random"), table_ratios(n, 3, m, "random", vjp="short-c"))
                       for n in (13, 14) for m in (0, 1)], "g") > 1.0


def test_mutant_e_sign_of_zero_is_one():
    assert worst_over([((n, 1, "zeros"), table_ratios(n, 3, 1, "zeros", vjp="sign0")) for n in (1, 3, 13)], "g") > 1.0


def test_mutant_f_one_weight_dropped_on_a_large_q():
    assert worst_over([((n, B), reinforce_ratios(n, B, "peaked", False, "drop"))
                       for n, B in ((3, 64), (12, 65536), (16, 4099))], "d") > 1.0


def test_mutant_g_weights_rounded_1024_times_coarser():
    assert worst_over([((n, B, k), reinforce_ratios(n, B, k, False, "coarse"))
                       for n, B in ((12, 65536), (16, 4099)) for k in ("mixed", "peaked")], "d") > 1.0


# ---- the tie exception is capped -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,family", chp.TABLE_FAMILIES)
@pytest.mark.parametrize("n,rows", chp.TABLE_SHAPES)
def test_tie_exception_excuses_at_most_one_entry_in_ten_thousand(n, rows, mode, family):
    _, (q_star, _) = chp.forward_case(n, rows, mode, family)
    k = chp.tie_exceptions(q_star, chp.table_constants(n, mode)["q"])
    print(f"n={n} mode={mode} {family}: {k} of {q_star.size} entries within C_Q EPS64 q of a float32 tie")
    assert 10_000 * k <= q_star.size
