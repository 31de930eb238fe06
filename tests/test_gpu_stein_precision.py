"""Accuracy of the Stein path's HIP kernels, per entry, against extended precision (tests/hp_reference.py).

Every assertion is a ratio |got - ref| / (EPS64 * bound) <= C for each entry on its own -- no global maximum -- where
``bound`` is the entry's own sum of absolute terms and ``ref`` is computed in long double FROM THE KERNEL'S OWN INPUTS
(the fp64 matrix it was given, padded view included).  C is derived by counting roundings (scores, Gram, the finish) or
measured at test time for the N-term sums: max(16, 8 x the ratio NumPy fp64 reaches on the same inputs), capped by the
derived worst case (hp.measured_constant).  Inputs: hp.scores / hp.qvec families (rows or bits scaled over twelve orders
of magnitude, rows at 1e9 ... 1e11 on tile, strip and band edges, zero rows, peaked / sparse / subnormal / signed q) and
near-deterministic networks through the score kernel.  Each check prints a line ``PREC|table row|case|worst GPU ratio|
oracle ratio|C`` (pytest -s); DESIGN.md section "Accuracy of the Stein path" is filled from those lines.
A case is left out only if long double is unavailable or the dense matrix does not fit; the reason is printed.
"""
import numpy as np
import pytest
import torch

import hp_reference as hp
from oracle import stein as os_
from tensornetworks_amd.bayesian_network import pack_network, synthetic_network

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def be():
    from tensornetworks_amd import backend
    return backend


def _need(n):
    why = hp.unavailable(n)
    if why:
        print("left out:", why)
        pytest.skip(why)


def _check(row, case, got, ref, bound, C, floor=0.0, oracle=None):
    """One per-entry assertion; the message names the worst entry.  C may be an array (per entry)."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    r = hp.ratio(got.reshape(np.shape(ref)) if np.ndim(ref) else got.reshape(-1), ref, bound, floor)
    w, at = hp.worst(r / C)
    g, _ = hp.worst(r)
    Cat = float(np.broadcast_to(C, r.shape)[at]) if np.ndim(C) else float(C)
    print(f"PREC|{row}|{case}|{g:.3g}|{'' if oracle is None else format(oracle, '.3g')}|{Cat:.3g}")
    assert w <= 1.0, f"{row} [{case}]: |got - ref| = {r[at]:.4g} x EPS64 x bound at entry {at}, allowed C = {Cat:.4g}"


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).to(dev)


def _dense_check(row, case, K, q, y_gpu, k2_gpu, qfam=None, rows=None, cols=None):
    """y (and ksd2 when every row is present) of a dense-form kernel against the long-double product of the SAME fp64
    matrix, with the constant measured from NumPy's fp64 product of it.  q, y_gpu: [N] or [m, N]."""
    K64 = K.cpu().numpy()                                   # (a padded view arrives as the matrix it holds)
    N = K64.shape[1]                                        # (terms per y_i: the columns given, where q is non-zero)
    q2 = np.atleast_2d(q)
    fams = [qfam] * len(q2) if not isinstance(qfam, (list, tuple)) else list(qfam)
    fl = np.array([hp.underflow_floor(f, N) for f in fams])
    y, Yb, k2, K2b = hp.matvec(K64, q2, rows=rows, cols=cols)
    qc = q2 if cols is None else q2[:, cols]
    yo = qc @ K64.T
    Cy_max, Ck_max = hp.dense_constants(N)
    oy = hp.worst(hp.ratio(yo, y, Yb, fl[:, None]))[0]
    Cy = hp.measured_constant(oy, Cy_max)
    yg = np.atleast_2d(y_gpu.detach().cpu().numpy())
    _check(row, case + " y", yg, y, Yb, Cy, fl[:, None], oracle=oy)
    if k2_gpu is not None and rows is None:
        Nr = K64.shape[0]
        ok2 = hp.worst(hp.ratio(np.einsum("bi,bi->b", q2, yo), k2, K2b, fl * Nr))[0]
        _check(row, case + " ksd2", k2_gpu.detach().cpu().numpy().reshape(-1), k2, K2b,
               hp.measured_constant(ok2, hp.dense_constants(max(N, Nr))[1]), fl * Nr, oracle=ok2)
    return y, Yb, k2, K2b


# ------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("n", [3, 6, 10])
def test_score_per_entry(be, dev, n):
    """bornvi_score_from_cpts on near-deterministic tables.  Bound per score 1 + |p'/p|, per p(x, z) the sum of its
    (non-negative) marginal terms; C derived (hp.score_constants): V factors and 2^h addends per probability, + 2; twice
    that for a score.  The kernel must zero exactly the rows the reference zeroes (|p| < 1e-12), which the cut network
    puts 1e-3 on either side of the threshold."""
    _need(n)
    nets = [hp.sharp_network(n, s) for s in (0, 1, 2)] + ([hp.cut_network()] if n == 3 else [])
    for k, (bn, lat, obs, x) in enumerate(nets):
        packed = pack_network(bn, lat, x)
        S, pxz = be.score_from_packed(packed, len(lat), dev)
        Sr, pr, Sb, zeroed = hp.score_packed(packed, len(lat))
        Cp, Cs = hp.score_constants(packed)
        kept, big = hp.surviving_rows(zeroed, Sr)
        print(f"score net {k} n={len(lat)}: {kept} of {1 << len(lat)} rows keep a score, {big} of them with |s| > 1e4")
        assert k == 3 or (kept >= (1 << len(lat)) // 4 and big >= 1)
        margin = np.abs(hp.to_f64(pr) / 1e-12 - 1.0)
        assert margin.min() > 1e-9, "a p(x, z) of the test network sits on the cut itself: the case decides nothing"
        Sg = S.cpu().numpy()
        assert np.array_equal(np.all(Sg == 0.0, axis=1) & (np.abs(pxz.cpu().numpy()) < 1e-12), zeroed), \
            f"net {k}: rows zeroed by the kernel differ from the reference's at {np.nonzero(np.all(Sg == 0, axis=1) != zeroed)[0][:8]}"
        _check("score_from_packed", f"n={n} net={k} pxz", pxz, pr, pr, Cp)
        _check("score_from_packed", f"n={n} net={k} S", S, Sr, Sb, Cs)
    if n == 3:
        assert zeroed[0b111] and not zeroed[0b110]


# ------------------------------------------------------------------------------------------------ Gram
def _bn_sharp_scores(be, dev, n, seed):
    """Scores of a near-deterministic network from the score kernel (the whole chain CPT -> S -> K_p); a useful share of
    the rows must survive the 1e-12 cut and some must carry scores above 1e4."""
    bn, lat, obs, x = hp.sharp_network(n, seed)
    S, pxz = be.score_from_packed(pack_network(bn, lat, x), n, dev)
    kept = int((S != 0).any(dim=1).sum())
    big = int((S.abs().max(dim=1).values > 1e4).sum())
    print(f"bn-sharp n={n} seed={seed}: {kept} of {1 << n} rows keep a score, {big} of them with |s| > 1e4")
    assert kept >= (1 << n) // 8 and big >= 1
    return S, pxz


@pytest.mark.parametrize("ls", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("n", [1, 2, 5, 8, 9])
def test_gram_full_per_entry(be, dev, n, ls):
    """bornvi_stein_gram_build_rows_ld (full, rows=, padded ld=, out=) and bornvi_stein_kp_pairs: every entry within
    C = 3n + d + 12 units of EPS64 * B_ij (hp.gram_constant: n-term dot of three-term addends 3n; a^d as d products or
    one table product; 12 once per entry and operand), B_ij = a^d sum_b (|S_ib S_jb| + |c_b| (|S_ib| + |S_jb|) + 2 |c_b|).
    n <= 7 runs the vector kernel, n >= 8 the matrix-core one."""
    _need(n)
    N = 1 << n
    d = hp.popcount(np.arange(N)[:, None] ^ np.arange(N)[None, :])
    C = hp.gram_constant(n, d)
    fams = list(hp.SCORE_FAMILIES) + (["bn-sharp"] if n >= 5 else [])
    for fam in fams:
        S = _bn_sharp_scores(be, dev, n, 3)[0] if fam == "bn-sharp" else _t(hp.scores(fam, n, 1), dev)
        Sn = S.cpu().numpy()
        K, B = hp.gram_terms(Sn, n, ls)
        orc = hp.worst(hp.ratio(os_.gram_closed_form(Sn, n, ls), K, B))[0]
        case = f"n={n} l={ls} S={fam}"
        Kg = be.stein_gram(S, n, ls)
        _check("stein_gram", case + " full", Kg, K, B, C, oracle=orc)
        r0, r1 = N // 3, N - N // 5
        if r1 > r0:
            _check("stein_gram", case + " rows=", be.stein_gram(S, n, ls, rows=(r0, r1)), K[r0:r1], B[r0:r1], C[r0:r1])
        Kp = be.stein_gram(S, n, ls, ld=N + 32)
        assert Kp.stride(0) == N + 32
        _check("stein_gram", case + " ld=", Kp, K, B, C)
        buf = torch.zeros((N + 3, N + 6), dtype=torch.float64, device=dev)
        be.stein_gram(S, n, ls, out=buf[2:2 + N, :N])
        _check("stein_gram", case + " out=", buf[2:2 + N, :N], K, B, C)
        assert not buf[:2].any() and not buf[2 + N:].any() and not buf[:, N:].any()
        rng = np.random.default_rng(n)
        zi = np.concatenate([rng.integers(0, N, 300), np.arange(N)[:64]])
        zj = np.concatenate([rng.integers(0, N, 300), np.arange(N)[:64]])
        out = be.stein_kp_pairs(n, ls, torch.as_tensor(zi, device=dev), torch.as_tensor(zj, device=dev),
                                S[torch.as_tensor(zi, device=dev)].contiguous(), S[torch.as_tensor(zj, device=dev)].contiguous())
        _check("stein_kp_pairs", case, out, K[zi, zj], B[zi, zj], C[zi, zj])


@pytest.mark.parametrize("n,ls,fams", [(11, 0.3, ("wide", "spiky")), (11, 1.0, hp.SCORE_FAMILIES), (11, 3.0, ("wide", "spiky")),
                                       (13, 1.0, ("wide", "spiky", "wide-cols")), (14, 1.0, ("wide", "spiky")),
                                       (14, 3.0, ("wide-cols", "bn-sharp"))])
def test_gram_sampled_rows_per_entry(be, dev, n, ls, fams):
    """96 rows (block, strip and band edges plus random ones) x ALL columns of the matrix-core Gram at sizes where the
    whole matrix in long double is out of reach; same bound and C as test_gram_full_per_entry; dense and padded pitch."""
    _need(n)
    N = 1 << n
    rows = hp.sample_rows(n, 1)
    d = hp.popcount(rows[:, None] ^ np.arange(N)[None, :])
    C = hp.gram_constant(n, d)
    for fam in fams:
        S = _bn_sharp_scores(be, dev, n, 3)[0] if fam == "bn-sharp" else _t(hp.scores(fam, n, 1), dev)
        Sn = S.cpu().numpy()
        K, B, _ = hp.gram_bound(Sn, n, ls, rows=rows)
        Kg = be.stein_gram(S, n, ls, ld=be.gram_ld(n))
        _check("stein_gram", f"n={n} l={ls} S={fam} sampled", Kg[torch.as_tensor(rows, device=dev)], K, B, C)
        zi = np.repeat(rows[:16], 64)
        zj = np.random.default_rng(n).integers(0, N, len(zi))
        ti, tj = torch.as_tensor(zi, device=dev), torch.as_tensor(zj, device=dev)
        out = be.stein_kp_pairs(n, ls, ti, tj, S[ti].contiguous(), S[tj].contiguous())
        ri = np.searchsorted(rows, zi)
        _check("stein_kp_pairs", f"n={n} l={ls} S={fam}", out, K[ri, zj], B[ri, zj], C[ri, zj])
        del Kg


# ------------------------------------------------------------------------------------------------ contractions
def _all_q(n, seed=1):
    return [(f, hp.qvec(f, n, seed)) for f in hp.Q_FAMILIES]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 10])
def test_quadform_single_per_entry(be, dev, n):
    """bornvi_stein_quadform_ld, B = 1 (the HBM-bound GEMV): y_i within C of EPS64 * sum_j |K_ij| |q_j|, ksd2 within C of
    EPS64 * sum_ij |q_i| |K_ij| |q_j|; C measured (module docstring)."""
    _need(n)
    for fam in ("wide", "spiky", "zero-rows"):
        K = be.stein_gram(_t(hp.scores(fam, n, 2), dev), n, 1.0)
        for qf, q in _all_q(n):
            k2, Y = be.stein_quadform(K, _t(q, dev), n)
            _dense_check("stein_quadform B=1", f"n={n} S={fam} q={qf}", K, q, Y[0], k2, qf)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n,B", [(8, 2), (8, 5), (8, 129), (10, 2), (10, 5), (10, 129), (12, 2), (12, 5), (12, 129)])
def test_quadform_batched_per_entry(be, dev, n, B, padded):
    """The batched matrix-core form (v_mfma_f64_16x16x4, kernels_batched.hip): Q stacks one family per row, so rows of
    very different scale share MFMA tiles; dense K and the trainer's padded K; bounds as for B = 1, per entry of Y."""
    _need(n)
    N = 1 << n
    fam = ("wide", "spiky", "wide-cols")[B % 3]
    S = _t(hp.scores(fam, n, 4), dev)
    K = be.stein_gram(S, n, 1.0, ld=N + 32) if padded else be.stein_gram(S, n, 1.0)
    fams = [hp.Q_FAMILIES[b % len(hp.Q_FAMILIES)] for b in range(B)]
    Q = np.stack([hp.qvec(f, n, 10 + b) for b, f in enumerate(fams)])
    k2, Y = be.stein_quadform(K, _t(Q, dev), n)
    _dense_check("stein_quadform batched", f"n={n} B={B} S={fam} {'padded' if padded else 'dense'}", K, Q, Y, k2, fams)


@pytest.mark.parametrize("n,padded", [(4, False), (8, False), (9, False), (9, True), (11, False), (11, True), (12, False),
                                      (13, True), (14, False), (14, True)])
def test_quadform_sym_per_entry(be, dev, n, padded):
    """bornvi_stein_quadform_sym_ld: the full-matrix regime (dense K below n = 14), the band kernel at ld = 2^n (n = 14)
    and at the padded pitch 2^n + 32 (n = 9 ... 14): each y_i is a row-strip sum PLUS transposed partials, which the
    strip-sparse, band-sparse and odd-index q separate."""
    _need(n)
    N = 1 << n
    for fam in ("wide", "spiky"):
        S = _t(hp.scores(fam, n, 2), dev)
        K = be.stein_gram(S, n, 1.0, ld=N + 32) if padded else be.stein_gram(S, n, 1.0)
        qs = _all_q(n)
        ys, ks = [], []
        for qf, q in qs:
            k2, y = be.stein_quadform_sym(K, _t(q, dev), n)
            ys.append(y)
            ks.append(k2)
        _dense_check("stein_quadform_sym", f"n={n} S={fam} {'padded' if padded else 'dense'}", K, np.stack([q for _, q in qs]),
                     torch.stack(ys), torch.cat(ks), [f for f, _ in qs])


@pytest.mark.parametrize("n", [9, 12])
@pytest.mark.parametrize("world", [1, 3, 8])
def test_shards_assembled_per_entry(be, dev, n, world):
    """bornvi_stein_quadform_rows (row shard) and bornvi_stein_quadform_sym_pairs_ld (strip-pair shard): the result
    assembled from W ranks' messages, judged like the unsharded one."""
    _need(n)
    N = 1 << n
    for fam in ("wide", "spiky"):
        S = _t(hp.scores(fam, n, 2), dev)
        K = be.stein_gram(S, n, 1.0)
        qs = _all_q(n)
        ys_r, ks_r, ys_p, ks_p = [], [], [], []
        for qf, q in qs:
            qt = _t(q, dev)
            cut = [N * w // world for w in range(world + 1)]
            msgs = [be.stein_quadform_rows(be.stein_gram(S, n, 1.0, rows=(cut[w], cut[w + 1])), cut[w], cut[w + 1], qt, n)
                    for w in range(world)]
            ys_r.append(torch.cat([m[:-1] for m in msgs]))
            ks_r.append(torch.stack([m[-1] for m in msgs]).sum().reshape(1))
            total = torch.zeros(N + 1, dtype=torch.float64, device=dev)
            for rank in range(world):
                (pa, pb), (l0, l1), (h0, h1) = be.sym_pair_shard(n, rank, world)
                K_lo = be.stein_gram(S, n, 1.0, rows=(l0, l1)) if l1 > l0 else None
                K_hi = be.stein_gram(S, n, 1.0, rows=(h0, h1)) if h1 > h0 else None
                total += be.stein_quadform_sym_pairs(K_lo, K_hi, pa, pb, qt, n)
            ys_p.append(total[:-1])
            ks_p.append(total[-1:])
        Q = np.stack([q for _, q in qs])
        fams = [f for f, _ in qs]
        _dense_check("stein_quadform_rows", f"n={n} W={world} S={fam}", K, Q, torch.stack(ys_r), torch.cat(ks_r), fams)
        _dense_check("stein_quadform_sym_pairs", f"n={n} W={world} S={fam}", K, Q, torch.stack(ys_p), torch.cat(ks_p), fams)


def _kron_check(be, dev, case, S, Sn, q, qf, n, ls):
    k2, y = be.stein_matvec_kron(S, _t(q, dev), n, ls)
    yr, Yb, k2r, K2b = hp.kron(Sn, q, n, ls)
    N = 1 << n
    fl = hp.underflow_floor(qf, N)
    Cy_max, Ck_max = hp.kron_constant(n)
    yo = os_.stein_matvec_kron(Sn, q, n, ls)
    oy = hp.worst(hp.ratio(yo, yr, Yb, fl * n))[0]
    ok2 = hp.worst(hp.ratio(q @ yo, k2r, K2b, fl * n * N))[0]
    _check("stein_matvec_kron", case + " y", y, yr, Yb, hp.measured_constant(oy, Cy_max), fl * n, oracle=oy)
    _check("stein_matvec_kron", case + " ksd2", k2, k2r, K2b, hp.measured_constant(ok2, Ck_max), fl * n * N, oracle=ok2)
    return k2, y, k2r, K2b


@pytest.mark.parametrize("ls", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("n", [2, 5, 9, 12, 14, 16])
def test_kron_per_entry(be, dev, n, ls):
    """bornvi_stein_matvec_kron against the recipe in long double and the recipe's OWN term bound (|q|, |S|, every
    subtraction an addition); a -> 1 at length_scale 3 is where u and its flip nearly cancel."""
    _need(n)
    for fam in ("wide", "spiky", "wide-cols", "zero-rows"):
        Sn = hp.scores(fam, n, 3)
        S = _t(Sn, dev)
        for qf, q in _all_q(n):
            _kron_check(be, dev, f"n={n} l={ls} S={fam} q={qf}", S, Sn, q, qf, n, ls)


# ------------------------------------------------------------------------------------------------ the finish
@pytest.mark.parametrize("want_dldq", [False, True])
@pytest.mark.parametrize("n,n_shift", [(4, 1), (4, 7), (12, 1), (12, 7)])
def test_grad_finish_per_entry(be, dev, n, n_shift, want_dldq):
    """bornvi_ksd_grad_finish: loss, dL/dq (derived C = 3: sqrt, reciprocal, product) and the parameter-shift dots
    (bound sum_z |y_z| |q+_z - q-_z| / (2 loss), C measured), on the loss-by-dot path (no dL/dq) and the separate-pass
    path; ksd2 = -1e-13, 0, 1e-13, 1e-12 and its two neighbours: the clamp is taken on the reference's side."""
    N = 1 << n
    rng = np.random.default_rng(n + n_shift)
    y = hp.scores("wide", n, 5)[:, 0].copy()
    shifted = rng.dirichlet(np.full(N, 0.3), 2 * n_shift)
    shifted[1] = shifted[0] * (1 + 1e-9)                     # a nearly cancelling pair
    for k2 in hp.KSD2_EDGE_VALUES:
        ref = hp.finish(shifted, y, np.array([k2]))
        loss, grad, dldq = be.ksd_grad_finish(n, _t(shifted, dev), n_shift, _t(y, dev), _t([k2], dev), want_dldq=want_dldq)
        case = f"n={n} n_shift={n_shift} ksd2={k2!r} {'separate' if want_dldq else 'loss_by_dot'}"
        inv = 0.0 if k2 < 1e-12 else 1.0 / np.sqrt(max(k2, 1e-12))
        go = ((shifted[0::2] - shifted[1::2]) @ y) * (0.5 * inv)
        og = hp.worst(hp.ratio(go, ref["grad"], ref["grad_bound"]))[0]
        _check("ksd_grad_finish", case + " loss", loss, ref["loss"], ref["loss"], hp.FINISH_DERIVED_C)
        _check("ksd_grad_finish", case + " dots", grad, ref["grad"], ref["grad_bound"],
               hp.measured_constant(og, N + 2 + hp.FINISH_DERIVED_C), oracle=og)
        if want_dldq:
            _check("ksd_grad_finish", case + " dLdq", dldq, ref["dldq"], ref["dldq_bound"], hp.FINISH_DERIVED_C)
        if k2 < 1e-12:
            assert loss.item() == 1e-6 and not grad.any() and (dldq is None or not dldq.any())


# ------------------------------------------------------------------------------------------------ at the posterior
@pytest.mark.parametrize("n,sharp", [(8, False), (8, True), (10, False), (10, True), (12, False)])
def test_every_form_at_the_posterior(be, dev, n, sharp):
    """q = p(z | x) of the network the scores come from, through every form of the contraction.
    sharp = False (synthetic_network, no row under the 1e-12 cut -- asserted): the cancellation case.  K_p q is rounding
    and q^T K_p q is what the trainer takes the square root of: |ksd2| <= C EPS64 K2b for every form, C the form's
    measured constant (test_hp_reference.py shows NumPy fp64 at 0.1 ... 0.3 of EPS64 K2b there, the long-double value of
    the fp64 matrix included).  sharp = True is NOT a cancellation case: rows under the cut get a zero score
    (stein_utils.py:126-128) and still carry posterior mass, so ksd2 is O(1) or larger; it is the posterior as the
    trainer meets it on such a network, and the number of surviving rows is printed.
    In both cases each form's ksd2 lies within its own C of its own long-double reference, and any two forms agree
    within the sum of their bounds; between a dense form and the matrix-free one the fp64 rounding of K_p's entries is
    added: (3n + n + 12) EPS64 sum_ij |q_i| B_ij |q_j| (hp.gram_constant at d = n)."""
    _need(n)
    N = 1 << n
    bn, lat, obs, x = hp.sharp_network(n, 5) if sharp else synthetic_network(n, 5)
    S, pxz = be.score_from_packed(pack_network(bn, lat, x), n, dev)
    zero_rows = int((~(S != 0).any(dim=1)).sum())
    print(f"posterior n={n} sharp={sharp}: {N - zero_rows} of {N} rows keep a score")
    assert (zero_rows > 0) == sharp
    post = (pxz / pxz.sum()).contiguous()
    q = post.cpu().numpy()
    Sn = S.cpu().numpy()
    K = be.stein_gram(S, n, 1.0)
    forms = {}

    def dense(name, Kx, k2, y, stack=1):
        qq, ff = (q, "posterior") if stack == 1 else (np.stack([q] * stack), ["posterior"] * stack)
        yr, Yb, k2r, K2b = _dense_check("posterior", f"n={n} sharp={sharp} {name}", Kx, qq, y, k2, ff)
        k2r, K2b = np.atleast_1d(k2r)[0], float(np.atleast_1d(K2b)[0])
        K64 = Kx.cpu().numpy()
        C = hp.measured_constant(hp.worst(hp.ratio(q @ (K64 @ q), k2r, K2b))[0], hp.dense_constants(N)[1])
        forms[name] = (float(k2.reshape(-1)[0]), C * hp.EPS64 * K2b, k2r, C, K2b)

    k2, Y = be.stein_quadform(K, post, n)
    dense("quadform", K, k2, Y[0])
    k2b, Y2 = be.stein_quadform(K, torch.stack([post, post]), n)
    dense("batched", K, k2b, Y2, stack=2)
    k2s, ysym = be.stein_quadform_sym(K, post, n)
    dense("sym", K, k2s, ysym)
    if n >= 9:
        Kp = be.stein_gram(S, n, 1.0, ld=N + 32)
        k2p, yp = be.stein_quadform_sym(Kp, post, n)
        dense("sym padded", Kp, k2p, yp)
    k2k, yk, k2kr, K2bk = _kron_check(be, dev, f"n={n} sharp={sharp} posterior", S, Sn, q, "posterior", n, 1.0)
    Ck = hp.measured_constant(hp.worst(hp.ratio(q @ os_.stein_matvec_kron(Sn, q, n, 1.0), k2kr, K2bk))[0], hp.kron_constant(n)[1])
    forms["kron"] = (k2k.item(), Ck * hp.EPS64 * float(K2bk), k2kr, Ck, float(K2bk))
    _, B, _ = hp.gram_bound(Sn, n, 1.0)
    qa = np.abs(q).astype(np.longdouble)
    entry = float(qa @ (B @ qa)) * hp.EPS64 * float(hp.gram_constant(n, n))
    names = list(forms)
    for i, a in enumerate(names):
        got, bound, ref, C, K2b = forms[a]
        print(f"PREC|posterior |ksd2||n={n} sharp={sharp} {a}|{abs(got) / (hp.EPS64 * K2b):.3g}|{abs(float(ref)) / (hp.EPS64 * K2b):.3g}|{C:.3g}")
        assert abs(got - float(ref)) <= bound
        if not sharp:
            assert abs(got) <= bound, f"|ksd2| at the posterior, {a}: {abs(got) / (hp.EPS64 * K2b):.4g} x EPS64 x K2b, allowed C = {C:.4g}"
        for b in names[i + 1:]:
            slack = entry if (a == "kron") != (b == "kron") else 0.0
            assert abs(got - forms[b][0]) <= bound + forms[b][1] + slack, \
                f"ksd2 at the posterior: {a} {got!r} vs {b} {forms[b][0]!r}, bounds {bound:.3g} + {forms[b][1]:.3g} + {slack:.3g}"


# ------------------------------------------------------------------------------------------------ n = 16, once
def test_full_size_once(be, dev):
    """n = 16, the 32 GiB dense K_p: 96 sampled rows x all columns of the Gram; the B = 1 GEMV and the symmetric band
    kernel on a band-sparse q (full long-double reference of y and ksd2 from the 256 columns that matter) and on a
    Dirichlet q (y at the sampled rows)."""
    n = 16
    _need(n)
    N = 1 << n
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 8 * N * N + (2 << 30):
        why = f"the dense matrix does not fit: n = 16 needs {8 * N * N / 2**30:.0f} GiB, {free / 2**30:.0f} GiB free"
        print("left out:", why)
        pytest.skip(why)
    Sn = hp.scores("wide", n, 1)
    S = _t(Sn, dev)
    K = be.stein_gram(S, n, 1.0)
    rows = hp.sample_rows(n, 1)
    tr = torch.as_tensor(rows, device=dev)
    Kr, B, _ = hp.gram_bound(Sn, n, 1.0, rows=rows)
    d = hp.popcount(rows[:, None] ^ np.arange(N)[None, :])
    Ks = K[tr]
    _check("stein_gram", "n=16 l=1.0 S=wide sampled", Ks, Kr, B, hp.gram_constant(n, d))
    qb, qd = hp.qvec("band", n, 1), hp.qvec("dirichlet", n, 1)
    Kband = K[:, N - 256:].contiguous()
    for name, fn in (("stein_quadform B=1", lambda q: (lambda r: (r[0], r[1][0]))(be.stein_quadform(K, q, n))),
                     ("stein_quadform_sym", lambda q: be.stein_quadform_sym(K, q, n))):
        k2, y = fn(_t(qb, dev))
        _dense_check(name, "n=16 S=wide q=band", Kband, qb, y, k2, "band", cols=np.arange(N - 256, N))
        k2, y = fn(_t(qd, dev))
        _dense_check(name, "n=16 S=wide q=dirichlet sampled rows", Ks, qd, y[tr], None, "dirichlet", rows=rows)
