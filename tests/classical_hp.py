"""Extended-precision references and derived per-entry bounds of the table-family kernels: bornvi_born_table_probs /
bornvi_born_table_vjp (kernels_born_table.hip) and bornvi_reinforce_step (kernels_reinforce.hip).  Test infrastructure,
shared by test_classical_precision_host.py (CPU) and test_gpu_classical_precision.py (MI355X); not under test.

Every reference takes the float32 inputs exactly as given and runs in x87 long double (hp_reference.LD).  Every
``*_check`` returns, per output, the per-entry ratio |got - ref| / allowed; a correct kernel stays at or below 1.
``allowed`` is built from constants counted on the kernel's own chains -- every rounding on the longest path counts as
one whole unit of EPS64 = 2^-52 (a correctly rounded operation errs by half a unit, the device's exp and log by at most
one) -- and the chain lengths come from the geometry the kernels use (bt_geom / rf_geom, restated here).  Nothing is
fitted to a measurement.

Chains.  A block sum is the per-thread terms, 6 butterfly levels and the 4 wave totals; every row reduction is two such
sums, one over a workgroup's chunk and one over the row's G partials:
    L(N) = T + 10 + ceil(G / 256) + 10,   T = 4 ceil(chunk / 1024) (the float4 path; the scalar path has fewer).
  q:  mode 1  |w| / S: the S chain and the quotient,                      C_Q = L + 1;
      mode 0  exp(w - M) / S: the exp, the quotient, and per link of the S chain one max-shift combine
              S exp(M - m) + s (exp, product, sum),                       C_Q = 3 L + 2.
      w - M is exact in float64 for the inputs used here (exact_differences asserts it).
  H:  log, product, the chain; then one float32 rounding,                 C_H = L + 2.
  dL/dw:  g_i = float32(y_i a) + lambda (log c_i + [q_i >= 1e-10]): log, sum, product, sum (4); g_i - c and the product
      with q_i (2): C_1 = 6 (mode 0); mode 1 divides by sum |w| instead: its chain, the reciprocal and two products more,
      C_1 = 6 + L + 3.  c = sum_j q_j g_j: g_j (4), the product (1), the chain: C_c = L + 5.  One float32 rounding.
  REINFORCE: T_mean = ceil(chunk_s / 256) + 10 + ceil(G_s / 256) + 10 + 2 (raw_b itself, the division by B); the loss
      sums ceil(chunk_z / 256) + 10 + ceil(G_z / 256) + 10 partial terms, each log c_i S_i 2^-e (log, conversion, product)
      and is divided by B: T_loss = that + 4.
"""
import functools

import numpy as np
import torch

import hp_reference as hp
from hp_reference import EPS64, LD, to_f64

F32_HALF_ULP = 2.0 ** -24
F32_MIN_NORMAL = 2.0 ** -126
CLAMP32 = np.float32(1e-10)                   # BT_CLAMP; also the float32 q_floor of the REINFORCE step
THREADS = 256
BT_PER_WG, RF_SAMPLES_PER_WG, RF_OUTCOMES_PER_WG, MAX_WG = 4096, 1024, 4096, 1024


def unavailable():
    """None, or why the module is skipped: the references need a 64-bit mantissa (as hp_reference.unavailable)."""
    if hp.HAVE_LONGDOUBLE:
        return None
    return f"long double unavailable (np.longdouble eps {np.finfo(LD).eps:.3g})"


def ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


def allowed_ratio(got, ref, allowed):
    """|got - ref| / allowed per entry through hp.ratio (allowed == 0: only got == ref passes)."""
    return hp.ratio(got, ref, np.asarray(allowed, dtype=LD) / LD(EPS64))


# ------------------------------------------------------------------------------------------------ geometry
def _cdiv(a, b):
    return -(-a // b)


def bt_geom(N):
    """(chunk, G) of kernels_born_table.hip: bt_geom."""
    G = min(MAX_WG, max(1, _cdiv(N, BT_PER_WG)))
    chunk = (_cdiv(N, G) + 3) & ~3
    return chunk, _cdiv(N, chunk)


def rf_geom(count, per_wg):
    """(chunk, G) of kernels_reinforce.hip: rf_geom."""
    G = min(MAX_WG, max(1, _cdiv(count, per_wg)))
    chunk = _cdiv(count, G)
    return chunk, _cdiv(count, chunk)


def _two_level(per_thread, G):
    return per_thread + 10 + _cdiv(G, THREADS) + 10


def table_constants(n, mode):
    chunk, G = bt_geom(1 << n)
    L = _two_level(4 * _cdiv(chunk, 4 * THREADS), G)
    return {"L": L, "G": G, "chunk": chunk, "q": float(3 * L + 2 if mode == 0 else L + 1), "H": float(L + 2),
            "g1": float(6 if mode == 0 else 9 + L), "gc": float(L + 5)}


def reinforce_constants(n, B):
    cs, Gs = rf_geom(B, RF_SAMPLES_PER_WG)
    cz, Gz = rf_geom(1 << n, RF_OUTCOMES_PER_WG)
    return {"T_mean": float(_two_level(_cdiv(cs, THREADS), Gs) + 2), "T_loss": float(_two_level(_cdiv(cz, THREADS), Gz) + 4),
            "Gs": Gs, "Gz": Gz}


# ------------------------------------------------------------------------------------------------ table inputs
TABLE_SHAPES = [(n, 3) for n in (1, 2, 3, 12, 13, 14)] + [(21, 1)]
TABLE_FAMILIES = [(0, "random"), (0, "spread"), (0, "edge"), (1, "random"), (1, "spread"), (1, "zeros"), (1, "edge")]
KSD2 = np.array([2.5, 1e-13, 0.7])            # row 1: the clamp at 1e-12 is active
LAMBDA = 0.013
# (y present, ksd2 present, lambda): both terms; KSD alone; y as dL/dq itself with and without entropy; entropy alone
VJP_CONFIGS = [(True, True, LAMBDA), (True, True, 0.0), (True, False, LAMBDA), (True, False, 0.0), (False, False, LAMBDA)]
EDGE_AT = (5, 6, 7)                           # columns of the edge rows: one float32 ulp below the clamp, at it, above it
EDGE_TARGETS = (np.nextafter(CLAMP32, np.float32(0)), CLAMP32, np.nextafter(CLAMP32, np.float32(1)))


def _edge_row_abs(N, rng):
    """|w| / sum |w| = EDGE_TARGETS exactly at EDGE_AT once rounded to float32: sum |w| is 2^10 to 2^-40 relative.  The
    other entries are multiples of 2^-16 (their sum is exact); two closing entries bring the total to 2^10."""
    w = (rng.integers(1, 1 << 12, N).astype(np.float64) / (1 << 16) * (1024.0 / N)).astype(np.float32)
    w[::5] *= -1.0
    if N < 16:
        return w
    for c, t in zip(EDGE_AT, EDGE_TARGETS):
        w[c] = np.float32(np.float64(t) * 1024.0)
    w[1] = w[2] = 0.0
    rest = LD(1024.0) - np.abs(ld(w)).sum()
    w[1] = np.float32(rest)
    if ld(w[1]) > rest:                          # round down: what is left for the second entry is not negative
        w[1] = np.nextafter(w[1], np.float32(0))
    w[2] = np.float32(rest - ld(w[1]))
    assert w[1] > 0 and w[2] >= 0
    return w


def table_rows(n, rows, mode, family, seed=0):
    """float32 [rows, 2^n] raw parameters.  'random', 'spread' and 'zeros' are test_gpu_classical.make_rows' (on the CPU
    generator); 'edge': mode 1 rows whose q holds the float32 clamp 1e-10, its lower and its upper neighbour exactly
    (N >= 16); mode 0 random logits with a band 20 ... 26 below the maximum (q around 1e-10) and -inf at 3, 4 and N - 1."""
    N = 1 << n
    gen = torch.Generator().manual_seed(1000 * n + 10 * mode + len(family) + 7919 * seed)
    if family == "random":
        w = (torch.randn(rows, N, generator=gen) * 2.0).numpy()
    elif family == "spread":
        w = (torch.rand(rows, N, generator=gen) * 200.0 - 200.0).numpy()
        if mode == 1:
            w = np.abs(w)
    elif family == "zeros":
        w = torch.randn(rows, N, generator=gen).numpy()
        w[:, ::3] = 0.0
    elif family == "edge":
        rng = np.random.default_rng([n, mode, seed, 5])
        if mode == 1:
            w = np.stack([_edge_row_abs(N, rng) for _ in range(rows)])
        else:
            w = (rng.standard_normal((rows, N)) * 2.0).astype(np.float32)
            band = rng.random((rows, N)) < 0.25
            w[band] = (w.max() - 20.0 - 6.0 * rng.random(int(band.sum()))).astype(np.float32)
            if N >= 8:
                w[:, [3, 4, N - 1]] = -np.inf
    else:
        raise ValueError(family)
    return np.ascontiguousarray(w, dtype=np.float32)


def vjp_inputs(n, rows, seed=0):
    """(y float64 [rows, 2^n], ksd2 float64 [rows])."""
    rng = np.random.default_rng([n, rows, seed, 11])
    return rng.standard_normal((rows, 1 << n)), KSD2[:rows].copy()


def exact_differences(w):
    """Every difference of two finite entries of a row is exact in float64: all are multiples of 2^lo, below 2^(lo + 53)."""
    for r in np.asarray(w, dtype=np.float64):
        f = r[np.isfinite(r) & (r != 0.0)]
        if f.size:
            lo = int(np.frexp(np.abs(f).min())[1]) - 24
            hi = int(np.frexp(max(f.max() - f.min(), np.abs(f).max()))[1])
            assert hi - lo <= 53, (hi, lo)


# ------------------------------------------------------------------------------------------------ table forward
def forward_reference(w, mode):
    """q* [rows, N] and S* [rows] in long double."""
    wl = ld(w)
    if mode == 0:
        exact_differences(w)
        with np.errstate(all="ignore"):
            e = np.exp(wl - wl.max(axis=1, keepdims=True))
    else:
        e = np.abs(wl)
    S = e.sum(axis=1, keepdims=True)
    return e / S, S[:, 0]


@functools.lru_cache(maxsize=None)
def forward_case(n, rows, mode, family):
    """(w, (q*, S*)) of one case, computed once per process and shared (read-only) by the tests that need it."""
    w = table_rows(n, rows, mode, family)
    ref = forward_reference(w, mode)
    for a in (w,) + ref:
        a.setflags(write=False)
    return w, ref


def _tie_distance(q_star, other):
    """Distance of q* from the float32 rounding tie between float32(q*) and its neighbour `other`."""
    r = q_star.astype(np.float32)
    return np.abs((ld(r) + ld(other)) / 2 - q_star)


def q32_ratio(q32, q_star, c_q):
    """0 where q32 == float32(q*).  Where q32 is the neighbour of float32(q*) the kernel's float64 value lay beyond the
    tie between the two: ratio = (distance of q* from that tie) / (C_Q EPS64 q*).  Anything else: inf.  Below the float32
    normal range: |q32 - q*| / 2^-126."""
    q32 = np.asarray(q32, dtype=np.float32)
    r = q_star.astype(np.float32)                    # one correctly rounded conversion, gradual underflow
    delta = q_star * LD(c_q * EPS64)
    other = np.nextafter(r, q32)
    need = _tie_distance(q_star, other)
    rr = to_f64(need / np.where(delta > 0, delta, LD(1)))
    ratio = np.where(q32 == r, 0.0, np.where((other == q32) & (to_f64(delta) > 0), rr, np.inf))
    sub = (to_f64(q_star) < F32_MIN_NORMAL) & (q_star != 0)      # (an exact 0 -- a -inf logit, w = 0 -- stays exact)
    return np.where(sub, to_f64(np.abs(ld(q32) - q_star)) / F32_MIN_NORMAL, ratio)


def tie_exceptions(q_star, c_q):
    """How many entries of q* the tie exception of q32_ratio can excuse (from the reference alone)."""
    r = q_star.astype(np.float32)
    d = np.minimum(_tie_distance(q_star, np.nextafter(r, np.float32(np.inf))),
                   _tie_distance(q_star, np.nextafter(r, np.float32(-np.inf))))
    return int(np.count_nonzero((d <= q_star * LD(c_q * EPS64)) & (to_f64(q_star) >= F32_MIN_NORMAL)))


def underflow_mode(q32, q_star):
    """'gradual', 'flushed' or 'none': what the device's float64 -> float32 conversion did below the normal range."""
    zone = (to_f64(q_star) < F32_MIN_NORMAL) & (to_f64(q_star) > 2.0 ** -149)
    if not zone.any():
        return "none"
    return "gradual" if (np.asarray(q32)[zone] != 0).any() else "flushed"


def entropy_reference(q32):
    """(H*, allowed less C_H) from the kernel's own q32: H* = -sum q log max(q, 1e-10f), sum |q log c|."""
    q32 = np.asarray(q32, dtype=np.float32)
    t = ld(q32) * np.log(ld(np.maximum(q32, CLAMP32)))
    return -t.sum(axis=1), np.abs(t).sum(axis=1)


def forward_check(w, mode, q32, q64, H, ref=None):
    """-> {'q': (ratio, index), 'H': (ratio, index)} and asserts q64 == q32.double() bitwise."""
    n = int(w.shape[1]).bit_length() - 1
    C = table_constants(n, mode)
    q_star = (ref or forward_reference(w, mode))[0]
    q32, q64 = np.asarray(q32, dtype=np.float32), np.asarray(q64, dtype=np.float64)
    assert np.array_equal(q64.view(np.int64), q32.astype(np.float64).view(np.int64)), "q64 is not q32's exact upcast"
    out = {"q": hp.worst(q32_ratio(q32, q_star, C["q"]))}
    if H is not None:
        h_star, terms = entropy_reference(q32)
        chain = LD(C["H"] * EPS64) * terms
        out["H"] = hp.worst(allowed_ratio(H, h_star, chain + LD(F32_HALF_ULP) * (np.abs(h_star) + chain)))
    return out


# ------------------------------------------------------------------------------------------------ table VJP
def ksd_scale(ksd2, rows):
    """a = 1 / sqrt(ksd2), 0 under the clamp, 1 without ksd2: correctly rounded float64 operations, as the device's."""
    if ksd2 is None:
        return np.ones(rows)
    with np.errstate(all="ignore"):
        return np.where(ksd2 < 1e-12, 0.0, 1.0 / np.sqrt(ksd2))


def vjp_reference(w, q64, y, ksd2, lam, mode):
    """(dL/dw* [rows, N], allowed [rows, N]) from the kernel's own q64."""
    rows, N = w.shape
    C = table_constants(N.bit_length() - 1, mode)
    g = ld(np.zeros((rows, N)))
    if y is not None:
        g = ld((y * ksd_scale(ksd2, rows)[:, None]).astype(np.float32))
    if lam != 0.0:
        qf = np.asarray(q64).astype(np.float32)
        g = g + LD(lam) * (np.log(ld(np.maximum(qf, CLAMP32))) + ld(qf >= CLAMP32))
    ql = ld(q64)
    c = (ql * g).sum(axis=1, keepdims=True)
    inner = LD(C["g1"]) * (np.abs(g) + np.abs(c)) + LD(C["gc"]) * (ql * np.abs(g)).sum(axis=1, keepdims=True)
    if mode == 0:
        out, chain = ql * (g - c), LD(EPS64) * ql * inner
    else:
        sw = np.abs(ld(w)).sum(axis=1, keepdims=True)
        sg = ld(np.sign(w))
        out, chain = sg * (g - c) / sw, LD(EPS64) * np.abs(sg) * inner / sw
    rounding = np.where(to_f64(np.abs(out)) < F32_MIN_NORMAL, LD(F32_MIN_NORMAL), LD(F32_HALF_ULP) * (np.abs(out) + chain))
    return out, np.where(chain == 0, LD(0), chain + rounding)


def vjp_check(w, q64, y, ksd2, lam, mode, grad, loss=None):
    ref, allowed = vjp_reference(w, q64, y, ksd2, lam, mode)
    if loss is not None:
        want = np.sqrt(np.where(ksd2 < 1e-12, 1e-12, ksd2))
        assert np.array_equal(np.asarray(loss).view(np.int64), want.view(np.int64)), ("loss", loss, want)
    return {"g": hp.worst(allowed_ratio(grad, ref, allowed))}


# ------------------------------------------------------------------------------------------------ REINFORCE
REINFORCE_SHAPES = [(1, 1), (3, 64), (8, 1024), (8, 1025), (13, 1), (3, 5000), (12, 65536), (16, 4099)]
REINFORCE_KINDS = ("mixed", "one", "peaked")
BASELINE, DECAY, COEF = 0.7, 0.9, 0.01


def step_inputs(n, B, kind, seed):
    """(idx, logit, log_p, q32).  'mixed' and 'one' are test_gpu_adversarial_classical.step_inputs'; 'peaked': 90 % of the
    samples on min(3, N) outcomes with q > 0.1 (0.3, 0.25, 0.2; N = 2: 0.6, 0.4), the rest uniform over the table."""
    rng = np.random.default_rng(seed)
    N = 1 << n
    if kind == "peaked":
        hot = rng.choice(N, size=min(3, N), replace=False)
        q = rng.random(N) + 1e-3
        q[hot] = 0.0
        mass = np.array([0.3, 0.25, 0.2][:len(hot)]) if N > 2 else np.array([0.6, 0.4])
        q = q / max(q.sum(), 1e-300) * (1.0 - mass.sum())
        q[hot] = mass
        q32 = q.astype(np.float32)
        idx = np.where(rng.random(B) < 0.9, hot[rng.integers(0, len(hot), B)], rng.integers(0, N, B)).astype(np.int64)
        idx[0] = hot[0]
    else:
        q = rng.random(N) ** 4 + 1e-6
        q[0] = 1e-12 * q.sum()
        if N > 2:
            q[1] = 0.0
        q32 = (q / q.sum()).astype(np.float32)
        if kind == "one":
            idx = np.full(B, N - 1, dtype=np.int64)
        else:
            idx = rng.integers(0, max(1, N // 2), size=B).astype(np.int64)
            idx[0] = 0
            if B > 2 and N > 2:
                idx[1] = 1
                idx[2] = N - 1
    logit = (rng.standard_normal(B) * 5.0).astype(np.float32)
    big = rng.random(B) < 0.1
    logit[big] = (np.sign(rng.standard_normal(big.sum())) * (50.0 + rng.random(big.sum()))).astype(np.float32)
    log_p = (rng.standard_normal(N) * 3.0 - 5.0).astype(np.float32)
    return idx, logit, log_p, q32


def step_seed(n, B, kind, first):
    return 100 * n + B % 97 + int(first) + 1000 * REINFORCE_KINDS.index(kind)


def reinforce_reference(idx, logit, log_p, q32, baseline, first, decay, coef=COEF):
    """Long-double step and what each output may differ by: {'d': (ref, allowed), 'loss': ..., 'base': ...}, 'u', 'hits'."""
    B, N = int(idx.shape[0]), int(q32.shape[0])
    C = reinforce_constants(N.bit_length() - 1, B)
    raw = ld(logit) - ld(log_p)[idx]
    mean = raw.sum() / B
    base = mean if first else LD(decay) * LD(baseline) + (LD(1) - LD(decay)) * mean
    W = np.abs(raw).max() + np.abs(base) + LD(abs(coef))
    log2B = (B - 1).bit_length()
    u = LD(2.0) ** (int(np.frexp(W)[1]) - 1 + 1 - (60 - log2B))
    d_base = LD(EPS64) * (LD(C["T_mean"]) * np.abs(raw).sum() / B + 3 * np.abs(base))
    S = np.zeros(N, dtype=LD)
    np.add.at(S, idx, raw - base + LD(coef))
    hits = np.bincount(idx, minlength=N)
    S_allowed = ld(hits) * (u / 2 + 3 * LD(EPS64) * W + d_base)
    q = ld(q32)
    live = (q32 >= CLAMP32) & (hits > 0)
    Bq = B * np.where(live, q, LD(1))
    d = np.where(live, S / Bq, LD(0))
    d_allowed = np.where(live, S_allowed / Bq + 3 * LD(EPS64) * np.abs(d), LD(0))
    logc = np.abs(np.log(ld(np.maximum(q32, CLAMP32))))
    loss = -(logc * S).sum() / B
    chain = (logc * (S_allowed + LD(C["T_loss"] * EPS64) * np.abs(S))).sum() / B
    loss_allowed = chain + LD(F32_HALF_ULP) * (np.abs(loss) + chain)
    return {"d": (d, d_allowed), "loss": (loss, loss_allowed), "base": (base, d_base), "u": float(u), "hits": hits,
            "T_mean": C["T_mean"], "T_loss": C["T_loss"]}


def reinforce_check(ref, d, loss, base):
    dr, da = ref["d"]
    assert np.all(np.asarray(d)[to_f64(da) == 0.0] == 0.0), "an outcome never hit, or below the floor, is not exactly 0"
    return {"d": hp.worst(allowed_ratio(d, dr, da)), "loss": hp.worst(allowed_ratio(loss, *ref["loss"])),
            "base": hp.worst(allowed_ratio(base, *ref["base"]))}

