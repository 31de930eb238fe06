"""Oracle of the sampled MPS Born machine's exact queries (test infrastructure, plain NumPy, not under test).

Conventions of mps_sampled_mirror: np.longdouble where hp_reference.HAVE_LONGDOUBLE holds, no rescaling, tuple position 0 =
the most significant bit of an outcome index.  An evidence is a dict {position: 0 or 1}.
  words                 the (mask, value) words of an evidence
  clamped_environments  E^(j)_k with a clamped site allowing one s, and the same from |cores|
  log_marginal          log (E^(j)_0[0, 0] / E_0[0, 0]), with the two condition numbers
  marginals             m1[i] = q(z_i = 1), m2[i, j] = q(z_i = 1, z_j = 1) from the environments, and the same sums with every
                        term's magnitude (|cores| throughout, divided by the true Z)
  sample_clamped        the clamped sampler with the kernel's uniforms (mps_sampled_mirror.uniforms) and `undecided`
  conditionals_clamped  p1 at the free sites along given samples, log q(z | evidence), psi and psi_abs
  brute                 the same quantities by sums over all 2^n states (small n)
"""
import numpy as np

import mps_sampled_mirror as sm

LD = sm.LD


def words(ev, n):
    mask = value = 0
    for p, v in ev.items():
        mask |= 1 << (n - 1 - p)
        value |= int(v) << (n - 1 - p)
    return mask, value


def clamped_environments(cores, ev, dtype=None):
    """dict E [n + 1, D, D], Z (= E_0[0, 0]: the evidence's unnormalised mass), E_abs, Z_abs."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    out = {}
    for tag, A in (("", cores.astype(dtype)), ("_abs", np.abs(cores).astype(dtype))):
        E = np.zeros((n + 1, D, D), dtype)
        E[n, 0, 0] = 1
        for k in range(n, 0, -1):
            allowed = (ev[k - 1],) if (k - 1) in ev else (0, 1)
            E[k - 1] = sum(A[k - 1, s] @ E[k] @ A[k - 1, s].T for s in allowed)
        out["E" + tag], out["Z" + tag] = E, E[0, 0, 0]
    return out


def log_marginal(cores, ev, env=None, dtype=None):
    """dict logm, Zc (the evidence's mass), Z, kappa_c = Zc_abs / Zc, kappa_Z."""
    dtype = dtype or LD
    env = env or sm.environments(cores, dtype)
    c = clamped_environments(cores, ev, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        logm = np.log(c["Z"]) - np.log(env["Z"])
        kc = c["Z_abs"] / c["Z"] if c["Z"] != 0 else np.inf
    return {"logm": logm, "Zc": c["Z"], "Z": env["Z"], "kappa_c": kc, "kappa_Z": env["Z_abs"] / env["Z"]}


def marginals(cores, env=None, dtype=None):
    """dict m1 [n], m2 [n, n] and m1_abs, m2_abs (every term's magnitude over the true Z)."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    env = env or sm.environments(cores, dtype)
    out = {}
    for tag, A in (("", cores.astype(dtype)), ("_abs", np.abs(cores).astype(dtype))):
        E, L = env["E" + tag], env["L" + tag]
        m1 = np.zeros(n, dtype)
        m2 = np.zeros((n, n), dtype)
        for i in range(1, n + 1):
            m1[i - 1] = (L[i - 1] * (A[i - 1, 1] @ E[i] @ A[i - 1, 1].T)).sum() / env["Z"]
            m2[i - 1, i - 1] = m1[i - 1]
            M = A[i - 1, 1].T @ L[i - 1] @ A[i - 1, 1]
            for j in range(i + 1, n + 1):
                v = (M * (A[j - 1, 1] @ E[j] @ A[j - 1, 1].T)).sum() / env["Z"]
                m2[i - 1, j - 1] = m2[j - 1, i - 1] = v
                M = sum(A[j - 1, s].T @ M @ A[j - 1, s] for s in (0, 1))
        out["m1" + tag], out["m2" + tag] = m1, m2
    return out


def _sweep(cores, ev, bits, U, dtype, margin):
    """Left to right against the clamped environments: bits given (conditionals) or drawn from U (sampling)."""
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    c = clamped_environments(cores, ev, dtype)
    A, Aa = cores.astype(dtype), np.abs(cores).astype(dtype)
    Bn = bits.shape[0] if bits is not None else U.shape[0]
    l = np.zeros((Bn, D), dtype)
    la = np.zeros((Bn, D), dtype)
    l[:, 0] = la[:, 0] = 1
    p1 = np.full((Bn, n), np.nan, dtype)
    drawn = np.zeros((Bn, n), np.int64)
    undecided = 0
    for k in range(1, n + 1):
        u = [l @ A[k - 1, s] for s in (0, 1)]
        ua = [la @ Aa[k - 1, s] for s in (0, 1)]
        m = [np.einsum('bc,cd,bd->b', u[s], c["E"][k], u[s]) for s in (0, 1)]
        if (k - 1) in ev:
            z = np.full(Bn, bool(ev[k - 1]))
        else:
            p1[:, k - 1] = m[1] / (m[0] + m[1])
            if bits is not None:
                z = bits[:, k - 1].astype(bool)
            else:
                Uk = U[:, k - 1].astype(dtype)
                undecided += int(((np.abs(Uk - p1[:, k - 1]) <= margin) | (np.abs(Uk - (1 - p1[:, k - 1])) <= margin)).sum())
                z = Uk * (m[0] + m[1]) >= m[0]
        drawn[:, k - 1] = z
        l = np.where(z[:, None], u[1], u[0])
        la = np.where(z[:, None], ua[1], ua[0])
    psi, psia = l[:, 0], la[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        logq = np.log(psi * psi) - np.log(c["Z"])
    return {"bits": drawn, "idx": sm.idx_of_bits(drawn), "p1": p1, "logq": logq, "psi": psi, "psi_abs": psia, "undecided": undecided,
            "Zc": c["Z"], "Zc_abs": c["Z_abs"]}


def sample_clamped(cores, ev, seed, epoch, B, dtype=None, margin=2.0 ** -40):
    """The clamped sampler with the kernel's uniforms: dict bits, idx, logq (= log q(z | evidence)), p1 (NaN at clamped sites),
    undecided (draws with U within `margin` of p1 or of 1 - p1, free sites only), Zc, Zc_abs."""
    dtype = dtype or LD
    n = np.asarray(cores).shape[0]
    return _sweep(cores, ev, None, sm.uniforms(seed, epoch, np.arange(B), n), dtype, margin)


def conditionals_clamped(cores, ev, bits, dtype=None):
    """The same along given samples (their clamped positions must carry the evidence)."""
    return _sweep(cores, ev, np.asarray(bits), None, dtype or LD, 0.0)


def brute(cores, dtype=None):
    """dict q [2^n] (long double), bits [2^n, n] by enumeration: what the queries are sums of."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    N = 1 << n
    bits = sm.bits_of_idx(np.arange(N), n)
    A = cores.astype(dtype)
    v = np.zeros((N, D), dtype)
    v[:, 0] = 1
    for k in range(n):
        v = np.einsum('za,zab->zb', v, A[k][bits[:, k]])
    psi2 = v[:, 0] ** 2
    return {"q": psi2 / psi2.sum(), "bits": bits}


def consistent(bits, ev):
    ok = np.ones(bits.shape[0], bool)
    for p, v in ev.items():
        ok &= bits[:, p] == v
    return ok
