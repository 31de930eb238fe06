"""Oracle of the matrix-free natural gradient of the sampled MPS Born machine (test infrastructure, plain NumPy, not under
test).  Conventions of sampled_fisher_mirror; np.longdouble where hp_reference.HAVE_LONGDOUBLE holds (mps_sampled_mirror.LD).

  jvp        t_b = <o_b, v>: sampled_fisher_mirror.score_rows' rows contracted with v, and t_abs = rows_abs . |v|, the value
             the kernel's error bound is expressed in (= 2 dpsi_abs / |psi_b| + sum_k <mu_abs_k, |V_k|>)
  c_jvp      the derived per-entry error constant of bornvi_mps_score_jvp
  matvec     x -> X (X^T x) / B from rows X [P, B]: the Fisher estimate's product without the matrix
  cg         the recurrence of bornvi_cg_init / _step / _finish, word for word, in the dtype asked for
  residual   ||g - (F + lam I) x|| / ||g|| in extended precision
"""
import numpy as np

import mps_sampled_mirror as sm
import sampled_fisher_mirror as fm

LD = sm.LD


def jvp(cores, bits, v, env=None, sr=None):
    """dict t, t_abs [B] (extended precision), sr: the score rows' dict (kappa per sample among its entries)."""
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    sr = sr or fm.score_rows(cores, bits, env)
    vl = np.asarray(v, dtype=np.float64).astype(LD).reshape(n, 2 * D * D)
    t = (sr["rows"] * vl[:, :, None]).sum(axis=(0, 1))
    t_abs = (sr["rows_abs"] * np.abs(vl)[:, :, None]).sum(axis=(0, 1))
    return {"t": t, "t_abs": t_abs, "sr": sr}


def c_jvp(n, D, kappa_b, kappa_Z):
    """Derived C of one entry of bornvi_mps_score_jvp, units of EPS64 on t_abs, every rounding a whole unit, derived as
    sampled_fisher_mirror.c_rows is:
      the sample term 2 dpsi / psi: the term of site j of dl_n[0] = sum_j l_{j-1} V_j A_{j+1} ... A_n carries l_{j-1}
        ((j - 1) D-term fma chains) and then one 2 D-term chain per site j .. n (dl A and l V share a chain): at most
        (j - 1) D + 2 D (n - j + 1) <= 2 n D; the common power-of-two rescalings add nothing; 1 / psi_b costs
        C_PSI kappa_b = (n D + 2) kappa_b; the doubling is exact and the quotient one rounding: 1;
      c = sum_k <mu_k, V_k>: a mu entry as in c_rows ((n - 1)(3 D + 1) + 2 D + n (3 D + 1) kappa_Z + 2), the site's chain of
        2 D^2 products and the n sites in order: 2 D^2 + n;
      the subtraction and the product with scale: 2.
    Both terms are bounded by the same t_abs, so the constant is 2 + the larger of the two."""
    sample = 2 * n * D + (n * D + 2) * np.asarray(kappa_b, dtype=np.float64) + 1
    cterm = (n - 1) * (3 * D + 1) + 2 * D + n * (3 * D + 1) * kappa_Z + 2 + 2 * D * D + n
    return 2.0 + np.maximum(sample, cterm)


def matvec(X, B=None):
    """x -> X (X^T x) / B in X's own arithmetic."""
    den = X.dtype.type(X.shape[1] if B is None else B)
    Xt = np.ascontiguousarray(X.T)
    return lambda x: X @ (Xt @ x) / den


def cg(mv, g, lam, K, tol, dtype=np.float64):
    """The device recurrence: dict x, iters, relres, info, done, and x_iterate (the last CG iterate, before the fallback).
    mv(p) is F p without the damping."""
    dt = np.dtype(dtype).type
    g = np.asarray(g).astype(dtype).reshape(-1)
    lam, tol2 = dt(lam), dt(tol) * dt(tol)
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    rr = r @ r
    rr0, iters = rr, 0
    bad = not np.all(np.isfinite(g))
    done = bad or not rr > 0 or not np.isfinite(rr)
    fallback = bad or not np.isfinite(rr)
    relres = dt(0) if rr == 0 else np.sqrt(rr / rr)
    for _ in range(K):
        if done:
            continue
        q = mv(p) + lam * p
        pq = p @ q
        if not pq > 0 or not np.isfinite(pq):
            done = True
            fallback = fallback or iters == 0
            continue
        alpha = rr / pq
        x = x + alpha * p
        r = r - alpha * q
        rr1 = r @ r
        p = r + (rr1 / rr) * p
        rr, iters = rr1, iters + 1
        relres = np.sqrt(rr / rr0)
        if rr <= tol2 * rr0:
            done = True
    out = {"x_iterate": x, "iters": iters, "relres": relres, "done": bool(done)}
    if fallback or not np.all(np.isfinite(x)):
        out.update(x=g.copy(), info=1)
    else:
        out.update(x=x, info=0)
    return out


def residual(X, g, x, lam, B=None):
    """||g - (X X^T / B + lam I) x||_2 / ||g||_2 in extended precision, X [P, B] the mirror's rows."""
    Xl = np.asarray(X).astype(LD)
    gl, xl = (np.asarray(a, dtype=np.float64).astype(LD).reshape(-1) for a in (g, x))
    res = gl - (matvec(Xl, B)(xl) + LD(lam) * xl)
    return float(np.sqrt(res @ res) / np.sqrt(gl @ gl))
