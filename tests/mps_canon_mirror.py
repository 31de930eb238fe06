"""Mirror of bornvi_mps_canonicalise (test infrastructure, plain NumPy, not under test): the two sweeps of
csrc/kernels_mps_canon.hip written once over a dtype -- float64, the arithmetic of the kernel, and hp_reference's extended
one (np.longdouble), the reference -- and, for n <= 12, an independent route to the Schmidt values.

The sweeps (psi(z) = e0^T A_1[z_1] .. A_n[z_n] e0, cores [n, 2, D, D]):
  left, k = 1 .. n - 1:   M = [C A_k[0]; C A_k[1]] (2 D x D), C_0 = e0 e0^T (only row 0 of the first core enters psi);
                          M 2^-e = Q (S V^T) by `jacobi`;  Q_k[s] = the blocks of Q;  C = S V^T / |S V^T|_F;
                          log += log |S V^T|_F + e ln 2.   Then T_n[s] = C A_n[s].
  right, k = n .. 2:      M = [T_k[0] R, T_k[1] R] (D x 2 D), T_k = Q_k for k < n, R_n = e0 e0^T (only column 0 of the last
                          core enters psi);  M^T 2^-e = G V^T by `jacobi`, so M = V S W with the rows of W the normalised
                          columns of G;  sigma sorted descending, ties by index;  schmidt[k - 2] = sigma / |sigma|;
                          the cut (`cut`);  A_k[s] = the kept rows of W's blocks;  R = (V S)[:, kept] / |S[kept]|.
                          At k = n:  log += log |sigma| + e ln 2.
  last:                   A_1[s] = Q_1[s] R.   log_norm = 2 log.   n = 1: the one core over its norm.

The Jacobi routine (one-sided, Hestenes) orthogonalises the columns of a matrix with <= 64 rows and D <= 32 columns by plane
rotations, accumulated in V; pairs in round-robin tournament order (`tournament`), at most MAX_SWEEPS sweeps, a sweep
without a rotation ends it.  A pair (i, j) with a = |g_i|^2, b = |g_j|^2, c = g_i . g_j rotates when
|c| > rows EPS sqrt(a) sqrt(b), EPS the dtype's.

THE RANK RULE.  A pair is skipped when either column's squared norm is <= (D EPS64)^2 times the largest squared column norm
of the matrix as it was given to the routine, and such a column's singular value is reported as exactly 0.0 (its column of
Q, or row of W, as zeros).  EPS64 = 2^-52 in every dtype: the rule is part of the function computed, not of the rounding.
Without it two columns of pure rounding noise never pass the rotation test, and rank deficiency is the normal case here
(bond k has rank <= min(2^k, 2^(n-k)); zero-padded and expanded models have null columns).

`unfolded_schmidt`: psi enumerated in extended precision (mps_mirror.reference), reshaped to 2^k x 2^(n-k) at every bond,
np.linalg.svd of it: LAPACK, no sweep, no gauge.
"""
import numpy as np

import hp_reference as hp
import mps_mirror as mm

LD = mm.LD
EPS64 = hp.EPS64
MAX_SWEEPS = 30


def tournament(D):
    """[rounds][pairs] of (i, j), i < j < D: the circle method on m = D rounded up to even players, player m - 1 fixed;
    a pair with the dummy player D (odd D) is left out.  D - 1 rounds for even D, D for odd D."""
    m = D + (D & 1)
    out = []
    for r in range(m - 1):
        pairs = []
        for p in range(m // 2):
            i, j = (m - 1, r) if p == 0 else ((r + p) % (m - 1), (r - p + (m - 1)) % (m - 1))
            if i > j:
                i, j = j, i
            if j < D:
                pairs.append((i, j))
        out.append(pairs)
    return out


def jacobi(G, D, dtype):
    """G [rows, D] -> (G with orthogonal columns, V [D, D], sigma [D] with the rank rule's exact zeros, sweeps, converged)."""
    G = G.copy()
    rows = G.shape[0]
    V = np.eye(D, dtype=dtype)
    thr = dtype(D * EPS64) ** 2 * (G * G).sum(axis=0).max()
    tol = dtype(rows) * dtype(np.finfo(dtype).eps)
    rounds = [(np.array([p[0] for p in pr], dtype=np.int64), np.array([p[1] for p in pr], dtype=np.int64)) for pr in tournament(D)]
    sweeps, converged = 0, False
    for _ in range(MAX_SWEEPS):
        sweeps += 1
        rotated = False
        for I, J in rounds:
            if len(I) == 0:
                continue
            gi, gj = G[:, I], G[:, J]
            a, b, c = (gi * gi).sum(axis=0), (gj * gj).sum(axis=0), (gi * gj).sum(axis=0)
            with np.errstate(all="ignore"):
                do = (a > thr) & (b > thr) & (np.abs(c) > tol * np.sqrt(a) * np.sqrt(b))
                if not do.any():
                    continue
                rotated = True
                cs_ = np.where(do, c, dtype(1))
                zeta = (b - a) / (2 * cs_)
                t = np.where(zeta >= 0, dtype(1), dtype(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                cs = 1 / np.sqrt(1 + t * t)
                sn = cs * t
            cs = np.where(do, cs, dtype(1))
            sn = np.where(do, sn, dtype(0))
            G[:, I], G[:, J] = cs * gi - sn * gj, sn * gi + cs * gj
            vi, vj = V[:, I], V[:, J]
            V[:, I], V[:, J] = cs * vi - sn * vj, sn * vi + cs * vj
        if not rotated:
            converged = True
            break
    nrm2 = (G * G).sum(axis=0)
    sigma = np.where(nrm2 > thr, np.sqrt(nrm2), dtype(0))
    return G, V, sigma, sweeps, converged


def _rescale(M, dtype):
    """(M 2^-e, e): e = ilogb of the largest magnitude (0 for a zero or non-finite one), an exact scaling."""
    mx = np.abs(M).max()
    if not (mx > 0 and np.isfinite(mx)):
        return M, 0
    e = int(np.floor(np.log2(np.float64(mx))))
    if np.ldexp(np.float64(1.0), e) > np.float64(mx):
        e -= 1
    return np.ldexp(M, -e), e


def cut(sorted_sigma, D_out, cutoff, dtype):
    """(schmidt [D], discarded, rank, gap) of the sorted singular values: cumulative squares from the small end; the values
    behind D_out go, then more from the small end for as long as the dropped squares' normalised sum stays <= cutoff; one
    value always stays.  gap: the smallest kept normalised value minus the largest dropped one (inf when nothing is cut)."""
    D = len(sorted_sigma)
    cum = np.zeros(D + 1, dtype)
    for i in range(D - 1, -1, -1):
        cum[i] = cum[i + 1] + sorted_sigma[i] * sorted_sigma[i]
    total = cum[0]
    with np.errstate(all="ignore"):
        r = D_out
        while r > 1 and cum[r - 1] / total <= dtype(cutoff):
            r -= 1
        schmidt = sorted_sigma / np.sqrt(total)
        discarded = cum[r] / total if r < D else dtype(0)
    gap = np.inf if r == D else float(schmidt[r - 1] - schmidt[r])
    return schmidt, discarded, r, total, gap


def canonicalise(cores, D_out=None, cutoff=0.0, dtype=np.float64):
    """dict: cores_out [n, 2, D_out, D_out], schmidt [n - 1, D], discarded [n - 1], rank [n - 1], log_norm, status,
    sweeps (the largest count of one factorisation), gap (the smallest of `cut`'s over the bonds), log_abs (log_norm's sum
    with every term's magnitude), all in dtype."""
    cores64 = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores64.shape
    Do = D if D_out is None else int(D_out)
    A = cores64.astype(dtype)
    ln2 = np.log(dtype(2))
    out = np.zeros((n, 2, Do, Do), dtype)
    schmidt = np.zeros((max(n - 1, 0), D), dtype)
    discarded = np.zeros(max(n - 1, 0), dtype)
    rank = np.zeros(max(n - 1, 0), np.int32)
    status, sweeps, gap = 0, 0, np.inf
    if not np.isfinite(cores64).all():
        return dict(cores_out=out + np.nan, schmidt=schmidt + np.nan, discarded=discarded + np.nan, rank=rank,
                    log_norm=dtype(np.nan), status=1, sweeps=0, gap=gap)
    log = labs = dtype(0)
    C = np.zeros((D, D), dtype)
    C[0, 0] = 1
    T = np.zeros((n, 2, D, D), dtype)
    with np.errstate(all="ignore"):
        for k in range(1, n):
            M = np.concatenate([C @ A[k - 1, 0], C @ A[k - 1, 1]], axis=0)
            M, e = _rescale(M, dtype)
            G, V, sigma, sw, ok = jacobi(M, D, dtype)
            sweeps = max(sweeps, sw)
            status |= 0 if ok else 4
            Q = np.where(sigma > 0, G / np.where(sigma > 0, sigma, dtype(1)), dtype(0))
            T[k - 1, 0], T[k - 1, 1] = Q[:D], Q[D:]
            C = sigma[:, None] * V.T
            nrm = np.sqrt((C * C).sum())
            C = C / nrm
            log = log + np.log(nrm) + e * ln2
            labs = labs + np.abs(np.log(nrm)) + abs(e) * ln2
        T[n - 1, 0], T[n - 1, 1] = C @ A[n - 1, 0], C @ A[n - 1, 1]
        R = np.zeros((D, D), dtype)
        R[0, 0] = 1
        for k in range(n, 1, -1):
            M = np.concatenate([T[k - 1, 0] @ R, T[k - 1, 1] @ R], axis=1)          # D x 2 D
            Mt, e = _rescale(M.T.copy(), dtype)
            G, V, sigma, sw, ok = jacobi(Mt, D, dtype)
            sweeps = max(sweeps, sw)
            status |= 0 if ok else 4
            order = np.argsort(-sigma, kind="stable")
            sch, disc, r, total, gp = cut(sigma[order], Do, cutoff, dtype)
            gap = min(gap, gp)
            schmidt[k - 2], discarded[k - 2], rank[k - 2] = sch, disc, r
            if k == n:
                log = log + np.log(np.sqrt(total)) + e * ln2
                labs = labs + np.abs(np.log(np.sqrt(total))) + abs(e) * ln2
            kept = order[:r]
            sk = sigma[kept]
            W = np.where(sk > 0, G[:, kept] / np.where(sk > 0, sk, dtype(1)), dtype(0))       # [2 D, r]: W^T's kept columns
            for s in (0, 1):
                out[k - 1, s, :r, :] = W[s * D:s * D + Do, :].T
            ksum = dtype(0)
            for i in range(r - 1, -1, -1):
                ksum = ksum + sk[i] * sk[i]
            R = np.zeros((D, D), dtype)
            R[:, :r] = V[:, kept] * sk[None, :] / np.sqrt(ksum)
        if n == 1:
            a0, a1 = T[0, 0, 0, 0], T[0, 1, 0, 0]
            nrm = np.sqrt(a0 * a0 + a1 * a1)
            out[0, 0, 0, 0], out[0, 1, 0, 0] = a0 / nrm, a1 / nrm
            log = log + np.log(nrm)
            labs = labs + np.abs(np.log(nrm))
        else:
            for s in (0, 1):
                out[0, s, 0, :] = (T[0, s] @ R)[0, :Do]
            out[n - 1, :, :, 1:] = 0
    log_norm = 2 * log
    if not np.isfinite(log_norm):
        return dict(cores_out=out + np.nan, schmidt=schmidt, discarded=discarded, rank=rank, log_norm=dtype(np.nan),
                    status=status | 1, sweeps=sweeps, gap=gap)
    return dict(cores_out=out, schmidt=schmidt, discarded=discarded, rank=rank, log_norm=log_norm, status=status,
                sweeps=sweeps, gap=gap, log_abs=2 * labs)


def psi_of(cores):
    """(psi [2^n], Z) in extended precision, every z its own product of n matrices (mps_mirror.reference)."""
    ref = mm.reference(np.asarray(cores, dtype=np.float64))
    return ref["psi"], ref["Z"]


def unfolded_schmidt(cores):
    """[n - 1, D] float64: the singular values of psi / |psi| unfolded to 2^k x 2^(n-k) at every bond k, descending, cut or
    zero-padded to D (a bond has at most D non-zero ones)."""
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    psi, Z = psi_of(cores)
    v = hp.to_f64(psi / np.sqrt(Z))
    out = np.zeros((n - 1, D))
    for k in range(1, n):
        s = np.linalg.svd(v.reshape(1 << k, 1 << (n - k)), compute_uv=False)
        m = min(D, len(s))
        out[k - 1, :m] = s[:m]
    return out


def expand(cores, D_new, noise=0.0, seed=0):
    """MPSCores.expand_ on the CPU: the old cores in the leading block of zeros; noise * randn of a generator seeded by seed
    in the new entries, the first core's rows >= 1 and the last core's columns >= 1 left 0."""
    import torch
    c = torch.as_tensor(np.asarray(cores, dtype=np.float64))
    n, _, D, _ = c.shape
    out = torch.zeros(n, 2, D_new, D_new, dtype=torch.float64)
    out[:, :, :D, :D] = c
    if noise != 0.0:
        gen = torch.Generator().manual_seed(int(seed))
        fresh = torch.ones(n, 2, D_new, D_new, dtype=torch.bool)
        fresh[:, :, :D, :D] = False
        fresh[0, :, 1:, :] = False
        fresh[n - 1, :, :, 1:] = False
        out = out + noise * torch.randn(n, 2, D_new, D_new, dtype=torch.float64, generator=gen) * fresh
    return out.numpy()


def derived_constant(n, D):
    """First-order worst case of the canonicaliser's outputs, units of EPS64 against 1 (the state has norm 1; a Schmidt
    value is <= 1).  One factorisation: a column takes part in at most MAX_SWEEPS (D - 1) rotations, each rounding an
    entry three times (two products, one sum); the three dot products of a pair and the final norms are 2 D-term chains
    with a 4-level butterfly (2 D + 4); forming M is a D-term chain (D); the rotation test leaves the columns orthogonal to
    2 D EPS64 (2 D); dividing by sigma, S V^T and its norm, the rescale (8).  The errors of the 2 (n - 1) factorisations add:
    every one acts on an orthonormal frame.  Plus 8 for site 1 and the logs."""
    per = 3 * MAX_SWEEPS * max(D - 1, 1) + (2 * D + 4) + D + 2 * D + 8
    return float(2 * max(n - 1, 0) * per + 8)
