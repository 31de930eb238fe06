"""Mirror of bornvi_mps_twosite_sweep (test infrastructure, plain NumPy, not under test): the round trip of
csrc/kernels_mps_twosite.hip written once over a dtype -- float64, the arithmetic of the kernel, and hp_reference's extended
one (np.longdouble), the reference.  The factorisation and the cut are mps_canon_mirror's `jacobi` (mc_jacobi's pair order)
and `cut`.

Conventions: cores [n, 2, D, D], psi(z) = e0^T A_1[z_1] .. A_n[z_n] e0, z_k = bit n - k of the index.
On entry the sites 2 .. n are right-canonical and Z = 1.  One call is a round trip: the bonds k = 1 .. n - 1 left to right,
then n - 1 .. 1 right to left.  At bond (k, k + 1), the j-th visited:
  M[s, t] = A_k[s] A_{k+1}[t];   psi_b = l_b^T M[s_b, t_b] r_b,  l_b = e0^T A_1 .. A_{k-1},  r_b = A_{k+2} .. A_n e0;
  a sample counts when psi_b is finite and not 0;  W = the sum of the w_b that count;
  L = W log |M|^2 - sum_b w_b log psi_b^2;   dL/dM = 2 (W M / |M|^2 - sum_b (w_b / psi_b) l_b r_b^T at [s_b, t_b]);
  `steps` times  M <- M - lr dL/dM,  M <- M / |M|_F;   loss[j] = L after the last step;
  the split: M as 2 D x 2 D, rows (s, a), columns (t, c);  M 2^-e = G V^T by `jacobi`;  sigma sorted descending, ties by index;
  `cut` with D_keep and cutoff;  s = sigma_kept / |sigma_kept|;  going right A_k = U_kept, A_{k+1} = s V_kept^T;  going left
  A_k = U_kept s, A_{k+1} = V_kept^T;  exact zeros beyond the kept rank, in the first core's rows >= 1 and the last core's
  columns >= 1;  then l_b <- l_b A_k[s_b] (right) or r_b <- A_{k+1}[t_b] r_b (left).
  The return pass records schmidt[k - 1] (the kept s, then zeros), rank[k - 1], discarded[k - 1].
"""
import numpy as np

import hp_reference as hp
import mps_canon_mirror as cm

LD = cm.LD
EPS64 = hp.EPS64


def bits_of(idx, n):
    """[B, n] int64: column k - 1 is z_k = bit n - k of the index word."""
    idx = np.asarray(idx).astype(np.uint64)
    shifts = (n - 1 - np.arange(n)).astype(np.uint64)
    return ((idx[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.int64)


def merged(Ak, Ak1):
    """M[s, t, a, c] = (A_k[s] A_{k+1}[t])[a, c]."""
    return np.einsum("sae,tec->stac", Ak, Ak1)


def psi_samples(M, l, r, s, t):
    return np.einsum("ba,bac,bc->b", l, M[s, t], r)


def loss_and_grad(M, l, r, s, t, w):
    """(L, dL/dM, the samples that count) of the merged tensor M [2, 2, D, D] for left vectors l [B, D], right vectors r [B, D],
    the samples' bits s, t [B] at the two sites and weights w [B]."""
    dtype = M.dtype.type
    with np.errstate(all="ignore"):
        psi = psi_samples(M, l, r, s, t)
        good = np.isfinite(psi) & (psi != 0)
        safe = np.where(good, psi, dtype(1))
        wg = np.where(good, w, dtype(0))
        W = wg.sum()
        nrm2 = (M * M).sum()
        loss = W * np.log(nrm2) - (wg * np.log(safe * safe)).sum()
        coef = wg / safe
        G = np.zeros_like(M)
        for s0 in (0, 1):
            for t0 in (0, 1):
                m = (s == s0) & (t == t0)
                G[s0, t0] = np.einsum("b,ba,bc->ac", coef[m], l[m], r[m])
        grad = 2 * (W * M / nrm2 - G)
    return loss, grad, good


def split(M, k, n, direction, D_keep, cutoff, dtype):
    """(A_k, A_{k+1}, kept values over their norm [D], discarded, rank, gap, sweeps, converged) of the merged tensor."""
    D = M.shape[2]
    mat = M.transpose(0, 2, 1, 3).reshape(2 * D, 2 * D)
    mat, _ = cm._rescale(mat, dtype)
    G, V, sigma, sw, ok = cm.jacobi(mat, 2 * D, dtype)
    order = np.argsort(-sigma, kind="stable")
    _, disc, r, total, gap = cm.cut(sigma[order], D_keep, cutoff, dtype)
    kept = order[:r]
    sk = sigma[kept]
    ksum = dtype(0)
    for i in range(r - 1, -1, -1):
        ksum = ksum + sk[i] * sk[i]
    with np.errstate(all="ignore"):
        sn = sk / np.sqrt(ksum)
        U = np.where(sk > 0, G[:, kept] / np.where(sk > 0, sk, dtype(1)), dtype(0))      # [2 D, r]
    Vk = V[:, kept]                                                                       # [2 D, r]
    if direction > 0:
        Vk = Vk * sn[None, :]
    else:
        U = U * sn[None, :]
    Ak = np.zeros((2, D, D), dtype)
    Ak1 = np.zeros((2, D, D), dtype)
    for s in (0, 1):
        Ak[s, :, :r] = U[s * D:(s + 1) * D, :]
        Ak1[s, :r, :] = Vk[s * D:(s + 1) * D, :].T
    if k == 1:
        Ak[:, 1:, :] = 0
    if k + 1 == n:
        Ak1[:, :, 1:] = 0
    sch = np.zeros(D, dtype)
    sch[:r] = sn
    return Ak, Ak1, sch, disc, r, gap, sw, ok


def sweep(cores, idx, w=None, lr=0.05, steps=5, D_keep=None, cutoff=0.0, dtype=np.float64, on_bond=None):
    """One round trip -> dict: cores [n, 2, D, D], loss [2 (n - 1)], schmidt [n - 1, D], discarded [n - 1], rank [n - 1] int32,
    status, sweeps (the largest count of one factorisation), loss_scale [2 (n - 1)] (|L| + 2 sum_b w_b / |psi_b|: a norm-wise
    error e of the state moves log psi_b^2 by 2 e / |psi_b|), gap (the smallest of `cut`'s over every bond of both passes, in
    units of the bond's normalised values), all in dtype.  on_bond(j, cores): called after every bond with the cores so far."""
    cores64 = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores64.shape
    Dk = D if D_keep is None else int(D_keep)
    idx = np.asarray(idx)
    B = len(idx)
    bits = bits_of(idx, n)
    w64 = np.full(B, 1.0 / B) if w is None else np.asarray(w, dtype=np.float64)
    w_ = w64.astype(dtype)
    lr_ = dtype(np.float64(lr))
    c = cores64.astype(dtype)
    nb = n - 1
    loss = np.zeros(2 * nb, dtype)
    schmidt = np.zeros((nb, D), dtype)
    discarded = np.zeros(nb, dtype)
    rank = np.zeros(nb, np.int32)
    loss_scale = np.zeros(2 * nb, dtype)        # |L| + 2 sum_b w_b / |psi_b|: what a norm-wise error of the state does to L
    status, sweeps, gap = 0, 0, np.inf
    if not np.isfinite(cores64).all():
        return dict(cores=c + np.nan, loss=loss + np.nan, schmidt=schmidt + np.nan, discarded=discarded + np.nan, rank=rank,
                    status=1, sweeps=0, gap=gap)
    e0 = np.zeros((B, D), dtype)
    e0[:, 0] = 1
    vec = [None] * (n + 2)                      # slot j = 1 .. n: l_j where the sweep has passed, r_j where it has not
    vec[0], vec[n + 1] = e0, e0
    with np.errstate(all="ignore"):
        r = e0
        for k in range(n, 2, -1):
            r = np.einsum("bac,bc->ba", c[k - 1][bits[:, k - 1]], r)
            vec[k] = r
        for j in range(2 * nb):
            direction = 1 if j < nb else -1
            k = j + 1 if direction > 0 else 2 * nb - j
            M = merged(c[k - 1], c[k])
            nrm2 = (M * M).sum()
            if not (np.isfinite(nrm2) and nrm2 > 0):
                status |= 1
                break
            if abs(float(nrm2) - 1.0) > 2.0 ** -20:
                status |= 8
            l, rr = vec[k - 1], vec[k + 2]
            s, t = bits[:, k - 1], bits[:, k]
            for _ in range(steps):
                _, grad, good = loss_and_grad(M, l, rr, s, t, w_)
                if not good.all():
                    status |= 2
                M = M - lr_ * grad
                M = M / np.sqrt((M * M).sum())
            if not np.isfinite(M).all():
                status |= 1
                break
            L, _, good = loss_and_grad(M, l, rr, s, t, w_)
            if not good.all():
                status |= 2
            loss[j] = L
            psi = np.where(good, psi_samples(M, l, rr, s, t), dtype(1))
            loss_scale[j] = np.abs(L) + 2 * (np.where(good, w_, dtype(0)) / np.abs(psi)).sum()
            Ak, Ak1, sch, disc, rk, gp, sw, ok = split(M, k, n, direction, Dk, cutoff, dtype)
            c[k - 1], c[k] = Ak, Ak1
            sweeps = max(sweeps, sw)
            gap = min(gap, gp)
            status |= 0 if ok else 4
            if direction < 0:
                schmidt[k - 1], discarded[k - 1], rank[k - 1] = sch, disc, rk
            if direction > 0:
                vec[k] = np.einsum("ba,bac->bc", l, Ak[s])
            else:
                vec[k + 1] = np.einsum("bac,bc->ba", Ak1[t], rr)
            if on_bond is not None:
                on_bond(j, c.copy())
    if status & 1:
        return dict(cores=c + np.nan, loss=loss + np.nan, schmidt=schmidt + np.nan, discarded=discarded + np.nan, rank=rank * 0,
                    status=status, sweeps=sweeps, gap=gap)
    return dict(cores=c, loss=loss, schmidt=schmidt, discarded=discarded, rank=rank, status=status, sweeps=sweeps, gap=gap,
                loss_scale=loss_scale)


def canonical(cores):
    """The entry gauge of `cores` in float64: mps_canon_mirror's canonical form (sites 2 .. n right-canonical, Z = 1)."""
    return hp.to_f64(cm.canonicalise(np.asarray(cores, dtype=np.float64))["cores_out"])


def product_state(n, D):
    """The uniform product state zero-padded to bond dimension D, already canonical: psi(z) = 2^(-n/2)."""
    c = np.zeros((n, 2, D, D))
    c[:, :, 0, 0] = 1.0 / np.sqrt(2.0)
    return c


def probabilities(cores):
    """q [2^n] float64 of cores (n <= 12 or so), psi enumerated in extended precision."""
    psi, Z = cm.psi_of(hp.to_f64(cores))
    return hp.to_f64(psi * psi / Z)


def forward_kl(cores, p):
    q = probabilities(cores)
    m = p > 0
    with np.errstate(all="ignore"):
        return float((p[m] * (np.log(p[m]) - np.log(np.maximum(q[m], 1e-300)))).sum())


def chain_network(n, seed=3):
    """(BayesianNetwork, site names): a Markov chain of n binary nodes, every bond of its joint has rank 2."""
    from tensornetworks_amd.bayesian_network import BayesianNetwork
    rng = np.random.default_rng(seed)
    row = lambda p1: {0: 1.0 - p1, 1: p1}
    bn = BayesianNetwork()
    bn.add_node("N0", cpt={(): row(float(rng.uniform(0.1, 0.9)))})
    for v in range(1, n):
        bn.add_node(f"N{v}", cpt={(0,): row(float(rng.uniform(0.1, 0.9))), (1,): row(float(rng.uniform(0.1, 0.9)))},
                    parent_names=[f"N{v - 1}"])
    return bn, [f"N{v}" for v in range(n)]


def derived_constant(n, D, steps):
    """First-order worst case of a round trip's gauge-free outputs, units of EPS64 against 1.  One bond:
    the factorisation of a 2 D x 2 D matrix is mps_canon_mirror's per-factorisation count at 2 D columns and 2 D rows (3 x 30
    (2 D - 1) rotations' roundings, the 2 D-term chains and the butterfly 2 D + 4, the rotation test's 4 D, 8 for the divisions
    and the norm); forming M is a D-term chain (D); every descent step adds the psi chain (D^2 terms, two roundings each, against
    |l| |M| |r| <= 1), the quotient, the MFMA sum over the samples and its partials relative to the gradient's own size (the
    weights sum to 1: 8), the update and the renormalisation (2 D^2 + 4): steps (3 D^2 + 12); the advance is a D-term chain (D).
    The errors of the 2 (n - 1) bonds add: each acts on an orthonormal frame.  Plus 8 for the logs of the loss."""
    per = 3 * cm.MAX_SWEEPS * max(2 * D - 1, 1) + (2 * D + 4) + 4 * D + 8 + 2 * D + (steps + 1) * (3 * D * D + 12)
    return float(2 * (n - 1) * per + 8)
