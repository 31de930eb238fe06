"""Oracle of the sampled KSD path (test infrastructure, plain NumPy / CPU torch, not under test).

Everything takes the samples themselves, idx [B] and S [B, n] (hp_reference.gram_bound indexes S by outcome, which cannot
exist at n = 63), and works in hp_reference's extended arithmetic unless told otherwise (X=F64: plain float64, the replay's).
  kappa_bound       (K, Bt, d) [B, B]: k_p(z_b, z_b') bit by bit from the closed form, and its absolute-term sum B~
  kappa_four_terms  K from the four-term definition (n <= 6)
  kappa             the four-term K for n <= 6, the closed form above, and B~
  gemm_form         (K, A): the Gram arrangement the kernel evaluates, and the sum of the absolute values of ITS terms
  rowsums           r_b = sum over b' != b BY INDEX, T = sum_b r_b
  scores            S [B, n] from a packed network with floored factors, |ratio| and the number k of affected factors
  weights           U, m, w of the estimator
  pairs_geometry    (tiles per column range, G) of the row-sum kernel: a restatement of kernels_ksd_sampled.hip's kp_geom
  replay            float64 restatement of SampledKSDVariationalInference.train (torch autograd for the gradient)
"""
import math

import numpy as np
import torch

import hp_reference as hp
import mps_sampled_mirror as sm


class F64:
    """hp_reference's arithmetic interface in plain float64."""
    name = "float64"

    @staticmethod
    def arr(x):
        return np.asarray(x, dtype=np.float64)

    num = staticmethod(np.float64)
    exp = staticmethod(np.exp)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, np.float64)


def _setup(idx, S, n, length_scale, X):
    X = X or hp.arithmetic()
    idx = np.asarray(idx, dtype=np.int64)
    x = idx[:, None] ^ idx[None, :]
    one = X.num(1)
    nl = X.num(n) * X.num(float(length_scale))
    return X, idx, x, one, nl, X.arr(np.asarray(S, dtype=np.float64).reshape(len(idx), n))


def kappa_bound(idx, S, n, length_scale=1.0, X=None):
    """K_bb' = a^d sum_i [s_i s'_i - c_i (s_i + s'_i) + 2 c_i],  B~_bb' = a^d sum_i (|s_i s'_i| + |c_i| (|s_i| + |s'_i|) + 2 |c_i|),
    c_i = 1 - a where bit i agrees, 1 - 1/a where it differs (oracle/stein.py: gram_closed_form, hp_reference.gram_bound)."""
    X, idx, x, one, nl, Sx = _setup(idx, S, n, length_scale, X)
    a = X.exp(-one / nl)
    c_same, c_diff = one - a, one - one / a
    T, Bt = X.zeros(x.shape), X.zeros(x.shape)
    for b in range(n):
        bit = ((x >> (n - 1 - b)) & 1).astype(bool)
        c = np.where(bit, c_diff, c_same)
        si, sj = Sx[:, b][:, None], Sx[:, b][None, :]
        T = T + (si * sj - c * (si + sj) + 2 * c)
        Bt = Bt + (np.abs(si * sj) + np.abs(c) * (np.abs(si) + np.abs(sj)) + 2 * np.abs(c))
    d = hp.popcount(x)
    pw = np.empty(n + 1, dtype=Sx.dtype)
    for k in range(n + 1):
        pw[k] = a ** k
    return pw[d] * T, pw[d] * Bt, d


def kappa_four_terms(idx, S, n, length_scale=1.0, X=None):
    """The four-term definition (stein_utils.py:138-197, Eq. 13) with the base kernel evaluated at every flipped pair."""
    X, idx, x, one, nl, Sx = _setup(idx, S, n, length_scale, X)
    tab = np.empty(n + 2, dtype=Sx.dtype)
    for k in range(n + 2):
        tab[k] = X.exp(-X.num(k) / nl)
    d = hp.popcount(x)
    k0 = tab[d]
    K = X.zeros(x.shape)
    for b in range(n):
        bit = ((x >> (n - 1 - b)) & 1).astype(bool)
        kb = tab[np.where(bit, d - 1, d + 1)]
        si, sj = Sx[:, b][:, None], Sx[:, b][None, :]
        K = K + (si * sj * k0 - si * (k0 - kb) - (k0 - kb) * sj + (k0 - kb - kb + k0))
    return K


def kappa(idx, S, n, length_scale=1.0, X=None):
    K, Bt, _ = kappa_bound(idx, S, n, length_scale, X)
    if n <= 6:
        K = kappa_four_terms(idx, S, n, length_scale, X)
    return K, Bt


def gemm_form(idx, S, n, length_scale=1.0, X=None):
    """kappa = a^d [ s.s' - h t.t' + h (t - sigma).(t' - sigma') + h (n - 2 d) + m (n - sum s) + m (n - sum s') ],
    h = sinh(1/(n l)) = (u - v)/2, m = (u + v)/2, u = 1 - a, v = 1 - 1/a, sigma = 1 - 2 z, t = sigma s;
    A = a^d x the same with every term replaced by its magnitude (the kernel's own absolute-term sum)."""
    X, idx, x, one, nl, Sx = _setup(idx, S, n, length_scale, X)
    a = X.exp(-one / nl)
    u, v = one - a, one - one / a
    m, h = (u + v) / 2, (u - v) / 2
    Bn = len(idx)
    G, A = X.zeros((Bn, Bn)), X.zeros((Bn, Bn))
    for b in range(n):
        sg = X.arr(1.0 - 2.0 * ((idx >> (n - 1 - b)) & 1))
        s = Sx[:, b]
        t = sg * s
        e = t - sg
        G = G + (s[:, None] * s[None, :] - h * t[:, None] * t[None, :] + h * e[:, None] * e[None, :])
        A = A + (np.abs(s[:, None] * s[None, :]) + h * np.abs(t[:, None] * t[None, :]) + h * np.abs(e[:, None] * e[None, :]))
    d = hp.popcount(x)
    rc = m * (n - Sx.sum(axis=1))
    rca = np.abs(m) * (n + np.abs(Sx).sum(axis=1))
    nd = X.arr((n - 2 * d).astype(np.float64))
    pw = np.empty(n + 1, dtype=Sx.dtype)
    for k in range(n + 1):
        pw[k] = a ** k
    K = pw[d] * (G + h * nd + rc[:, None] + rc[None, :])
    A = pw[d] * (A + h * np.abs(nd) + rca[:, None] + rca[None, :])
    return K, A


def rowsums(K):
    """(r, T): r_b = sum over b' != b by index (the diagonal entry left out, duplicates of the state kept).  The diagonal
    is set to 0 before the sum, not subtracted after it: at n = 63, l = 1/63 it is 1e10 times a row's other entries."""
    K = np.array(K, copy=True)
    np.fill_diagonal(K, 0)
    r = K.sum(axis=1)
    return r, r.sum()


def scores(packed, idx, n, p_floor=1e-30, X=None):
    """(S [B, n], ratio [B, n], k [n]): S[b, i] = 1 - prod_v max(f_v(flip_i z_b), p_floor) / max(f_v(z_b), p_floor) over
    node i's own factor and its children's (k_i of them); every other factor cancels exactly."""
    X = X or hp.arithmetic()
    role, npar, par, off = (np.asarray(packed[k]) for k in ("role", "n_parents", "parents", "cpt_off"))
    if (role == -3).any():
        raise ValueError("summed-out node")
    cpt = X.arr(packed["cpt"])
    fl = X.arr(np.float64(p_floor))
    V = len(role)
    bits = sm.bits_of_idx(idx, n)
    Bn = bits.shape[0]
    vals = np.zeros((Bn, V), np.int64)
    for v in range(V):
        if role[v] >= 0:
            vals[:, v] = bits[:, role[v]]
        elif role[v] == -2:
            vals[:, v] = 1

    def factor(v, vl):
        cfg = np.zeros(Bn, np.int64)
        for p in range(int(npar[v])):
            cfg = cfg * 2 + vl[:, par[v, p]]
        return np.maximum(cpt[int(off[v]) + 2 * cfg + vl[:, v]], fl)

    S, R = X.zeros((Bn, n)), X.zeros((Bn, n))
    k = np.zeros(n, np.int64)
    for i in range(n):
        vi = int(np.nonzero(role == i)[0][0])
        nodes = [v for v in range(V) if v == vi or vi in [int(q) for q in par[v, :int(npar[v])]]]
        k[i] = len(nodes)
        fv = vals.copy()
        fv[:, vi] ^= 1
        ratio = X.arr(np.ones(Bn))
        for v in nodes:
            ratio = ratio * (factor(v, fv) / factor(v, vals))
        S[:, i] = 1 - ratio
        R[:, i] = np.abs(ratio)
    return S, R, k


def weights(r, T, B):
    """(U, m, w) of the estimator from the row sums and their total."""
    U = T / (B * (B - 1))
    m = (T - 2 * r) / ((B - 1) * (B - 2))
    w = (2.0 / B) * (r / (B - 1) - m)
    return U, m, w


def pairs_geometry(B):
    """(tiles per column range, G): rows in blocks of 64, columns in tiles of 32; G = min(64, tiles, ceil(1024 / row blocks))
    column ranges wanted, per = ceil(tiles / wanted) tiles each, G = ceil(tiles / per)."""
    rb, tiles = (B + 63) // 64, (B + 31) // 32
    want = max(1, min(64, tiles, (1024 + rb - 1) // rb))
    per = (tiles + want - 1) // want
    return per, (tiles + per - 1) // per


def c_entry(n):
    """Derived C of one kappa entry of the row-sum kernel, units of EPS64 x its own absolute-term sum A (<= 4 B~), counted in
    half-units (one rounding each): a feature pair costs at most 4 (t - sigma; h rounded, h t' or h (t' - sigma')),
    the MFMA chain 3 n + 3 accumulations, h (n - 2 d) 2, the two constants m (n - sum s) n + 2 each, the three additions of
    the epilogue 3, a^d 1 and the final product 1: 5 n + 18 half-units."""
    return (5 * n + 18) / 2.0


def c_sum(B):
    """Derived C of a row sum over the entries' magnitudes: per column range a chain of 2 additions per tile, a 16-lane
    butterfly (4), then the G partials in order: half a unit each."""
    per, G = pairs_geometry(B)
    return (2 * per + 4 + G) / 2.0


def c_total(B):
    """The total on top of a row sum: ceil(B / 256) additions per thread, a 64-lane butterfly (6), four waves (3)."""
    return ((B + 255) // 256 + 9) / 2.0


AMPLIFICATION = 4.0     # A <= 4 B~ for n l >= 1 (test_ksd_sampled_host.py checks 3.4 on its grid)


# ---------------------------------------------------------------------------------------------- float64 restatement
def replay(cores0, packed, B, seed, epochs, lr, length_scale=1.0, objective="ksd2", optimizer_type="adam", clip=10.0,
           p_floor=1e-30, margin=1e-8):
    """SampledKSDVariationalInference.train on the CPU in float64: dict loss (U), grad_norm per epoch, idx of every epoch,
    the final cores and `undecided` (mps_sampled_mirror.sample), over the whole run."""
    cores = torch.nn.Parameter(torch.as_tensor(np.asarray(cores0), dtype=torch.float64).clone())
    n = cores.shape[0]
    opt = torch.optim.Adam([cores], lr=lr) if optimizer_type == "adam" else torch.optim.SGD([cores], lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr / 10)
    hist = {"loss": [], "grad_norm": [], "idx": [], "undecided": 0}
    for ep in range(epochs):
        opt.zero_grad()
        s = sm.sample(cores.detach().numpy(), seed, ep, B, dtype=np.float64, margin=margin)
        hist["undecided"] += s["undecided"]
        S, _, _ = scores(packed, s["idx"], n, p_floor, X=F64)
        K, _, _ = kappa_bound(s["idx"], S, n, length_scale, X=F64)
        r, T = rowsums(K)
        U, _, w = weights(r, T, B)
        if objective == "ksd":
            w = w * (0.0 if U < 1e-12 else 0.5 / math.sqrt(U))
        lq = sm.logq_torch(cores, s["bits"])
        (lq * torch.as_tensor(w)).sum().backward()
        gn = torch.nn.utils.clip_grad_norm_([cores], clip)
        opt.step()
        sched.step()
        hist["loss"].append(float(U))
        hist["grad_norm"].append(float(gn))
        hist["idx"].append(s["idx"])
    hist["cores"] = cores.detach().numpy().copy()
    return hist
