"""Oracle of the locally purified sampled MPS Born machine (test infrastructure, plain NumPy / CPU torch, not under test).

Conventions (include/bornvi_lps.h and kernels_lps.hip state the same):
  Parameter layout.  cores is float64 [n, 2, m, D, D], real: A_k[s, mu] in R^{D x D}, s the bit, mu = 0 .. m - 1 the
    purification index that is summed out.  Bit order, index word and boundary vectors e0 are the real family's: tuple
    position 0 = MSB of the outcome index.
  Amplitude:  psi(z, mu) = e0^T A_1[z_1, mu_1] ... A_n[z_n, mu_n] e0.
  Unnormalised mass:  T(z) = sum_{mu_1 .. mu_n} psi(z, mu)^2.   Normaliser and distribution:  Z = sum_z T(z),  q = T / Z.
  Left density:  rho_0 = e0 e0^T,  rho_k = sum_mu A_k[z_k, mu]^T rho_{k-1} A_k[z_k, mu];  T(z) = rho_n[0, 0].
  Right density:  R_n = e0 e0^T,  R_{k-1} = sum_mu A_k[z_k, mu] R_k A_k[z_k, mu]^T.
  Environments:  E_n = e0 e0^T,  E_{k-1} = sum_{s,mu} A_k[s, mu] E_k A_k[s, mu]^T;   L_0 = e0 e0^T,
    L_k = sum_{s,mu} A_k[s, mu]^T L_{k-1} A_k[s, mu];   Z = E_0[0, 0].
  Gradient of sum_b w_b log q(z_b).  Sample term: the block [k, z_{b,k}, mu] receives
    (2 w_b / T_b) rho_{b,k-1} A_k[z_{b,k}, mu] R_{b,k}.   Environment term: every block [k, s, mu] loses
    (sum_b w_b) 2 L_{k-1} A_k[s, mu] E_k / Z.
  Sampler: (z_k, mu_k) jointly with pure-state vectors.  u_{s,mu} = l A_k[s, mu], m_{s,mu} = u E_k u^T;  M0 = sum_mu m_{0,mu},
    M1 likewise, ascending mu;  M = M0 + M1;  z_k = [U_k M >= M0];  mu_k = the number of partial sums c_j = m_{z,0} + ... + m_{z,j},
    j < m - 1, with U_k M - z_k M0 >= c_j;  l <- u_{z_k,mu_k}.  aux: mu_k at bits 2 ((k - 1) mod 32) of word (k - 1) / 32.

Everything but `replay` works in np.longdouble where hp_reference.HAVE_LONGDOUBLE holds (else float64), or in the dtype given
(np.float64: the float64 evaluation hp.measured_constant wants), and without any rescaling.  The absolute-value majorants run the
same recursions over |cores|.
  brute_force, environments, densities, masses_on_prefix, decide, sample, score_gradient, exact_elbo_gradient, replay,
  and the derived error counts c_env, c_T, logq_bound, c_score of the GPU tests.
"""
import itertools
import math

import numpy as np
import torch

import hp_reference as hp
import mps_sampled_mirror as sm
from mps_sampled_mirror import bits_of_idx, idx_of_bits, log_joint, uniforms  # noqa: F401

LD = sm.LD


def _dt(dtype):
    return LD if dtype is None else dtype


FREQ_SEED = 77          # the sampler-frequency tests' seed (host: the mirror alone; GPU: the kernel), chosen on the CPU


def random_cores(n, m, D, seed, spread=0.3):
    """Test cores: (identity in mu = 0 + spread x normal) / sqrt 2, float64 [n, 2, m, D, D]."""
    rng = np.random.default_rng(seed)
    c = spread * rng.standard_normal((n, 2, m, D, D))
    c[:, :, 0] += np.eye(D)
    return c / np.sqrt(2.0)


def all_bits(n):
    return bits_of_idx(np.arange(1 << n, dtype=np.int64), n)


def brute_force(cores, dtype=None):
    """(T [2^n], q [2^n]) by the definition: every (z, mu) amplitude as a product of matrices, squared and summed over mu."""
    dtype = _dt(dtype)
    A = np.asarray(cores, dtype=np.float64).astype(dtype)
    n, _, m, D, _ = A.shape
    T = np.zeros(1 << n, dtype)
    for z in range(1 << n):
        zb = [(z >> (n - 1 - k)) & 1 for k in range(n)]
        for mu in itertools.product(range(m), repeat=n):
            v = np.zeros(D, dtype)
            v[0] = 1
            for k in range(n):
                v = v @ A[k, zb[k], mu[k]]
            T[z] += v[0] * v[0]
    return T, T / T.sum()


def environments(cores, dtype=None):
    """dict E [n + 1, D, D], L [n + 1, D, D], Z, and E_abs, L_abs, Z_abs from |cores|."""
    dtype = _dt(dtype)
    cores = np.asarray(cores, dtype=np.float64)
    n, _, m, D, _ = cores.shape
    out = {}
    for tag, A in (("", cores.astype(dtype)), ("_abs", np.abs(cores).astype(dtype))):
        A = A.reshape(n, 2 * m, D, D)
        E = np.zeros((n + 1, D, D), dtype)
        L = np.zeros((n + 1, D, D), dtype)
        E[n, 0, 0] = 1
        L[0, 0, 0] = 1
        for k in range(n, 0, -1):
            E[k - 1] = sum(A[k - 1, j] @ E[k] @ A[k - 1, j].T for j in range(2 * m))
        for k in range(1, n + 1):
            L[k] = sum(A[k - 1, j].T @ L[k - 1] @ A[k - 1, j] for j in range(2 * m))
        out["E" + tag], out["L" + tag], out["Z" + tag] = E, L, E[0, 0, 0]
    return out


def _left_step(rho, Ak):
    """sum_mu A^T rho A per sample: rho [B, D, D], Ak [B, m, D, D]."""
    return sum(np.matmul(Ak[:, mu].transpose(0, 2, 1), np.matmul(rho, Ak[:, mu])) for mu in range(Ak.shape[1]))


def _right_step(R, Ak):
    return sum(np.matmul(Ak[:, mu], np.matmul(R, Ak[:, mu].transpose(0, 2, 1))) for mu in range(Ak.shape[1]))


def _e0(Bn, D, dtype):
    X = np.zeros((Bn, D, D), dtype)
    X[:, 0, 0] = 1
    return X


def _right_stack(A, bits, dtype):
    """R [n + 1, B, D, D] of cores A [n, 2, m, D, D] along the samples' bits."""
    n, _, m, D, _ = A.shape
    R = np.zeros((n + 1, bits.shape[0], D, D), dtype)
    R[n] = _e0(bits.shape[0], D, dtype)
    for k in range(n, 0, -1):
        R[k - 1] = _right_step(R[k], A[k - 1][bits[:, k - 1]])
    return R


def _left_stack(A, bits, dtype):
    n, _, m, D, _ = A.shape
    rho = np.zeros((n + 1, bits.shape[0], D, D), dtype)
    rho[0] = _e0(bits.shape[0], D, dtype)
    for k in range(1, n + 1):
        rho[k] = _left_step(rho[k - 1], A[k - 1][bits[:, k - 1]])
    return rho


def _left_T(A, bits, dtype):
    """T [B] = rho_n[0, 0] without keeping the stack."""
    n, _, m, D, _ = A.shape
    rho = _e0(bits.shape[0], D, dtype)
    for k in range(1, n + 1):
        rho = _left_step(rho, A[k - 1][bits[:, k - 1]])
    return rho[:, 0, 0].copy()


def densities(cores, bits, dtype=None):
    """dict rho, R [n + 1, B, D, D], T [B] = rho_n[0, 0], and rho_abs, R_abs, T_abs from |cores| (small shapes: four stacks)."""
    dtype = _dt(dtype)
    cores = np.asarray(cores, dtype=np.float64)
    A, Aa = cores.astype(dtype), np.abs(cores).astype(dtype)
    rho, rhoa = _left_stack(A, bits, dtype), _left_stack(Aa, bits, dtype)
    return {"rho": rho, "R": _right_stack(A, bits, dtype), "T": rho[-1][:, 0, 0], "rho_abs": rhoa, "R_abs": _right_stack(Aa, bits, dtype),
            "T_abs": rhoa[-1][:, 0, 0]}


def logq_of(cores, bits, env=None, dtype=None):
    """dict logq [B] = log T - log Z, T, T_abs, kappa = T_abs / T."""
    dtype = _dt(dtype)
    env = env or environments(cores, dtype)
    cores = np.asarray(cores, dtype=np.float64)
    T, Ta = _left_T(cores.astype(dtype), bits, dtype), _left_T(np.abs(cores).astype(dtype), bits, dtype)
    with np.errstate(divide="ignore"):
        logq = np.log(T) - np.log(env["Z"])
    ok = T != 0
    return {"logq": logq, "T": T, "T_abs": Ta, "kappa": np.where(ok, Ta / np.where(ok, T, 1), np.inf)}


# ---------------------------------------------------------------------------------------------- the sampler
def aux_of_mus(mus):
    """int64 [B, 2] from mu draws [B, n]: two bits a site, sites 1 .. 32 in word 0, 33 .. 63 in word 1."""
    Bn, n = mus.shape
    aux = np.zeros((Bn, 2), np.uint64)
    for k in range(1, n + 1):
        aux[:, (k - 1) // 32] |= mus[:, k - 1].astype(np.uint64) << np.uint64(2 * ((k - 1) % 32))
    return aux.view(np.int64)


def mus_of_aux(aux, n):
    aux = np.asarray(aux, dtype=np.int64).view(np.uint64)
    mus = np.zeros((aux.shape[0], n), np.int64)
    for k in range(1, n + 1):
        mus[:, k - 1] = ((aux[:, (k - 1) // 32] >> np.uint64(2 * ((k - 1) % 32))) & np.uint64(3)).astype(np.int64)
    return mus


def decide(masses, U, margin=2.0 ** -40):
    """The joint-draw rule on masses [B, 2, m] with uniforms U [B] -> (z [B], mu [B], undecided: the draws with U M within
    margin * M of one of the thresholds it is compared with)."""
    dtype = masses.dtype
    Bn, _, m = masses.shape
    c = np.zeros((Bn, 2, m), dtype)                       # ascending partial sums per s
    c[:, :, 0] = masses[:, :, 0]
    for j in range(1, m):
        c[:, :, j] = c[:, :, j - 1] + masses[:, :, j]
    M0, M1 = c[:, 0, m - 1], c[:, 1, m - 1]
    M = M0 + M1
    x = U.astype(dtype) * M
    z = x >= M0
    close = np.abs(x - M0) <= margin * M
    v = np.where(z, x - M0, x)
    cz = np.where(z[:, None], c[:, 1], c[:, 0])
    mu = np.zeros(Bn, np.int64)
    for j in range(m - 1):
        mu += (v >= cz[:, j]).astype(np.int64)
        close |= np.abs(v - cz[:, j]) <= margin * M
    return z.astype(np.int64), mu, int(close.sum())


def _site_masses(l, Ak, Ek):
    """u [B, 2, m, D] = l A_k[s, mu] and m [B, 2, m] = u E_k u^T."""
    u = np.einsum('ba,smac->bsmc', l, Ak)
    return u, (np.matmul(u, Ek) * u).sum(axis=-1)


def masses_on_prefix(cores, bits, mus, env=None, dtype=None):
    """masses [n, B, 2, m] at every site along each sample's own prefix of (bits, mus)."""
    dtype = _dt(dtype)
    A = np.asarray(cores, dtype=np.float64).astype(dtype)
    n, _, m, D, _ = A.shape
    env = env or environments(cores, dtype)
    Bn = bits.shape[0]
    l = np.zeros((Bn, D), dtype)
    l[:, 0] = 1
    out = np.zeros((n, Bn, 2, m), dtype)
    ar = np.arange(Bn)
    for k in range(1, n + 1):
        u, out[k - 1] = _site_masses(l, A[k - 1], env["E"][k])
        l = u[ar, bits[:, k - 1], mus[:, k - 1]]
        mx = np.abs(l).max(axis=1, keepdims=True)          # any positive scale: the rule is homogeneous in l
        l = l / np.where(mx > 0, mx, 1)
    return out


def sample(cores, seed, epoch, B, dtype=None, margin=2.0 ** -40):
    """The sampler with the kernel's uniforms: dict bits [B, n], mus [B, n], idx [B], aux [B, 2], undecided."""
    dtype = _dt(dtype)
    A = np.asarray(cores, dtype=np.float64).astype(dtype)
    n, _, m, D, _ = A.shape
    env = environments(cores, dtype)
    U = uniforms(seed, epoch, np.arange(B), n)
    l = np.zeros((B, D), dtype)
    l[:, 0] = 1
    bits, mus = np.zeros((B, n), np.int64), np.zeros((B, n), np.int64)
    undecided = 0
    ar = np.arange(B)
    for k in range(1, n + 1):
        u, ms = _site_masses(l, A[k - 1], env["E"][k])
        z, mu, und = decide(ms, U[:, k - 1], margin)
        undecided += und
        bits[:, k - 1], mus[:, k - 1] = z, mu
        l = u[ar, z, mu]
        mx = np.abs(l).max(axis=1, keepdims=True)
        l = l / np.where(mx > 0, mx, 1)
    return {"bits": bits, "mus": mus, "idx": idx_of_bits(bits), "aux": aux_of_mus(mus), "undecided": undecided}


def joint_probabilities(cores, dtype=None):
    """P(z, mu) of the joint-draw rule, [2^n, m^n], by the chain rule over the exact conditionals m_{s,mu} / M (small n)."""
    dtype = _dt(dtype)
    A = np.asarray(cores, dtype=np.float64).astype(dtype)
    n, _, m, D, _ = A.shape
    env = environments(cores, dtype)
    P = np.zeros((1 << n, m ** n), dtype)
    for z in range(1 << n):
        zb = [(z >> (n - 1 - k)) & 1 for k in range(n)]
        for i, mu in enumerate(itertools.product(range(m), repeat=n)):
            l = np.zeros((1, D), dtype)
            l[0, 0] = 1
            p = dtype(1)
            for k in range(1, n + 1):
                u, ms = _site_masses(l, A[k - 1], env["E"][k])
                p = p * ms[0, zb[k - 1], mu[k - 1]] / ms[0].sum()
                l = u[:, zb[k - 1], mu[k - 1]]
            P[z, i] = p
    return P


# ---------------------------------------------------------------------------------------------- the gradient
def score_gradient(cores, bits, w, env=None, dtype=None):
    """dict grad [n, 2, m, D, D] = sum_b w_b grad log q(z_b), grad_abs (every term's magnitude: |cores|, |w|, + for -, divided
    by the true T_b and the true Z), logq, T, T_abs, kappa (T_abs / T per sample)."""
    dtype = _dt(dtype)
    cores = np.asarray(cores, dtype=np.float64)
    n, _, m, D, _ = cores.shape
    env = env or environments(cores, dtype)
    A, Aa = cores.astype(dtype), np.abs(cores).astype(dtype)
    wl = np.asarray(w, dtype=np.float64).astype(dtype)
    R, Ra = _right_stack(A, bits, dtype), _right_stack(Aa, bits, dtype)      # the left densities run beside the site loop
    T, Ta = R[0][:, 0, 0].copy(), Ra[0][:, 0, 0].copy()
    ok = T != 0
    safe = np.where(ok, T, 1)
    coef = np.where(ok, 2 * wl / safe, 0)
    coefa = np.where(ok, 2 * np.abs(wl) / np.abs(safe), 0)
    W, Wa = wl.sum(), np.abs(wl).sum()
    grad, grada = np.zeros(cores.shape, dtype), np.zeros(cores.shape, dtype)
    Bn = bits.shape[0]
    rho, rhoa = _e0(Bn, D, dtype), _e0(Bn, D, dtype)

    def block(c, X, Amat, Y):
        """sum_b c_b X_b A Y_b."""
        left = np.matmul(c[:, None, None] * X, Amat)                                  # [B, D, D]
        return left.transpose(1, 0, 2).reshape(D, -1) @ Y.reshape(-1, D)
    for k in range(1, n + 1):
        for s in (0, 1):
            rows = bits[:, k - 1] == s
            for mu in range(m):
                grad[k - 1, s, mu] = block(coef[rows], rho[rows], A[k - 1, s, mu], R[k][rows]) \
                    - W * 2 * (env["L"][k - 1] @ A[k - 1, s, mu] @ env["E"][k]) / env["Z"]
                grada[k - 1, s, mu] = block(coefa[rows], rhoa[rows], Aa[k - 1, s, mu], Ra[k][rows]) \
                    + Wa * 2 * (env["L_abs"][k - 1] @ Aa[k - 1, s, mu] @ env["E_abs"][k]) / env["Z"]
        rho, rhoa = _left_step(rho, A[k - 1][bits[:, k - 1]]), _left_step(rhoa, Aa[k - 1][bits[:, k - 1]])
    T, Ta = rho[:, 0, 0].copy(), rhoa[:, 0, 0].copy()                                 # logq from the left sweep, as the kernel
    with np.errstate(divide="ignore"):
        logq = np.log(T) - np.log(env["Z"])
    return {"grad": grad, "grad_abs": grada, "logq": logq, "T": T, "T_abs": Ta,
            "kappa": np.where(ok, Ta / np.abs(safe), np.inf)}


def exact_elbo_gradient(cores, logp, dtype=None):
    """The exact gradient of sum_z q(z) (log q(z) - log p(z)) over all 2^n states: the score identity."""
    n = np.asarray(cores).shape[0]
    bits = all_bits(n)
    lq = logq_of(cores, bits, dtype=dtype)["logq"]
    q = np.exp(lq)
    f = lq - np.asarray(logp, dtype=np.float64)
    return score_gradient(cores, bits, hp.to_f64(q * f), dtype=dtype)["grad"]


# ---------------------------------------------------------------------------------------------- derived error counts
# Units of EPS64, derived from the kernels' chains in the docstring of test_gpu_lps_kernel.py; kept here so that the kernel and
# the trainer tests share one statement of them.
TILE, MAX_WG_SMALL, MAX_WG_LARGE = 16, 1024, 256      # include/bornvi_lps.h: BORNVI_LPS_SCORE_TILE, BORNVI_LPS_MAX_WG_*
WAVES = 4                                             # kernels_lps.hip: LP_WAVES, each wave owns TILE / WAVES samples of a tile


def max_wg(D):
    return MAX_WG_LARGE if D > 8 else MAX_WG_SMALL


def geometry(B, D):
    """(workgroups G, tiles per workgroup) of the score kernel."""
    tiles = -(-B // TILE)
    G = min(tiles, max_wg(D))
    return G, -(-tiles // G)


def c_env(j, m, D):
    """E_k, L_k after j steps against the majorant environment: a D-term chain (T_j) and a 2 m D-term one, and the store."""
    return float(j * ((2 * m + 1) * D + 1))


def c_T(j, m, D):
    """A density after j steps against its majorant: per step a D-term product (rho A) and an m D-term one, each matrix-core
    term counted twice (the product sum and the accumulation)."""
    return float(j * 2 * D * (m + 1))


def logq_bound(n, m, D, kappa_b, kappa_Z, logq, logZ):
    lT = np.where(np.isfinite(logq), logq + logZ, 0.0)
    return c_T(n, m, D) * kappa_b + c_env(n, m, D) * kappa_Z + 8 * (np.abs(lT) + abs(logZ) + 4)


def c_score(n, m, D, B, kappa_max, kappa_Z):
    G, tiles = geometry(B, D)
    sample = c_T(n - 1, m, D) + c_T(n, m, D) * kappa_max + 3 + 2 * D + 2 * (TILE // WAVES) * D + WAVES * tiles + G
    envt = c_env(n - 1, m, D) + 2 * D + c_env(n, m, D) * kappa_Z + TILE * tiles + 6 + (-(-G // 256)) + 3 + 4
    return 1.0 + max(sample, envt)


# ---------------------------------------------------------------------------------------------- float64 torch restatement
def logq_torch(cores, bits):
    """log q(z_b) [B], differentiable in cores float64 [n, 2, m, D, D]: the left densities by einsum, Z by the right environments."""
    n, _, m, D, _ = cores.shape
    Bt = torch.as_tensor(bits, dtype=torch.int64)
    rho = torch.zeros(Bt.shape[0], D, D, dtype=torch.float64)
    rho[:, 0, 0] = 1.0
    for k in range(n):
        Ak = cores[k][Bt[:, k]]
        rho = torch.einsum('bmac,bad,bmde->bce', Ak, rho, Ak)
    E = torch.zeros(D, D, dtype=torch.float64)
    E[0, 0] = 1.0
    for k in range(n - 1, -1, -1):
        Ak = cores[k].reshape(2 * m, D, D)
        E = torch.einsum('jac,cd,jed->ae', Ak, E, Ak)
    return torch.log(rho[:, 0, 0]) - torch.log(E[0, 0])


def autograd_score(cores, bits, w):
    A = torch.tensor(np.asarray(cores, dtype=np.float64), requires_grad=True)
    (logq_torch(A, bits) * torch.as_tensor(np.asarray(w, dtype=np.float64))).sum().backward()
    return A.grad.numpy()


def elbo_weights(packed, p_floor=1e-30):
    """The sampled ELBO trainer's (loss, w) from an epoch's (idx, bits, logq)."""
    def weights(idx, bits, logq):
        f = logq - log_joint(packed, bits, p_floor)
        loss = f.mean()
        B = len(f)
        return float(loss), ((f - loss) / (B - 1) if B > 1 else f.copy())
    return weights


def ksd_weights(packed, n, length_scale=1.0, p_floor=1e-30):
    """The sampled KSD trainer's (U, w) (objective ksd2), through ksd_sampled_mirror's float64 pieces."""
    import ksd_sampled_mirror as km

    def weights(idx, bits, logq):
        S, _, _ = km.scores(packed, idx, n, p_floor, X=km.F64)
        K, _, _ = km.kappa_bound(idx, S, n, length_scale, X=km.F64)
        r, T = km.rowsums(K)
        U, _, w = km.weights(r, T, len(idx))
        return float(U), np.asarray(w, dtype=np.float64)
    return weights


def mmd_weights(data, n, kappa):
    """The sampled MMD trainer's (U, w), through mmd_mirror.sampled."""
    import mmd_mirror as mq

    def weights(idx, bits, logq):
        U, w, _, _, _ = mq.sampled(idx, np.asarray(data), n, kappa)
        return float(U), np.asarray(w, dtype=np.float64)
    return weights


def replay(cores0, weights, B, seed, epochs, lr, optimizer_type="adam", clip=10.0, margin=1e-8):
    """SampledTrainer.train with purified cores on the CPU in float64: mps_sampled_mirror.replay's loop (Adam, cosine schedule,
    clip) with this family's sampler and log q; `weights` (elbo_weights, ksd_weights, mmd_weights) is the objective."""
    cores = torch.nn.Parameter(torch.as_tensor(np.asarray(cores0), dtype=torch.float64).clone())
    opt = torch.optim.Adam([cores], lr=lr) if optimizer_type == "adam" else torch.optim.SGD([cores], lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr / 10)
    hist = {"loss": [], "grad_norm": [], "idx": [], "undecided": 0}
    for ep in range(epochs):
        opt.zero_grad()
        s = sample(cores.detach().numpy(), seed, ep, B, dtype=np.float64, margin=margin)
        hist["undecided"] += s["undecided"]
        lq = logq_torch(cores, s["bits"])
        loss, w = weights(s["idx"], s["bits"], lq.detach().numpy())
        (lq * torch.as_tensor(w)).sum().backward()
        gn = torch.nn.utils.clip_grad_norm_([cores], clip)
        opt.step()
        sched.step()
        hist["loss"].append(float(loss))
        hist["grad_norm"].append(float(gn))
        hist["idx"].append(s["idx"])
    hist["cores"] = cores.detach().numpy().copy()
    return hist
