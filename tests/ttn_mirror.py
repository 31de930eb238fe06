"""Oracle of the tree-tensor-network sampled Born machine (test infrastructure, plain NumPy / CPU torch, not under test).

Conventions (include/bornvi_ttn.h and kernels_ttn.hip state the same):
  Tree.  h = max(1, ceil(log2 n)), L = 2^h leaf positions, 1 <= n <= 63, so L <= 64.  Position j < n holds tuple position j:
    z_{j+1}, bit n - 1 - j of the int64 outcome index, the real family's bit order.  Positions j >= n are padding and carry
    the fixed value 0.  Nodes are heap-numbered v = 1 .. L - 1, their children are 2 v and 2 v + 1; nodes v >= L / 2 are
    bottom nodes, their children are the positions 2 (v - L / 2) and 2 (v - L / 2) + 1.
  Parameter.  cores float64 [L - 1, D, D, D]: cores[v - 1] = T_v[p, a, b], p the parent bond, a, b the left and right
    child bonds.  A leaf is the one-hot vector e_z in R^D, so a bottom node is an ordinary node whose children are one-hot.
  Dead entries.  Never read, and their gradient is exactly 0.0: the root at p >= 1; a bottom node at a >= 2 or b >= 2; a
    bottom node at the value 1 of a padding child.
  Amplitude.  x_v[p] = sum_{a,b} T_v[p, a, b] x_{2v}[a] x_{2v+1}[b], contracted as M = T x_{2v} over a, then M x_{2v+1} over b;
    psi(z) = x_1[0];  Z = sum_z psi(z)^2;  q = psi^2 / Z.
  Environments.  Up densities: U_v = sum_{z in the subtree} x_v x_v^T (padding values are not summed over).  Down densities:
    V_1 = e0 e0^T,  V_{2v}[a, a'] = sum V_v[p, p'] T[p, a, b] T[p', a', b'] U_{2v+1}[b, b'],  V_{2v+1} the same with U_{2v}.
    Z = U_1[0, 0].  dZ/dT_v[p, a, b] = 2 sum V_v[p, p'] T_v[p', a', b'] U_{2v}[a, a'] U_{2v+1}[b, b'].
  Per-sample down vectors.  y_1 = e0,  y_{2v}[a] = sum y_v[p] T[p, a, b] x_{2v+1}[b],  y_{2v+1}[b] = sum y_v[p] T[p, a, b] x_{2v}[a].
  Gradient of sum_b w_b log q(z_b).  Block v receives sum_b (2 w_b / psi_b) y_{b,v} (x) x_{b,2v} (x) x_{b,2v+1} and loses
    (sum_b w_b) dZ/dT_v / Z.
  Sampler.  Depth first, positions left to right, exact.  Node v has the density P_v of everything outside its subtree (drawn
    positions as pure vectors, undrawn ones traced), P_1 = e0 e0^T.  At a node:
    P_{2v}[a, a'] = sum P_v[p, p'] T[p, a, b] T[p', a', b'] U_{2v+1}[b, b'];  descend left, which returns x_{2v};  M = T x_{2v},
    P_{2v+1} = M^T P_v M;  descend right;  return x_v = M x_{2v+1}.  A position with density P has the masses m_0 = P[0, 0],
    m_1 = P[1, 1] and draws z = [U (m_0 + m_1) >= m_0]; a padding position draws nothing and is 0.  U for position j is
    bornvi_mps_sample's Philox4x32-10 uniform at (seed, epoch, b, k = j + 1).

Everything but `replay` works in np.longdouble where hp_reference.HAVE_LONGDOUBLE holds (else float64), or in the dtype given
(np.float64: the float64 evaluation hp.measured_constant wants), and without any rescaling (the sampler's densities are divided
by their largest entry: the draw is homogeneous in them).  The absolute-value majorants run the same recursions over |cores|.
  tree_shape, live_mask, brute_force, environments, up_down, logq_of, walk (masses_on_prefix, chain_probability, sample),
  score_gradient, exact_elbo_gradient, replay, and the derived error counts c_x, c_u, c_v, c_y, logq_bound, c_score of the GPU tests.
"""
import numpy as np
import torch

import hp_reference as hp
import lps_mirror as lp
import mps_sampled_mirror as sm
from lps_mirror import decide, elbo_weights, ksd_weights, mmd_weights  # noqa: F401
from mps_sampled_mirror import bits_of_idx, idx_of_bits, log_joint, uniforms  # noqa: F401

LD = sm.LD

FREQ_SEED = 2          # the sampler-frequency tests' seed (host: the mirror alone; GPU: the kernel), chosen on the CPU
LANES, MAX_WG = 64, 1024      # kernels_ttn.hip: TT_LANES; include/bornvi_ttn.h: BORNVI_TTN_MAX_WG


def _dt(dtype):
    return LD if dtype is None else dtype


def tree_shape(n):
    h = max(1, (n - 1).bit_length())
    return h, 1 << h


def live_mask(n, D):
    """bool [L - 1, D, D, D]: the entries that enter psi."""
    _, L = tree_shape(n)
    live = np.ones((L - 1, D, D, D), bool)
    live[0, 1:] = False
    for v in range(L // 2, L):
        j = 2 * v - L
        live[v - 1, :, 2:, :] = False
        live[v - 1, :, :, 2:] = False
        if j >= n:
            live[v - 1, :, 1, :] = False
        if j + 1 >= n:
            live[v - 1, :, :, 1] = False
    return live


def uniform_cores(n, D):
    """The exactly uniform q: internal nodes e0 (x) e0 (x) e0, bottom nodes 2^(-c/2) at [0, s, s'] over the allowed values."""
    _, L = tree_shape(n)
    live = live_mask(n, D)
    c = np.zeros((L - 1, D, D, D))
    c[:, 0, 0, 0] = 1.0
    for v in range(L // 2, L):
        j = 2 * v - L
        c[v - 1, 0][live[v - 1, 0]] = 2.0 ** (-((j < n) + (j + 1 < n)) / 2.0)
    return c


def random_cores(n, D, seed, spread=0.3):
    """Test cores: the uniform state + spread x normal on the live entries, dead entries 0.0; float64 [L - 1, D, D, D]."""
    rng = np.random.default_rng(seed)
    live = live_mask(n, D)
    return uniform_cores(n, D) + spread * rng.standard_normal(live.shape) * live


def all_bits(n):
    return bits_of_idx(np.arange(1 << n, dtype=np.int64), n)


def _masked(cores, n, dtype, absolute=False):
    c = np.asarray(cores, dtype=np.float64)
    c = np.where(live_mask(n, c.shape[1]), np.abs(c) if absolute else c, 0.0)      # dead entries are never read
    return c.astype(dtype)


def _leaves(bits, n, L, D, dtype):
    """x of the positions [L, B, D]: one-hot of the bit, e0 for padding."""
    Bn = bits.shape[0]
    x = np.zeros((L, Bn, D), dtype)
    for j in range(L):
        z = bits[:, j] if j < n else np.zeros(Bn, np.int64)
        x[j, np.arange(Bn), z] = 1
    return x


def up_down(cores, n, bits, dtype=None, absolute=False, down=True):
    """(x [2 L, B, D] by heap index, leaves included; y [L, B, D] or None) along the samples' bits."""
    dtype = _dt(dtype)
    A = _masked(cores, n, dtype, absolute)
    D = A.shape[1]
    h, L = tree_shape(n)
    Bn = bits.shape[0]
    x = np.zeros((2 * L, Bn, D), dtype)
    x[L:] = _leaves(bits, n, L, D, dtype)
    for v in range(L - 1, 0, -1):
        M = np.einsum('pab,ka->kpb', A[v - 1], x[2 * v])
        x[v] = np.einsum('kpb,kb->kp', M, x[2 * v + 1])
    if not down:
        return x, None
    y = np.zeros((L, Bn, D), dtype)
    y[1, :, 0] = 1
    for v in range(1, L // 2):
        N = np.einsum('kp,pab->kab', y[v], A[v - 1])
        y[2 * v] = np.einsum('kab,kb->ka', N, x[2 * v + 1])
        y[2 * v + 1] = np.einsum('kab,ka->kb', N, x[2 * v])
    return x, y


def brute_force(cores, n, dtype=None):
    """(psi^2 [2^n], q [2^n]) by the definition, every z."""
    x, _ = up_down(cores, n, all_bits(n), dtype, down=False)
    T = x[1][:, 0] ** 2
    return T, T / T.sum()


def environments(cores, n, dtype=None):
    """dict U [2 L, D, D] (leaves included), V [L, D, D], dZ [L - 1, D, D, D], Z, and U_abs, V_abs, dZ_abs, Z_abs from |cores|."""
    dtype = _dt(dtype)
    h, L = tree_shape(n)
    out = {}
    for tag, absolute in (("", False), ("_abs", True)):
        A = _masked(cores, n, dtype, absolute)
        D = A.shape[1]
        U = np.zeros((2 * L, D, D), dtype)
        for j in range(L):
            U[L + j, 0, 0] = 1
            if j < n:
                U[L + j, 1, 1] = 1
        for v in range(L - 1, 0, -1):
            U[v] = np.einsum('pab,qcd,ac,bd->pq', A[v - 1], A[v - 1], U[2 * v], U[2 * v + 1])
        V = np.zeros((L, D, D), dtype)
        V[1, 0, 0] = 1
        for v in range(1, L // 2):
            V[2 * v] = np.einsum('pq,pab,qcd,bd->ac', V[v], A[v - 1], A[v - 1], U[2 * v + 1])
            V[2 * v + 1] = np.einsum('pq,pab,qcd,ac->bd', V[v], A[v - 1], A[v - 1], U[2 * v])
        dZ = np.zeros(A.shape, dtype)
        for v in range(1, L):
            dZ[v - 1] = 2 * np.einsum('pq,qcd,ac,bd->pab', V[v], A[v - 1], U[2 * v], U[2 * v + 1])
        out["U" + tag], out["V" + tag], out["dZ" + tag], out["Z" + tag] = U, V, dZ, U[1, 0, 0]
    return out


def logq_of(cores, n, bits, env=None, dtype=None):
    """dict logq [B] = log psi^2 - log Z, psi, psi_abs, kappa = psi_abs / |psi|."""
    dtype = _dt(dtype)
    env = env or environments(cores, n, dtype)
    psi = up_down(cores, n, bits, dtype, down=False)[0][1][:, 0]
    pa = up_down(cores, n, bits, dtype, absolute=True, down=False)[0][1][:, 0]
    with np.errstate(divide="ignore"):
        logq = np.log(psi * psi) - np.log(env["Z"])
    ok = psi != 0
    return {"logq": logq, "psi": psi, "psi_abs": pa, "kappa": np.where(ok, pa / np.abs(np.where(ok, psi, 1)), np.inf)}


# ---------------------------------------------------------------------------------------------- the sampler
def walk(cores, n, B, U=None, forced=None, env=None, dtype=None, margin=2.0 ** -40):
    """The depth-first walk for B samples: with `forced` bits [B, n] along those, else drawing with the uniforms U [B, n].
    dict bits [B, n], masses [n, B, 2] (m_0, m_1 of every position on the sample's own prefix), psi [B] = x_1[0], undecided."""
    dtype = _dt(dtype)
    env = env or environments(cores, n, dtype)
    A = _masked(cores, n, dtype)
    D = A.shape[1]
    h, L = tree_shape(n)
    bits = np.zeros((B, n), np.int64)
    masses = np.zeros((n, B, 2), dtype)
    state = {"undecided": 0}

    def scaled(P):
        mx = np.abs(P).max(axis=(1, 2), keepdims=True)
        return P / np.where(mx > 0, mx, 1)

    def descend(v, P):
        if v >= L:
            j = v - L
            x = np.zeros((B, D), dtype)
            if j >= n:
                x[:, 0] = 1
                return x
            masses[j, :, 0], masses[j, :, 1] = P[:, 0, 0], P[:, 1, 1]
            if forced is not None:
                z = forced[:, j]
            else:
                z, _, und = decide(masses[j][:, :, None], U[:, j], margin)
                state["undecided"] += und
            bits[:, j] = z
            x[np.arange(B), z] = 1
            return x
        T = A[v - 1]
        Y = np.einsum('kpq,pad->kqad', P, np.einsum('pab,bd->pad', T, env["U"][2 * v + 1]))
        xl = descend(2 * v, scaled(np.einsum('kqad,qcd->kac', Y, T)))
        M = np.einsum('pab,ka->kpb', T, xl)
        xr = descend(2 * v + 1, scaled(np.einsum('kqb,kqd->kbd', np.einsum('kpb,kpq->kqb', M, P), M)))
        return np.einsum('kpb,kb->kp', M, xr)
    P1 = np.zeros((B, D, D), dtype)
    P1[:, 0, 0] = 1
    x1 = descend(1, P1)
    return {"bits": bits, "masses": masses, "psi": x1[:, 0], "undecided": state["undecided"]}


def masses_on_prefix(cores, n, bits, env=None, dtype=None):
    """masses [n, B, 2] at every position along each sample's own bits."""
    return walk(cores, n, bits.shape[0], forced=bits, env=env, dtype=dtype)["masses"]


def chain_probability(cores, n, bits, env=None, dtype=None):
    """The product over the positions of the sampler's conditionals m_z / (m_0 + m_1) along the bits: q(z) if the sampler is exact."""
    m = masses_on_prefix(cores, n, bits, env, dtype)
    p = np.ones(bits.shape[0], m.dtype)
    for j in range(n):
        p = p * m[j, np.arange(bits.shape[0]), bits[:, j]] / m[j].sum(axis=1)
    return p


def sample(cores, n, seed, epoch, B, dtype=None, margin=2.0 ** -40):
    """The sampler with the kernel's uniforms: dict bits [B, n], idx [B], logq [B], undecided."""
    dtype = _dt(dtype)
    env = environments(cores, n, dtype)
    r = walk(cores, n, B, U=uniforms(seed, epoch, np.arange(B), n), env=env, dtype=dtype, margin=margin)
    with np.errstate(divide="ignore"):
        logq = np.log(r["psi"] ** 2) - np.log(env["Z"])
    return {"bits": r["bits"], "idx": idx_of_bits(r["bits"]), "logq": logq, "undecided": r["undecided"]}


# ---------------------------------------------------------------------------------------------- the gradient
def score_gradient(cores, n, bits, w, env=None, dtype=None):
    """dict grad [L - 1, D, D, D] = sum_b w_b grad log q(z_b) (0 in the dead entries), grad_abs (every term's magnitude: |cores|,
    |w|, + for -, divided by the true psi_b and the true Z), logq, psi, psi_abs, kappa (psi_abs / |psi| per sample)."""
    dtype = _dt(dtype)
    env = env or environments(cores, n, dtype)
    h, L = tree_shape(n)
    wl = np.asarray(w, dtype=np.float64).astype(dtype)
    x, y = up_down(cores, n, bits, dtype)
    xa, ya = up_down(cores, n, bits, dtype, absolute=True)
    psi, pa = x[1][:, 0], xa[1][:, 0]
    ok = psi != 0
    safe = np.where(ok, psi, 1)
    coef = np.where(ok, 2 * wl / safe, 0)
    coefa = np.where(ok, 2 * np.abs(wl) / np.abs(safe), 0)
    W, Wa = wl.sum(), np.abs(wl).sum()
    D = np.asarray(cores).shape[1]
    live = live_mask(n, D)
    grad, grada = np.zeros(live.shape, dtype), np.zeros(live.shape, dtype)
    for v in range(1, L):
        grad[v - 1] = np.einsum('k,kp,ka,kb->pab', coef, y[v], x[2 * v], x[2 * v + 1]) - W * env["dZ"][v - 1] / env["Z"]
        grada[v - 1] = np.einsum('k,kp,ka,kb->pab', coefa, ya[v], xa[2 * v], xa[2 * v + 1]) + Wa * env["dZ_abs"][v - 1] / env["Z"]
    grad, grada = np.where(live, grad, 0), np.where(live, grada, 0)
    with np.errstate(divide="ignore"):
        logq = np.log(psi * psi) - np.log(env["Z"])
    return {"grad": grad, "grad_abs": grada, "logq": logq, "psi": psi, "psi_abs": pa,
            "kappa": np.where(ok, pa / np.abs(safe), np.inf)}


def exact_elbo_gradient(cores, n, logp, dtype=None):
    """The exact gradient of sum_z q(z) (log q(z) - log p(z)) over all 2^n states: the score identity."""
    bits = all_bits(n)
    lq = logq_of(cores, n, bits, dtype=dtype)["logq"]
    q = np.exp(lq)
    f = lq - np.asarray(logp, dtype=np.float64)
    return score_gradient(cores, n, bits, hp.to_f64(q * f), dtype=dtype)["grad"]


# ---------------------------------------------------------------------------------------------- derived error counts
# Units of EPS64, derived from the kernels' chains in the docstring of test_gpu_ttn_kernel.py; kept here so that the kernel and
# the trainer tests share one statement of them.  t: a node's height above the positions (bottom nodes 1, the root h); d: its
# depth below the root (the root 0).
def geometry(B):
    """(workgroups G, tiles of 64 samples per workgroup) of the sampler and the score kernel."""
    tiles = -(-B // LANES)
    G = min(tiles, MAX_WG)
    return G, -(-tiles // G)


def c_x(t, D):
    """x_v against its majorant: per node a D-term chain (M) and a D-term chain (M x_r), and both children's errors."""
    return float(2 * D * (2 ** t - 1))


def c_u(t, D):
    """U_v: per node two D-term chains (A, W) and a D^2-term one, and both children's errors."""
    return float((D * D + 2 * D) * (2 ** t - 1))


def c_v(d, h, D):
    """V_v at depth d: per step down a D-term chain (Y) over V and R = T U_sibling (a D-term chain and the sibling's c_u) and a D^2-term chain."""
    return float(sum(2 * D + D * D + c_u(h - k - 1, D) for k in range(d)))


def c_y(d, h, D):
    """y_v at depth d: per step down a D-term chain (N), a D-term chain with the sibling's x (c_x of its height)."""
    return float(sum(2 * D + c_x(h - k - 1, D) for k in range(d)))


def logq_bound(n, D, kappa_b, kappa_Z, logq, logZ):
    h, _ = tree_shape(n)
    lpsi2 = np.where(np.isfinite(logq), logq + logZ, 0.0)
    return 2 * c_x(h, D) * kappa_b + c_u(h, D) * kappa_Z + 8 * (np.abs(lpsi2) + abs(logZ) + 4)


def c_score(n, D, B, kappa_max, kappa_Z):
    h, _ = tree_shape(n)
    G, tiles = geometry(B)
    worst = 0.0
    for d in range(h):
        sample = c_x(h, D) * kappa_max + 2 + c_y(d, h, D) + 1 + 2 * c_x(h - d - 1, D) + 2 * LANES * tiles + G
        c_w = tiles + 6 + (-(-G // 256)) + 6 + 3
        envt = c_v(d, h, D) + D + 2 * D + 2 * c_u(h - d - 1, D) + 1 + c_u(h, D) * kappa_Z + 1 + c_w + 1
        worst = max(worst, sample, envt)
    return 1.0 + worst


# ---------------------------------------------------------------------------------------------- float64 torch restatement
def logq_torch(cores, n, bits):
    """log q(z_b) [B], differentiable in cores float64 [L - 1, D, D, D] (dead entries masked: their gradient is 0)."""
    h, L = tree_shape(n)
    D = cores.shape[1]
    A = cores * torch.as_tensor(live_mask(n, D))
    x = [None] * (2 * L)
    leaves = torch.as_tensor(hp.to_f64(_leaves(np.asarray(bits), n, L, D, np.float64)))
    U = [None] * (2 * L)
    for j in range(L):
        x[L + j] = leaves[j]
        U[L + j] = torch.diag(torch.tensor([1.0, 1.0 if j < n else 0.0] + [0.0] * (D - 2), dtype=torch.float64))
    for v in range(L - 1, 0, -1):
        x[v] = torch.einsum('pab,ka,kb->kp', A[v - 1], x[2 * v], x[2 * v + 1])
        U[v] = torch.einsum('pab,qcd,ac,bd->pq', A[v - 1], A[v - 1], U[2 * v], U[2 * v + 1])
    return torch.log(x[1][:, 0] ** 2) - torch.log(U[1][0, 0])


def autograd_score(cores, n, bits, w):
    A = torch.tensor(np.asarray(cores, dtype=np.float64), requires_grad=True)
    (logq_torch(A, n, bits) * torch.as_tensor(np.asarray(w, dtype=np.float64))).sum().backward()
    return A.grad.numpy()


def replay(cores0, n, weights, B, seed, epochs, lr, optimizer_type="adam", clip=10.0, margin=1e-8):
    """SampledTrainer.train with tree cores on the CPU in float64: lps_mirror.replay's loop (Adam, cosine schedule, clip) with
    this family's sampler and log q; `weights` (elbo_weights, ksd_weights, mmd_weights) is the objective."""
    cores = torch.nn.Parameter(torch.as_tensor(np.asarray(cores0), dtype=torch.float64).clone())
    opt = torch.optim.Adam([cores], lr=lr) if optimizer_type == "adam" else torch.optim.SGD([cores], lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr / 10)
    hist = {"loss": [], "grad_norm": [], "idx": [], "undecided": 0}
    for ep in range(epochs):
        opt.zero_grad()
        s = sample(cores.detach().numpy(), n, seed, ep, B, dtype=np.float64, margin=margin)
        hist["undecided"] += s["undecided"]
        lq = logq_torch(cores, n, s["bits"])
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
