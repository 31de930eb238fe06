"""Oracle of amortised inference with the sampled MPS (test infrastructure, plain NumPy / float64 torch, not under test).

Conventions of mps_sampled_mirror and mps_query_mirror: np.longdouble where hp_reference.HAVE_LONGDOUBLE holds, no rescaling,
tuple position 0 = the most significant bit of an outcome index, an evidence is a dict {position: 0 or 1}.
  bn_uniforms, bn_sample   the network's ancestral sampler with the kernel's uniforms and its decision in float64
  clamped_left             L^(j)_k, the left environments under an evidence, and the same from |cores|
  log_marginal_gradient    sum_j c_j grad log q(evidence_j) with every term's magnitude and the per-entry bound of the kernel
  logm_torch               log q(evidence) by a dense float64 evaluation over all 2^n states, differentiable
  logm_env_torch           the same through clamped environments (any n), differentiable: what replay trains on
  site_joint, forward_kl   p over the sites by enumeration; KL(p || q)
  replay                   AmortisedMPSInference.train on the CPU in float64
"""
import itertools

import numpy as np
import torch

import mps_query_mirror as qm
import mps_sampled_mirror as sm
from shots_mirror import philox4x32_10

LD = sm.LD
BN_DOMAIN = 0xFFFFFFFE
MAX_WG = 256                    # kernels_mps_query.hip: MQ_VJP_MAX_WG


def bn_uniforms(seed, epoch, b, V):
    """U [len(b), V]: column v is the uniform of node v of sample b."""
    b = np.asarray(b, dtype=np.uint64)
    U = np.empty((len(b), V), dtype=np.float64)
    for j in range((V + 1) // 2):
        w = philox4x32_10(b, j, BN_DOMAIN, int(epoch) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        U[:, 2 * j] = (((w[1] << np.uint64(32)) | w[0]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        if 2 * j + 1 < V:
            U[:, 2 * j + 1] = (((w[3] << np.uint64(32)) | w[2]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return U


def bn_sample(packed, n, seed, epoch, B):
    """dict vals [B, V] (every node), bits [B, n] (the kept nodes by tuple position), idx [B] uint64, logp [B] long double
    (NaN for a dead sample), logp_abs [B] (the sum of |log factor|), dead [B].  The decision U (t0 + t1) >= t0 is taken in
    float64, as the kernel takes it: one add, one multiply, one compare."""
    role, npar, par, off, cpt = (packed[k] for k in ("role", "n_parents", "parents", "cpt_off", "cpt"))
    V = len(role)
    U = bn_uniforms(seed, epoch, np.arange(B), V)
    vals = np.zeros((B, V), np.int64)
    dead = np.zeros(B, bool)
    logp = np.zeros(B, LD)
    logp_abs = np.zeros(B, LD)
    for v in range(V):
        cfg = np.zeros(B, np.int64)
        for p in range(npar[v]):
            cfg = cfg * 2 + vals[:, par[v, p]]
        t0, t1 = cpt[off[v] + 2 * cfg], cpt[off[v] + 2 * cfg + 1]
        tot = t0 + t1
        dead |= ~((tot > 0) & np.isfinite(tot))
        bit = ~dead & (U[:, v] * tot >= t0)
        vals[:, v] = bit
        with np.errstate(divide="ignore", invalid="ignore"):
            lf = np.log(np.where(bit, t1, t0).astype(LD))
        logp += lf
        logp_abs += np.abs(lf)
    bits = np.zeros((B, n), np.int64)
    for v in range(V):
        if role[v] >= 0:
            bits[:, role[v]] = vals[:, v]
    idx = np.zeros(B, np.uint64)
    for p in range(n):
        idx |= bits[:, p].astype(np.uint64) << np.uint64(n - 1 - p)
    logp = np.where(dead, np.nan, logp)
    return {"vals": vals, "bits": bits, "idx": idx, "logp": logp, "logp_abs": logp_abs, "dead": dead}


def clamped_left(cores, ev, dtype=None):
    """dict L [n + 1, D, D] (L_0 = e0 e0^T, L_k = sum_{s allowed at k} A_k[s]^T L_{k-1} A_k[s]) and L_abs from |cores|."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    out = {}
    for tag, A in (("", cores.astype(dtype)), ("_abs", np.abs(cores).astype(dtype))):
        L = np.zeros((n + 1, D, D), dtype)
        L[0, 0, 0] = 1
        for k in range(1, n + 1):
            allowed = (ev[k - 1],) if (k - 1) in ev else (0, 1)
            L[k] = sum(A[k - 1, s].T @ L[k - 1] @ A[k - 1, s] for s in allowed)
        out["L" + tag] = L
    return out


def _term(cores, ev, dtype):
    """(2 L A_s E / m, the same from |cores| over the true m, m, kappa = m_abs / m) of one evidence; None where m is 0."""
    cores = np.asarray(cores, dtype=np.float64)
    n = cores.shape[0]
    c = qm.clamped_environments(cores, ev, dtype)
    if not c["Z"] > 0:
        return None
    l = clamped_left(cores, ev, dtype)
    A, Aa = cores.astype(dtype), np.abs(cores).astype(dtype)
    t, ta = np.zeros(cores.shape, dtype), np.zeros(cores.shape, dtype)
    for k in range(1, n + 1):
        for s in ((ev[k - 1],) if (k - 1) in ev else (0, 1)):
            t[k - 1, s] = 2 * (l["L"][k - 1] @ A[k - 1, s] @ c["E"][k]) / c["Z"]
            ta[k - 1, s] = 2 * (l["L_abs"][k - 1] @ Aa[k - 1, s] @ c["E_abs"][k]) / c["Z"]
    return t, ta, c["Z"], c["Z_abs"] / c["Z"]


def groups(Q):
    return min(Q, MAX_WG)


def log_marginal_gradient(cores, evs, c, dtype=None):
    """dict grad [n, 2, D, D] = sum_j c_j grad log q(evs[j]) (an evidence of mass 0 contributes nothing), grad_abs (every
    term's magnitude), bound: the kernel's per-entry error bound in units of EPS64:
      sum_j |c_j| t_abs_j (C_ENV(n - 1) + 2 D + 3 + C_ENV(n) kappa_j + Q / G + G + 1)
      + W_abs t_abs_Z (C_ENV(n - 1) + 2 D + 3 + C_ENV(n) kappa_Z + Q / G + 14),
    logm [Q] (-inf where impossible), kappa [Q]."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    cl = np.asarray(c, dtype=np.float64).astype(dtype)
    Q = len(evs)
    G = groups(Q)
    per = -(-Q // G)
    c_env = lambda j: j * (3 * D + 1)
    base = c_env(n - 1) + 2 * D + 3
    tZ, tZa, Z, kZ = _term(cores, {}, dtype)
    grad, grada, bound = (np.zeros(cores.shape, dtype) for _ in range(3))
    W, Wa = dtype(0), dtype(0)
    logm = np.full(Q, -np.inf, dtype)
    kappa = np.full(Q, np.inf)
    cache = {}
    for j, ev in enumerate(evs):
        key = tuple(sorted(ev.items()))
        if key not in cache:
            cache[key] = _term(cores, ev, dtype)
        r = cache[key]
        if r is None:
            continue
        t, ta, m, k = r
        logm[j] = np.log(m) - np.log(Z)
        kappa[j] = float(k)
        grad += cl[j] * t
        grada += np.abs(cl[j]) * ta
        bound += np.abs(cl[j]) * ta * (base + c_env(n) * k + per + G + 1)
        W += cl[j]
        Wa += np.abs(cl[j])
    grad -= W * tZ
    grada += Wa * tZa
    bound += Wa * tZa * (base + c_env(n) * kZ + per + 14)
    return {"grad": grad, "grad_abs": grada, "bound": bound, "logm": logm, "kappa": kappa, "kappa_Z": float(kZ)}


# ---------------------------------------------------------------------------------------------- float64 torch restatements
def logm_torch(cores, ev):
    """log q(evidence) by a dense evaluation: psi over all 2^n states, the consistent ones summed (small n)."""
    n, _, D, _ = cores.shape
    bits = sm.bits_of_idx(np.arange(1 << n), n)
    Bt = torch.as_tensor(bits, dtype=torch.int64)
    v = torch.zeros(1 << n, D, dtype=torch.float64)
    v[:, 0] = 1.0
    for k in range(n):
        v = torch.einsum('za,zab->zb', v, cores[k][Bt[:, k]])
    psi2 = v[:, 0] ** 2
    ok = torch.as_tensor(qm.consistent(bits, ev))
    return torch.log(psi2[ok].sum()) - torch.log(psi2.sum())


def autograd_logm(cores, evs, c):
    A = torch.tensor(np.asarray(cores, dtype=np.float64), requires_grad=True)
    sum(float(cj) * logm_torch(A, ev) for ev, cj in zip(evs, c)).backward()
    return A.grad.numpy()


def logm_env_torch(cores, mask_bits, value_bits):
    """log q(evidence_b) [B] through batched clamped environments: mask_bits, value_bits [B, n] of 0 / 1."""
    n, _, D, _ = cores.shape
    M = torch.as_tensor(mask_bits, dtype=torch.float64)
    Vb = torch.as_tensor(value_bits, dtype=torch.float64)
    Bn = M.shape[0]
    E = torch.zeros(Bn, D, D, dtype=torch.float64)
    E[:, 0, 0] = 1.0
    F = torch.zeros(D, D, dtype=torch.float64)
    F[0, 0] = 1.0
    for k in range(n - 1, -1, -1):
        t = [torch.einsum('ab,zbc,dc->zad', cores[k, s], E, cores[k, s]) for s in (0, 1)]
        a0 = (1 - M[:, k] * Vb[:, k])[:, None, None]               # s = 0 allowed unless clamped to 1
        a1 = (1 - M[:, k] * (1 - Vb[:, k]))[:, None, None]
        E = a0 * t[0] + a1 * t[1]
        F = cores[k, 0] @ F @ cores[k, 0].T + cores[k, 1] @ F @ cores[k, 1].T
    return torch.log(E[:, 0, 0]) - torch.log(F[0, 0])


def site_joint(bn, site_names):
    """p over the sites [2^n] float64, other nodes summed out, by enumeration of the whole network."""
    n = len(site_names)
    pos = {nm: site_names.index(nm) for nm in site_names}
    table = np.zeros(1 << n)
    for assignment in itertools.product((0, 1), repeat=len(bn.nodes)):
        state = 0
        for nm, v in zip(bn.nodes, assignment):
            if nm in pos:
                state |= v << (n - 1 - pos[nm])
        table[state] += bn.get_joint_probability(assignment)
    return table


def probabilities(cores):
    return np.asarray(qm.brute(cores)["q"]).astype(np.float64)


def forward_kl(cores, p):
    q = probabilities(cores)
    m = p > 0
    return float((p[m] * (np.log(p[m]) - np.log(q[m]))).sum())


def epoch_loss(cores, bits, observed_positions, objective):
    """The epoch's loss as a float64 torch scalar, differentiable in cores."""
    lq = sm.logq_torch(cores, bits)
    loss = -lq.mean()
    if objective == "conditional":
        mask = np.zeros_like(bits)
        mask[:, observed_positions] = 1
        loss = loss + logm_env_torch(cores, mask, bits * mask).mean()
    return loss


def replay(cores0, packed, n, observed_positions, B, seed, epochs, lr, objective="joint", clip=10.0):
    """AmortisedMPSInference.train (Adam, cosine annealing) on the CPU in float64: dict loss, grad_norm per epoch and the
    final cores."""
    cores = torch.nn.Parameter(torch.as_tensor(np.asarray(cores0), dtype=torch.float64).clone())
    opt = torch.optim.Adam([cores], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr / 10)
    hist = {"loss": [], "grad_norm": []}
    for ep in range(epochs):
        opt.zero_grad()
        s = bn_sample(packed, n, seed, ep, B)
        loss = epoch_loss(cores, s["bits"], observed_positions, objective)
        loss.backward()
        gn = torch.nn.utils.clip_grad_norm_([cores], clip)
        opt.step()
        sched.step()
        hist["loss"].append(float(loss.detach()))
        hist["grad_norm"].append(float(gn))
    hist["cores"] = cores.detach().numpy().copy()
    return hist
