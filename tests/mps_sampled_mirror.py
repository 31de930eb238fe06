"""Oracle of the sampled MPS Born machine (test infrastructure, plain NumPy / CPU torch, not under test).

  psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0,  q = psi^2 / Z;  cores [n, 2, D, D], tuple position 0 = MSB of the outcome index.

Everything but `replay` works in np.longdouble where hp_reference.HAVE_LONGDOUBLE holds (else float64) and without any
rescaling: the extended exponent range holds the unscaled environments of every shape the tests use.
  environments      E_k, L_k, Z and the same with |cores| (the absolute-value evaluation)
  uniforms          U[b, k-1] of kernels_mps_sample.hip: Philox4x32-10, counter (b, ceil(k/2) - 1, 0xffffffff, epoch), key = seed
  conditionals      p1[b, k-1] = m_1 / (m_0 + m_1) along each sample's own prefix, and log q
  sample            ancestral sampling with those uniforms
  score_gradient    sum_b w_b grad log q(z_b) by left and right vectors, and the same sums with every term's magnitude
  replay            float64 restatement of SampledELBOVariationalInference.train (torch autograd for the gradient)
"""
import numpy as np
import torch

import hp_reference as hp
import mps_mirror as mm
from shots_mirror import philox4x32_10

LD = np.longdouble if hp.HAVE_LONGDOUBLE else np.float64
DOMAIN = 0xFFFFFFFF


def bits_of_idx(idx, n):
    """[B, n] of 0/1 from int64 outcome indices (position 0 = most significant bit)."""
    idx = np.asarray(idx, dtype=np.int64)
    return ((idx[:, None] >> (n - 1 - np.arange(n, dtype=np.int64))[None, :]) & 1).astype(np.int64)


def idx_of_bits(bits):
    n = bits.shape[1]
    return (np.asarray(bits, dtype=np.int64) << (n - 1 - np.arange(n, dtype=np.int64))[None, :]).sum(axis=1)


def environments(cores, dtype=None):
    """dict E [n + 1, D, D], L [n + 1, D, D], Z, and E_abs, L_abs, Z_abs from |cores|."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    out = {}
    for tag, A in (("", cores.astype(dtype)), ("_abs", np.abs(cores).astype(dtype))):
        E = np.zeros((n + 1, D, D), dtype)
        L = np.zeros((n + 1, D, D), dtype)
        E[n, 0, 0] = 1
        L[0, 0, 0] = 1
        for k in range(n, 0, -1):
            E[k - 1] = sum(A[k - 1, s] @ E[k] @ A[k - 1, s].T for s in (0, 1))
        for k in range(1, n + 1):
            L[k] = sum(A[k - 1, s].T @ L[k - 1] @ A[k - 1, s] for s in (0, 1))
        out["E" + tag], out["L" + tag], out["Z" + tag] = E, L, E[0, 0, 0]
    return out


def uniforms(seed, epoch, b, n):
    """U [len(b), n]: column k - 1 is U_k of sample b."""
    b = np.asarray(b, dtype=np.uint64)
    U = np.empty((len(b), n), dtype=np.float64)
    for j in range((n + 1) // 2):
        w = philox4x32_10(b, j, DOMAIN, int(epoch) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        U[:, 2 * j] = (((w[1] << np.uint64(32)) | w[0]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        if 2 * j + 1 < n:
            U[:, 2 * j + 1] = (((w[3] << np.uint64(32)) | w[2]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return U


def conditionals(cores, bits, env=None, dtype=None):
    """dict p1 [B, n] (m_1 / (m_0 + m_1) at each site along the sample's own prefix), logq [B] = log psi^2 - log Z, psi and
    psi_abs [B]."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    env = env or environments(cores, dtype)
    A, Aa = cores.astype(dtype), np.abs(cores).astype(dtype)
    Bn = bits.shape[0]
    l = np.zeros((Bn, D), dtype)
    la = np.zeros((Bn, D), dtype)
    l[:, 0] = 1
    la[:, 0] = 1
    p1 = np.zeros((Bn, n), dtype)
    for k in range(1, n + 1):
        u = [l @ A[k - 1, s] for s in (0, 1)]
        ua = [la @ Aa[k - 1, s] for s in (0, 1)]
        m = [np.einsum('bc,cd,bd->b', u[s], env["E"][k], u[s]) for s in (0, 1)]
        p1[:, k - 1] = m[1] / (m[0] + m[1])
        z = bits[:, k - 1].astype(bool)
        l = np.where(z[:, None], u[1], u[0])
        la = np.where(z[:, None], ua[1], ua[0])
    psi, psia = l[:, 0], la[:, 0]
    with np.errstate(divide="ignore"):
        logq = np.log(psi * psi) - np.log(env["Z"])
    return {"p1": p1, "logq": logq, "psi": psi, "psi_abs": psia}


def sample(cores, seed, epoch, B, dtype=None, margin=2.0 ** -40):
    """Ancestral sampling with the kernel's uniforms: dict bits [B, n], idx [B], logq [B], undecided: the number of draws with
    U within `margin` of p1 or of the decision boundary m_0 / (m_0 + m_1) = 1 - p1 (z_k = 1 iff U >= 1 - p1)."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    env = environments(cores, dtype)
    A = cores.astype(dtype)
    U = uniforms(seed, epoch, np.arange(B), n)
    l = np.zeros((B, D), dtype)
    l[:, 0] = 1
    bits = np.zeros((B, n), np.int64)
    undecided = 0
    for k in range(1, n + 1):
        u = [l @ A[k - 1, s] for s in (0, 1)]
        m = [np.einsum('bc,cd,bd->b', u[s], env["E"][k], u[s]) for s in (0, 1)]
        p1 = m[1] / (m[0] + m[1])
        Uk = U[:, k - 1].astype(dtype)
        undecided += int(((np.abs(Uk - p1) <= margin) | (np.abs(Uk - (1 - p1)) <= margin)).sum())
        z = U[:, k - 1].astype(dtype) * (m[0] + m[1]) >= m[0]
        bits[:, k - 1] = z
        l = np.where(z[:, None], u[1], u[0])
    psi = l[:, 0]
    return {"bits": bits, "idx": idx_of_bits(bits), "logq": np.log(psi * psi) - np.log(env["Z"]), "undecided": undecided}


def score_gradient(cores, bits, w, env=None, dtype=None):
    """dict grad [n, 2, D, D] = sum_b w_b grad log q(z_b), grad_abs (every term's magnitude: |cores|, |w|, + for -, divided
    by the true |psi_b| and the true Z), logq, psi, psi_abs, kappa (psi_abs / |psi| per sample)."""
    dtype = dtype or LD
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    env = env or environments(cores, dtype)
    A, Aa = cores.astype(dtype), np.abs(cores).astype(dtype)
    wl = np.asarray(w, dtype=np.float64).astype(dtype)
    L, R = mm._left_right(A, bits, dtype)
    La, Ra = mm._left_right(Aa, bits, dtype)
    psi, psia = L[n][:, 0], La[n][:, 0]
    ok = psi != 0
    safe = np.where(ok, psi, 1)
    coef = np.where(ok, 2 * wl / safe, 0)
    coefa = np.where(ok, 2 * np.abs(wl) / np.abs(safe), 0)
    W, Wa = wl.sum(), np.abs(wl).sum()
    grad, grada = np.zeros(cores.shape, dtype), np.zeros(cores.shape, dtype)
    for k in range(1, n + 1):
        for s in (0, 1):
            rows = bits[:, k - 1] == s
            grad[k - 1, s] = (L[k - 1, rows] * coef[rows, None]).T @ R[k, rows] \
                - W * 2 * (env["L"][k - 1] @ A[k - 1, s] @ env["E"][k]) / env["Z"]
            grada[k - 1, s] = (La[k - 1, rows] * coefa[rows, None]).T @ Ra[k, rows] \
                + Wa * 2 * (env["L_abs"][k - 1] @ Aa[k - 1, s] @ env["E_abs"][k]) / env["Z"]
    with np.errstate(divide="ignore"):
        logq = np.log(psi * psi) - np.log(env["Z"])
    return {"grad": grad, "grad_abs": grada, "logq": logq, "psi": psi, "psi_abs": psia,
            "kappa": np.where(ok, psia / np.abs(safe), np.inf)}


# ---------------------------------------------------------------------------------------------- float64 torch restatement
def logq_torch(cores, bits):
    """log q(z_b) [B], differentiable in cores (float64 torch): psi by an einsum chain, Z by the right environments."""
    n, _, D, _ = cores.shape
    Bt = torch.as_tensor(bits, dtype=torch.int64)
    v = torch.zeros(Bt.shape[0], D, dtype=torch.float64)
    v[:, 0] = 1.0
    for k in range(n):
        v = torch.einsum('za,zab->zb', v, cores[k][Bt[:, k]])
    E = torch.zeros(D, D, dtype=torch.float64)
    E[0, 0] = 1.0
    for k in range(n - 1, -1, -1):
        E = cores[k, 0] @ E @ cores[k, 0].T + cores[k, 1] @ E @ cores[k, 1].T
    return torch.log(v[:, 0] ** 2) - torch.log(E[0, 0])


def autograd_score(cores, bits, w):
    A = torch.tensor(np.asarray(cores, dtype=np.float64), requires_grad=True)
    (logq_torch(A, bits) * torch.as_tensor(np.asarray(w, dtype=np.float64))).sum().backward()
    return A.grad.numpy()


def log_joint(packed, bits, p_floor=1e-30):
    """logp [B] float64: sum over the nodes, in descriptor order, of log max(CPT factor, p_floor)."""
    role, npar, par, off, cpt = (packed[k] for k in ("role", "n_parents", "parents", "cpt_off", "cpt"))
    V = len(role)
    Bn = bits.shape[0]
    vals = np.zeros((Bn, V), np.int64)
    for v in range(V):
        if role[v] >= 0:
            vals[:, v] = bits[:, role[v]]
        elif role[v] == -2:
            vals[:, v] = 1
        elif role[v] != -1:
            raise ValueError("summed-out node")
    out = np.zeros(Bn, np.float64)
    for v in range(V):
        cfg = np.zeros(Bn, np.int64)
        for p in range(npar[v]):
            cfg = cfg * 2 + vals[:, par[v, p]]
        out += np.log(np.maximum(cpt[off[v] + 2 * cfg + vals[:, v]], p_floor))
    return out


def replay(cores0, packed, B, seed, epochs, lr, optimizer_type="adam", clip=10.0, p_floor=1e-30, margin=1e-8):
    """SampledELBOVariationalInference.train on the CPU in float64: dict loss, grad_norm per epoch, idx of every epoch, the
    final cores and `undecided`, the number of draws within `margin` of p1 or of the decision boundary, over the whole run."""
    cores = torch.nn.Parameter(torch.as_tensor(np.asarray(cores0), dtype=torch.float64).clone())
    n = cores.shape[0]
    opt = torch.optim.Adam([cores], lr=lr) if optimizer_type == "adam" else torch.optim.SGD([cores], lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr / 10)
    hist = {"loss": [], "grad_norm": [], "idx": [], "undecided": 0}
    for ep in range(epochs):
        opt.zero_grad()
        s = sample(cores.detach().numpy(), seed, ep, B, dtype=np.float64, margin=margin)
        hist["undecided"] += s["undecided"]
        lq = logq_torch(cores, s["bits"])
        f = lq.detach() - torch.as_tensor(log_joint(packed, s["bits"], p_floor))
        loss = f.mean()
        w = (f - loss) / (B - 1) if B > 1 else f.clone()
        (lq * w).sum().backward()
        gn = torch.nn.utils.clip_grad_norm_([cores], clip)
        opt.step()
        sched.step()
        hist["loss"].append(float(loss))
        hist["grad_norm"].append(float(gn))
        hist["idx"].append(s["idx"])
    hist["cores"] = cores.detach().numpy().copy()
    return hist
