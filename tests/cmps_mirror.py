"""Oracle of the sampled MPS Born machine with complex cores (test infrastructure, plain NumPy / CPU torch, not under test).

Conventions (kernels_cmps.hip states the same):
  cores is float64 [n, 2, D, D, 2] with (re, im) last: torch.view_as_real of a complex128 [n, 2, D, D].  A_k[s] = X + iY.
  psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0 in C: a plain product, no conjugate.  q(z) = |psi(z)|^2 / Z,  Z = sum_z |psi(z)|^2.
  Bit order, index word and boundary vectors as in the real family: tuple position 0 = MSB of the outcome index.
  Environments, Hermitian and positive semi-definite:  E_n = e0 e0^T,  E_{k-1} = sum_s A_k[s] E_k A_k[s]^H;  L_0 = e0 e0^T,
  L_k = sum_s A_k[s]^T L_{k-1} conj(A_k[s]);  Z = Re E_0[0, 0].
  Gradient: that of the real function sum_b w_b log q(z_b) in the 2 . 2 n D^2 real numbers.  With T_b = l_{b,k-1}[a] r_{b,k+1}[c] / psi_b
  at block [k, z_{b,k}]: d/dX = 2 w_b Re T_b, d/dY = -2 w_b Im T_b;  with G_k[s] = L_{k-1} conj(A_k[s]) E_k^T / Z:
  d log Z / dX = 2 Re G, d log Z / dY = -2 Im G, subtracted (sum_b w_b) times.

Everything but `replay` works in np.clongdouble where hp_reference.HAVE_LONGDOUBLE holds (else complex128), or in the dtype
given (np.float64: the float64 evaluation hp.measured_constant wants), and without any rescaling.
The absolute-value majorants use M_k[s] = |X| + |Y| entrywise in the REAL recursions: every real product of a complex chain,
of either part, is bounded term by term by the same chain over M.
  environments, uniforms (mps_sampled_mirror's), conditionals, sample, score_gradient, exact_elbo_gradient, replay,
  and the derived error counts c_env, logq_bound, c_score of the GPU tests
"""
import numpy as np
import torch

import hp_reference as hp
import mps_mirror as mm
import mps_sampled_mirror as sm
from mps_sampled_mirror import bits_of_idx, idx_of_bits, log_joint, uniforms  # noqa: F401

LD = sm.LD
CLD = np.clongdouble if hp.HAVE_LONGDOUBLE else np.complex128


def _types(dtype):
    """(real dtype, complex dtype) of a real dtype, default the extended one."""
    if dtype is None or dtype == LD:
        return LD, CLD
    return np.float64, np.complex128


def as_complex(cores, dtype=None):
    """complex [n, 2, D, D] of float64 [n, 2, D, D, 2]."""
    _, C = _types(dtype)
    cores = np.asarray(cores, dtype=np.float64)
    assert cores.ndim == 5 and cores.shape[-1] == 2
    out = np.empty(cores.shape[:-1], C)
    out.real = cores[..., 0]
    out.imag = cores[..., 1]
    return out


def majorant(cores, dtype=None):
    R, _ = _types(dtype)
    cores = np.asarray(cores, dtype=np.float64)
    return (np.abs(cores[..., 0]).astype(R) + np.abs(cores[..., 1]).astype(R))


def environments(cores, dtype=None):
    """dict E, L complex [n + 1, D, D], Z (real), and E_abs, L_abs, Z_abs (real) from the majorant."""
    R, C = _types(dtype)
    A, M = as_complex(cores, dtype), majorant(cores, dtype)
    n, _, D, _ = A.shape
    E, L = np.zeros((n + 1, D, D), C), np.zeros((n + 1, D, D), C)
    Ea, La = np.zeros((n + 1, D, D), R), np.zeros((n + 1, D, D), R)
    E[n, 0, 0] = L[0, 0, 0] = 1
    Ea[n, 0, 0] = La[0, 0, 0] = 1
    for k in range(n, 0, -1):
        E[k - 1] = sum(A[k - 1, s] @ E[k] @ A[k - 1, s].conj().T for s in (0, 1))
        Ea[k - 1] = sum(M[k - 1, s] @ Ea[k] @ M[k - 1, s].T for s in (0, 1))
    for k in range(1, n + 1):
        L[k] = sum(A[k - 1, s].T @ L[k - 1] @ A[k - 1, s].conj() for s in (0, 1))
        La[k] = sum(M[k - 1, s].T @ La[k - 1] @ M[k - 1, s] for s in (0, 1))
    return {"E": E, "L": L, "Z": E[0, 0, 0].real, "E_abs": Ea, "L_abs": La, "Z_abs": Ea[0, 0, 0]}


def _masses(u, Ek):
    """m = Re(u E u^H) per row of u."""
    return np.einsum('bc,cd,bd->b', u, Ek, u.conj()).real


def conditionals(cores, bits, env=None, dtype=None):
    """dict p1 [B, n] (m_1 / (m_0 + m_1) at each site along the sample's own prefix), logq [B] = log|psi|^2 - log Z, psi
    (complex) and psi_abs [B] (the majorant's)."""
    R, C = _types(dtype)
    A, M = as_complex(cores, dtype), majorant(cores, dtype)
    n, _, D, _ = A.shape
    env = env or environments(cores, dtype)
    Bn = bits.shape[0]
    l, la = np.zeros((Bn, D), C), np.zeros((Bn, D), R)
    l[:, 0] = 1
    la[:, 0] = 1
    p1 = np.zeros((Bn, n), R)
    for k in range(1, n + 1):
        u = [l @ A[k - 1, s] for s in (0, 1)]
        ua = [la @ M[k - 1, s] for s in (0, 1)]
        m = [_masses(u[s], env["E"][k]) for s in (0, 1)]
        p1[:, k - 1] = m[1] / (m[0] + m[1])
        z = bits[:, k - 1].astype(bool)
        l = np.where(z[:, None], u[1], u[0])
        la = np.where(z[:, None], ua[1], ua[0])
    psi, psia = l[:, 0], la[:, 0]
    with np.errstate(divide="ignore"):
        logq = np.log(psi.real * psi.real + psi.imag * psi.imag) - np.log(env["Z"])
    return {"p1": p1, "logq": logq, "psi": psi, "psi_abs": psia}


def sample(cores, seed, epoch, B, dtype=None, margin=2.0 ** -40):
    """Ancestral sampling with the kernel's uniforms: dict bits [B, n], idx [B], logq [B], undecided (as
    mps_sampled_mirror.sample counts them)."""
    R, C = _types(dtype)
    A = as_complex(cores, dtype)
    n, _, D, _ = A.shape
    env = environments(cores, dtype)
    U = uniforms(seed, epoch, np.arange(B), n)
    l = np.zeros((B, D), C)
    l[:, 0] = 1
    bits = np.zeros((B, n), np.int64)
    undecided = 0
    for k in range(1, n + 1):
        u = [l @ A[k - 1, s] for s in (0, 1)]
        m = [_masses(u[s], env["E"][k]) for s in (0, 1)]
        p1 = m[1] / (m[0] + m[1])
        Uk = U[:, k - 1].astype(R)
        undecided += int(((np.abs(Uk - p1) <= margin) | (np.abs(Uk - (1 - p1)) <= margin)).sum())
        z = Uk * (m[0] + m[1]) >= m[0]
        bits[:, k - 1] = z
        l = np.where(z[:, None], u[1], u[0])
    psi = l[:, 0]
    return {"bits": bits, "idx": idx_of_bits(bits), "logq": np.log(psi.real ** 2 + psi.imag ** 2) - np.log(env["Z"]),
            "undecided": undecided}


def score_gradient(cores, bits, w, env=None, dtype=None):
    """dict grad [n, 2, D, D, 2] = the gradient of sum_b w_b log q(z_b) in (re, im) of the cores, grad_abs [n, 2, D, D, 2]
    (every term's magnitude through the majorant, |w|, + for -, divided by the true |psi_b| and the true Z; the same for both
    parts), logq, psi, psi_abs, kappa (psi_abs / |psi| per sample)."""
    R, C = _types(dtype)
    A, M = as_complex(cores, dtype), majorant(cores, dtype)
    n, _, D, _ = A.shape
    env = env or environments(cores, dtype)
    wl = np.asarray(w, dtype=np.float64).astype(R)
    L, Rv = mm._left_right(A, bits, C)
    La, Ra = mm._left_right(M, bits, R)
    psi, psia = L[n][:, 0], La[n][:, 0]
    mag = np.abs(psi)
    ok = mag != 0
    safe = np.where(ok, psi, 1)
    coef = np.where(ok, 2 * wl / safe, 0)                   # complex: 2 w / psi
    coefa = np.where(ok, 2 * np.abs(wl) / np.abs(safe), 0)
    W, Wa = wl.sum(), np.abs(wl).sum()
    grad, grada = np.zeros(A.shape + (2,), R), np.zeros(A.shape + (2,), R)
    for k in range(1, n + 1):
        for s in (0, 1):
            rows = bits[:, k - 1] == s
            T = (L[k - 1, rows] * coef[rows, None]).T @ Rv[k, rows]                     # sum_b 2 w_b l[a] r[c] / psi_b
            G = env["L"][k - 1] @ A[k - 1, s].conj() @ env["E"][k].T / env["Z"]
            grad[k - 1, s, :, :, 0] = T.real - W * 2 * G.real
            grad[k - 1, s, :, :, 1] = -T.imag + W * 2 * G.imag
            Ta = (La[k - 1, rows] * coefa[rows, None]).T @ Ra[k, rows] \
                + Wa * 2 * (env["L_abs"][k - 1] @ M[k - 1, s] @ env["E_abs"][k].T) / env["Z"]
            grada[k - 1, s, :, :, 0] = Ta
            grada[k - 1, s, :, :, 1] = Ta
    with np.errstate(divide="ignore"):
        logq = np.log(psi.real ** 2 + psi.imag ** 2) - np.log(env["Z"])
    return {"grad": grad, "grad_abs": grada, "logq": logq, "psi": psi, "psi_abs": psia,
            "kappa": np.where(ok, psia / np.where(ok, mag, 1), np.inf)}


def all_bits(n):
    return bits_of_idx(np.arange(1 << n, dtype=np.int64), n)


def exact_elbo_gradient(cores, logp, dtype=None):
    """The exact gradient of sum_z q(z) (log q(z) - log p(z)) over all 2^n states, [n, 2, D, D, 2]: the score identity,
    sum_z q(z) (log q(z) - log p(z)) grad log q(z) (the mean of grad log q under q is 0)."""
    n = np.asarray(cores).shape[0]
    bits = all_bits(n)
    c = conditionals(cores, bits, dtype=dtype)
    q = np.exp(c["logq"])
    f = c["logq"] - np.asarray(logp, dtype=np.float64)
    return score_gradient(cores, bits, hp.to_f64(q * f), dtype=dtype)["grad"]


# ---------------------------------------------------------------------------------------------- derived error counts
# Units of EPS64, derived from the kernels' chains in the docstring of test_gpu_cmps_kernel.py (a complex D-term chain is two
# real 2 D-term chains); kept here so that the kernel and the trainer tests share one statement of them.
LANES, MAX_WG = 64, 256


def c_env(j, D):
    """E_k, L_k after j steps against the majorant environment."""
    return float(j * (6 * D + 1))


def geometry(B):
    """(workgroups G, tiles per workgroup) of the score kernel."""
    tiles = -(-B // LANES)
    G = min(tiles, MAX_WG)
    return G, -(-tiles // G)


def logq_bound(n, D, kappa_b, kappa_Z, logq, logZ):
    lpsi2 = np.where(np.isfinite(logq), logq + logZ, 0.0)
    return 2 * (2 * n * D + 2) * kappa_b + c_env(n, D) * kappa_Z + 8 * (np.abs(lpsi2) + abs(logZ) + 4) + 2


def c_score(n, D, B, kappa_max, kappa_Z):
    G, tiles = geometry(B)
    sample = 2 * (n - 1) * D + (2 * n * D + 2) * kappa_max + 8 + 128 + tiles + G
    envt = c_env(n - 1, D) + 4 * D + c_env(n, D) * kappa_Z + 6 + tiles + (-(-G // 256)) + 9 + 4
    return 1.0 + max(sample, envt)


# ---------------------------------------------------------------------------------------------- float64 torch restatement
def logq_torch(cores, bits):
    """log q(z_b) [B], differentiable in cores float64 [n, 2, D, D, 2] (torch complex128 autograd on the real view)."""
    A = torch.view_as_complex(cores)
    n, _, D, _ = A.shape
    Bt = torch.as_tensor(bits, dtype=torch.int64)
    v = torch.zeros(Bt.shape[0], D, dtype=torch.complex128)
    v[:, 0] = 1.0
    for k in range(n):
        v = torch.einsum('za,zab->zb', v, A[k][Bt[:, k]])
    E = torch.zeros(D, D, dtype=torch.complex128)
    E[0, 0] = 1.0
    for k in range(n - 1, -1, -1):
        E = A[k, 0] @ E @ A[k, 0].conj().T + A[k, 1] @ E @ A[k, 1].conj().T
    return torch.log(v[:, 0].real ** 2 + v[:, 0].imag ** 2) - torch.log(E[0, 0].real)


def autograd_score(cores, bits, w):
    A = torch.tensor(np.asarray(cores, dtype=np.float64), requires_grad=True)
    (logq_torch(A, bits) * torch.as_tensor(np.asarray(w, dtype=np.float64))).sum().backward()
    return A.grad.numpy()


def replay(cores0, packed, B, seed, epochs, lr, optimizer_type="adam", clip=10.0, p_floor=1e-30, margin=1e-8):
    """SampledELBOVariationalInference.train with complex cores on the CPU in float64: mps_sampled_mirror.replay's loop
    (Adam, cosine schedule, clip) with this family's sampler and log q."""
    cores = torch.nn.Parameter(torch.as_tensor(np.asarray(cores0), dtype=torch.float64).clone())
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
