"""Oracle of the matrix-product-state Born machine (test infrastructure, plain NumPy / CPU torch, not under test).

  psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0,  Z = sum psi^2,  q = psi^2 / Z;  cores [n, 2, D, D], tuple position 0 = MSB of z.

`reference` deliberately does NOT use prefix doubling: for every z it multiplies that z's own n matrices left to right (the
z's are batched, nothing is shared between two of them), in np.longdouble where hp_reference.HAVE_LONGDOUBLE holds, else
float64.  The gradient there is the sum over z of the outer products of z's own left and right vectors.  Beside every value
it returns the absolute-value evaluation in the manner of hp_reference: the same formula with every operand replaced by its
absolute value and every subtraction by an addition (Z, a sum of squares, stays what it is: it is a denominator).
`autograd_gradient` is a second, independent gradient (float64 torch autograd through an einsum chain per z);
`doubling` is the float64 prefix-doubling form for the sizes the per-z form is too slow for; `replay` restates the trainers'
epochs on the CPU in float64.
"""
import numpy as np
import torch

import hp_reference as hp

LD = np.longdouble if hp.HAVE_LONGDOUBLE else np.float64


def bits_of(n):
    """[2^n, n] of 0/1: tuple position k of outcome z (position 0 = most significant bit)."""
    z = np.arange(1 << n, dtype=np.int64)
    return (z[:, None] >> (n - 1 - np.arange(n))[None, :]) & 1


def _left_right(A, bits, dtype):
    """L [n + 1, Z, D], R [n + 1, Z, D] of the outcomes `bits` [Z, n]: L_k = e0^T A_1[z_1] .. A_k[z_k], R_k = A_{k+1}[z_{k+1}] .. A_n[z_n] e0."""
    n, _, D, _ = A.shape
    Zc = bits.shape[0]
    L = np.zeros((n + 1, Zc, D), dtype)
    R = np.zeros((n + 1, Zc, D), dtype)
    L[0, :, 0] = 1
    R[n, :, 0] = 1
    for k in range(1, n + 1):
        for s in (0, 1):
            rows = bits[:, k - 1] == s
            L[k, rows] = L[k - 1, rows] @ A[k - 1, s]
    for k in range(n, 0, -1):
        for s in (0, 1):
            rows = bits[:, k - 1] == s
            R[k - 1, rows] = R[k, rows] @ A[k - 1, s].T
    return L, R


def reference(cores, g=None, chunk=2048):
    """dict: psi, psi_abs, Z, Z_abs (= sum psi_abs^2), q, q_abs (= psi_abs^2 / Z) and, with g, c, c_abs, grad, grad_abs
    ([n, 2, D, D]); all in LD."""
    cores = np.asarray(cores, dtype=np.float64)
    n, _, D, _ = cores.shape
    A, Aa = cores.astype(LD), np.abs(cores).astype(LD)
    B = bits_of(n)
    N = 1 << n
    psi, psia = np.zeros(N, LD), np.zeros(N, LD)
    kept = []                                     # with g: every chunk's left and right vectors, for the gradient pass
    for z0 in range(0, N, chunk):
        b = B[z0:z0 + chunk]
        LR, LRa = _left_right(A, b, LD), _left_right(Aa, b, LD)
        psi[z0:z0 + chunk] = LR[0][n][:, 0]
        psia[z0:z0 + chunk] = LRa[0][n][:, 0]
        if g is not None:
            kept.append((z0, b, LR, LRa))
    Z = (psi * psi).sum()
    out = {"psi": psi, "psi_abs": psia, "Z": Z, "Z_abs": (psia * psia).sum(), "q": psi * psi / Z, "q_abs": psia * psia / Z}
    if g is None:
        return out
    gl = np.asarray(g, dtype=np.float64).astype(LD)
    c = (out["q"] * gl).sum()
    ca = (out["q_abs"] * np.abs(gl)).sum()
    G = 2 * psi * (gl - c) / Z
    Ga = 2 * psia * (np.abs(gl) + ca) / Z
    grad, grada = np.zeros(cores.shape, LD), np.zeros(cores.shape, LD)
    for z0, b, (L, R), (La, Ra) in kept:
        for k in range(1, n + 1):
            for s in (0, 1):
                rows = b[:, k - 1] == s
                grad[k - 1, s] += (L[k - 1, rows] * G[z0:z0 + chunk][rows, None]).T @ R[k, rows]
                grada[k - 1, s] += (La[k - 1, rows] * Ga[z0:z0 + chunk][rows, None]).T @ Ra[k, rows]
    out.update(c=c, c_abs=ca, grad=grad, grad_abs=grada)
    return out


def autograd_gradient(cores, g):
    """d(sum_z q_z g_z)/d cores by torch autograd in float64 on the CPU, psi through an einsum chain per z."""
    A = torch.tensor(np.asarray(cores, dtype=np.float64), requires_grad=True)
    n, _, D, _ = A.shape
    B = torch.from_numpy(bits_of(n))
    v = torch.zeros(1 << n, D, dtype=torch.float64)
    v[:, 0] = 1.0
    for k in range(n):
        v = torch.einsum('za,zab->zb', v, A[k][B[:, k]])
    psi = v[:, 0]
    q = psi * psi / (psi * psi).sum()
    (q * torch.tensor(np.asarray(g, dtype=np.float64))).sum().backward()
    return A.grad.numpy()


def doubling(cores, g=None, Z_true=None):
    """The issue's prefix-doubling formulas in float64 (torch, CPU): dict psi, Z, q and, with g, grad.  Z_true given: the
    absolute-value evaluation instead (|cores|, |g|, + for -), divided by that true Z and not by the sum of psi_abs^2."""
    A = torch.as_tensor(np.asarray(cores, dtype=np.float64))
    n, _, D, _ = A.shape
    Ztrue = None
    if Z_true is not None:
        Ztrue = float(Z_true)
        A = A.abs()
    V = [torch.zeros(1, D, dtype=torch.float64)]
    V[0][0, 0] = 1.0
    for k in range(1, n + 1):
        V.append(torch.stack([V[-1] @ A[k - 1, 0], V[-1] @ A[k - 1, 1]], dim=1).reshape(-1, D))
    psi = V[n][:, 0].clone()
    Z = (psi * psi).sum() if Ztrue is None else torch.tensor(Ztrue, dtype=torch.float64)
    out = {"psi": psi.numpy(), "Z": float(Z), "q": (psi * psi / Z).numpy()}
    if g is None:
        return out
    gt = torch.as_tensor(np.asarray(g, dtype=np.float64))
    if Ztrue is None:
        c = (psi * psi / Z * gt).sum()
        top = 2 * psi * (gt - c) / Z
    else:
        c = (psi * psi / Z * gt.abs()).sum()
        top = 2 * psi * (gt.abs() + c) / Z
    G = torch.zeros(1 << n, D, dtype=torch.float64)
    G[:, 0] = top
    grad = torch.zeros_like(A)
    for k in range(n, 0, -1):
        G2 = G.reshape(-1, 2, D)
        for s in (0, 1):
            grad[k - 1, s] = V[k - 1].T @ G2[:, s, :]
        G = G2[:, 0, :] @ A[k - 1, 0].T + G2[:, 1, :] @ A[k - 1, 1].T
    out["grad"] = grad.numpy()
    out["c"] = float(c)
    return out


def init_cores(n, D, method='small_random'):
    """The module's initialisation (born_machine_mps.py), drawn from torch's CPU generator."""
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    if method == 'zero':
        return (eye / np.sqrt(2.0)).clone()
    if method == 'small_random':
        return (eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / np.sqrt(2.0)
    return torch.randn(n, 2, D, D, dtype=torch.float64) / np.sqrt(2.0 * D)


# ---------------------------------------------------------------------------------------------- trainer replay (float64, CPU)
def _q_of(cores):
    n, _, D, _ = cores.shape
    B = torch.from_numpy(bits_of(n))
    v = torch.zeros(1 << n, D, dtype=torch.float64)
    v[:, 0] = 1.0
    for k in range(n):
        v = torch.einsum('za,zab->zb', v, cores[k][B[:, k]])
    psi = v[:, 0]
    return psi * psi / (psi * psi).sum()


def replay(cores0, objective, epochs, lr, optimizer_type="adam", entropy_weight=0.0, clip=10.0, K=None, log_p=None):
    """The classical trainers' epochs (ksd_vi.py train(): clip_grad_norm_, Adam or SGD with momentum 0.9, cosine schedule to
    lr / 10) on float64 CPU tensors through torch autograd.  objective 'elbo': L = sum q (log max(q, 1e-10) - log_p);
    'ksd': L = sqrt(max(q^T K q, 1e-12)); the gradient is that of L - entropy_weight * H.  -> dict of per-epoch loss,
    entropy, grad_norm and the final cores."""
    cores = torch.nn.Parameter(torch.as_tensor(np.asarray(cores0), dtype=torch.float64).clone())
    opt = torch.optim.Adam([cores], lr=lr) if optimizer_type == "adam" else torch.optim.SGD([cores], lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr / 10)
    hist = {"loss": [], "entropy": [], "grad_norm": []}
    for _ in range(epochs):
        opt.zero_grad()
        q = _q_of(cores)
        logq = torch.log(q.clamp(min=1e-10))
        H = -(q * logq).sum()
        if objective == "elbo":
            loss = (q * (logq - log_p)).sum()
        else:
            loss = torch.sqrt((q @ (K @ q)).clamp(min=1e-12))
        (loss - entropy_weight * H).backward()
        gn = torch.nn.utils.clip_grad_norm_([cores], clip)
        opt.step()
        sched.step()
        hist["loss"].append(float(loss.detach()))
        hist["entropy"].append(float(H.detach()))
        hist["grad_norm"].append(float(gn))
    hist["cores"] = cores.detach().numpy().copy()
    return hist
