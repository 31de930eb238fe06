"""NumPy mirror of the MMD objective with a Hamming-distance kernel (test infrastructure, not under test).

  kappa[d] = mean_c rho_c^d, rho_c = exp(-1 / (n l_c));   lam[j] = mean_c (1 + rho_c)^(n - j) (1 - rho_c)^j
  enumerated:  L = d^T K d,  w = 2 K d,  d = q - target  (dense K for n <= 10; the Walsh-Hadamard route in float64 or longdouble)
  sampled:     pair counts by a double loop, the row sums in ascending d with separately rounded multiply and add, U and w_b
  training:    the step q -> w -> parameter-shift gradient on oracle.circuit, and a float32-theta Adam loop as the trainers run it"""
import math

import numpy as np
import torch

from oracle import circuit as oc

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)


# ---- tables -----------------------------------------------------------------------------------------------------------------
def tables(n, scales, dtype=LD):
    """(kappa [n + 1], lam [n + 1]) in `dtype`, written out independently of hamming_kernel.py."""
    scales = [dtype(s) for s in np.atleast_1d(scales)]
    C = dtype(len(scales))
    rho = [np.exp(-dtype(1) / (dtype(n) * s)) for s in scales]
    kappa = np.array([sum(r ** d for r in rho) / C for d in range(n + 1)], dtype=dtype)
    lam = np.array([sum((1 + r) ** (n - j) * (1 - r) ** j for r in rho) / C for j in range(n + 1)], dtype=dtype)
    return kappa, lam


def popcounts(n):
    k = np.arange(1 << n, dtype=np.int64)
    pc = np.zeros(1 << n, dtype=np.int64)
    for b in range(n):
        pc += (k >> b) & 1
    return pc


def dense_K(n, kappa):
    """K[z, z'] = kappa[popcount(z xor z')], n <= 10."""
    assert n <= 10
    z = np.arange(1 << n, dtype=np.int64)
    x = z[:, None] ^ z[None, :]
    d = np.zeros_like(x)
    for b in range(n):
        d += (x >> b) & 1
    return np.asarray(kappa)[d]


def hadamard(n):
    H = np.array([[1.0]])
    for _ in range(n):
        H = np.kron(H, np.array([[1.0, 1.0], [1.0, -1.0]]))
    return H


def wht(v, dtype=np.float64):
    """Iterative Walsh-Hadamard transform (unnormalised) of a vector of 2^n entries, in `dtype`."""
    a = np.array(v, dtype=dtype).copy()
    N = a.size
    h = 1
    while h < N:
        a = a.reshape(-1, 2, h)
        x, y = a[:, 0, :].copy(), a[:, 1, :].copy()
        a[:, 0, :], a[:, 1, :] = x + y, x - y
        a = a.reshape(-1)
        h *= 2
    return a


def weights(q, target, lam, dtype=np.float64):
    """(L, w) by the Walsh-Hadamard route in `dtype`: L = 2^-n sum lam[pop k] dhat_k^2, w = 2^(1 - n) H (lam[pop] * dhat)."""
    q = np.asarray(q, dtype=dtype)
    d = q if target is None else q - np.asarray(target, dtype=dtype)
    n = int(q.size).bit_length() - 1
    lk = np.asarray(lam, dtype=dtype)[popcounts(n)]
    dh = wht(d, dtype)
    y = lk * dh
    L = (y * dh).sum() / dtype(2) ** n
    return L, wht(y, dtype) * (dtype(2) / dtype(2) ** n)


# ---- pairs -----------------------------------------------------------------------------------------------------------------
def pair_counts(za, zb, n, skip_same_index=False):
    """cnt [A, n + 1] int64 by a double loop over Python integers."""
    cnt = np.zeros((len(za), n + 1), dtype=np.int64)
    for a, x in enumerate(za):
        for j, y in enumerate(zb):
            if skip_same_index and j == a:
                continue
            cnt[a, bin(int(x) ^ int(y)).count("1")] += 1
    return cnt


def pair_counts_fast(za, zb, n, skip_same_index=False):
    """The same counts vectorised over the columns (for the larger shapes of the GPU tests)."""
    za, zb = np.asarray(za, dtype=np.uint64), np.asarray(zb, dtype=np.uint64)
    cnt = np.zeros((za.size, n + 1), dtype=np.int64)
    for a in range(za.size):
        x = za[a] ^ zb
        d = np.zeros(zb.size, dtype=np.int64)
        for b in range(n):
            d += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
        if skip_same_index:
            d = np.delete(d, a)
        cnt[a] = np.bincount(d, minlength=n + 1)
    return cnt


def rowsum(cnt, kappa):
    """r_a = sum_d kappa[d] * cnt[a, d] in ascending d, multiply and add rounded separately in float64."""
    kappa = np.asarray(kappa, dtype=np.float64)
    r = np.zeros(cnt.shape[0], dtype=np.float64)
    for d in range(cnt.shape[1]):
        r = r + kappa[d] * cnt[:, d].astype(np.float64)
    return r


def u_and_weights(rxx, rxy, Tyy, N, Txx=None, Txy=None, fsum=True):
    """(U, w_b) of mmd_objective.py from the row sums; the totals default to math.fsum of the rows."""
    rxx, rxy = np.asarray(rxx, dtype=np.float64), np.asarray(rxy, dtype=np.float64)
    B = rxx.size
    Txx = math.fsum(rxx) if Txx is None else Txx
    Txy = math.fsum(rxy) if Txy is None else Txy
    U = Txx / (B * (B - 1)) - 2.0 * Txy / (B * N) + Tyy / (N * N)
    m = (Txx - 2.0 * rxx) / ((B - 1) * (B - 2))
    c = (Txy - rxy) / ((B - 1) * N)
    w = (2.0 / B) * ((rxx / (B - 1) - m) - (rxy / N - c))
    return U, w


def sampled(z, y, n, kappa):
    """(U, w_b, rxx, rxy, Tyy) for samples z and data y (index lists)."""
    kappa = np.asarray(kappa, dtype=np.float64)
    rxx = rowsum(pair_counts_fast(z, z, n, True), kappa)
    rxy = rowsum(pair_counts_fast(z, y, n), kappa)
    Tyy = math.fsum(rowsum(pair_counts_fast(y, y, n), kappa))
    U, w = u_and_weights(rxx, rxy, Tyy, len(y))
    return U, w, rxx, rxy, Tyy


def u_double_loop(z, y, n, kappa):
    """U straight from its definition: three double loops over the kernel values."""
    k = lambda a, b: float(kappa[bin(int(a) ^ int(b)).count("1")])
    B, N = len(z), len(y)
    xx = math.fsum(k(z[i], z[j]) for i in range(B) for j in range(B) if i != j)
    xy = math.fsum(k(z[i], y[j]) for i in range(B) for j in range(N))
    yy = math.fsum(k(y[i], y[j]) for i in range(N) for j in range(N))
    return xx / (B * (B - 1)) - 2.0 * xy / (B * N) + yy / (N * N)


# ---- training ---------------------------------------------------------------------------------------------------------------
def loss_and_grad(ansatz, n, layers, theta, target, lam):
    """(loss, grad [P], q, w) at theta (float64): q, then w, then the parameter-shift gradient."""
    q = oc.probs(ansatz, n, layers, theta)
    L, w = weights(q, target, lam, np.float64)
    return float(L), oc.paramshift_vjp(ansatz, n, layers, theta, w), q, w


def train(ansatz, n, layers, target, lam, th0, lr, num_epochs, clip=10.0):
    """history {loss_mmd2, grad_norm, theta}: the loss of q BEFORE the epoch's update (float32 theta, torch's CPU Adam,
    CosineAnnealingLR to lr / 10, clip_grad_norm_), as the trainers record it."""
    theta = torch.nn.Parameter(torch.as_tensor(th0, dtype=torch.float32).clone())
    opt = torch.optim.Adam([theta], lr=lr, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=num_epochs, eta_min=lr / 10)
    h = {"loss_mmd2": [], "grad_norm": [], "theta": []}
    for _ in range(num_epochs):
        opt.zero_grad()
        loss, g, _, _ = loss_and_grad(ansatz, n, layers, theta.detach().to(torch.float64).numpy(), target, lam)
        theta.grad = torch.as_tensor(g, dtype=torch.float32)
        gn = torch.nn.utils.clip_grad_norm_([theta], clip)
        opt.step()
        sched.step()
        h["loss_mmd2"].append(loss)
        h["grad_norm"].append(float(gn))
        h["theta"].append(theta.detach().clone().numpy())
    return h
