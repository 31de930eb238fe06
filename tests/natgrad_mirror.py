"""Float64 NumPy mirror of the natural-gradient pieces (test infrastructure, not under test).

  F_ab = sum_z d_a(z) d_b(z) r_z,  d_a = 1/2 (row_2a - row_2a+1),  r_z = 1 / q_z where q_z >= q_floor, else 0
  (A + damping I) x = b by a plain Cholesky with the library's status rule: info = P + 1 when b is not finite (tested
  first), k + 1 when pivot k (from 0) is not positive or not finite, P + 2 when the solution is not finite; then x = b.

The training run is elbo_mirror's epoch with the gradient replaced by delta = (F + damping I)^-1 g and plain SGD."""
import numpy as np
import torch

import elbo_mirror as em
from oracle import circuit as oc

Q_FLOOR = 1e-10
DAMPING = 1e-3


def shifted_rows(ansatz, n, layers, theta):
    """[2 P, 2^n]: rows (+p, -p), the layout of backend.paramshift_probs without its base row."""
    theta = np.asarray(theta, dtype=np.float64)
    rows = np.empty((2 * theta.size, 1 << n))
    for p in range(theta.size):
        for k, s in enumerate((np.pi / 2, -np.pi / 2)):
            t = theta.copy()
            t[p] += s
            rows[2 * p + k] = oc.probs(ansatz, n, layers, t)
    return rows


def fisher(shifted, q, q_floor=Q_FLOOR):
    shifted = np.asarray(shifted, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    d = 0.5 * (shifted[0::2] - shifted[1::2])
    keep = q >= q_floor
    r = np.zeros_like(q)
    r[keep] = 1.0 / q[keep]
    d = np.where(keep[None, :], d, 0.0)
    return (d * r[None, :]) @ d.T


def spd_solve(A, b, damping=0.0):
    """-> (x, info)."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    P = b.size
    if not np.isfinite(b).all():
        return b.copy(), P + 1
    W = np.triu(A) + np.triu(A, 1).T + damping * np.eye(P)       # the upper triangle is what is read
    L = np.zeros((P, P))
    with np.errstate(all="ignore"):
        for k in range(P):
            piv = W[k, k] - L[k, :k] @ L[k, :k]
            if not (piv > 0.0) or not np.isfinite(piv):
                return b.copy(), k + 1
            L[k, k] = np.sqrt(piv)
            L[k + 1:, k] = (W[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
        y = np.zeros(P)
        for k in range(P):
            y[k] = (b[k] - L[k, :k] @ y[:k]) / L[k, k]
        x = np.zeros(P)
        for k in range(P - 1, -1, -1):
            x[k] = (y[k] - L[k + 1:, k] @ x[k + 1:]) / L[k, k]
    if not np.isfinite(x).all():
        return b.copy(), P + 2
    return x, 0


def precondition(ansatz, n, layers, theta, q, grad, damping=DAMPING, q_floor=Q_FLOOR):
    F = fisher(shifted_rows(ansatz, n, layers, theta), q, q_floor)
    return spd_solve(F, grad, damping) + (F,)


def train(ansatz, n, layers, log_p, log_evidence, th0, lr, num_epochs, damping=DAMPING, natural=True, clip=10.0,
          posterior=None):
    """elbo_mirror.train with SGD without momentum and a constant rate; natural=True steps along
    (F + damping I)^-1 g.  history {loss_elbo, kl, grad_norm, natgrad_info, tvd, theta}."""
    theta = torch.nn.Parameter(torch.as_tensor(th0, dtype=torch.float32).clone())
    opt = torch.optim.SGD([theta], lr=lr, momentum=0.0)
    h = {"loss_elbo": [], "kl": [], "grad_norm": [], "natgrad_info": [], "tvd": [], "theta": []}
    for _ in range(num_epochs):
        opt.zero_grad()
        th = theta.detach().to(torch.float64).numpy()
        loss, _, g, q = em.loss_and_grad(ansatz, n, layers, th, log_p)
        info = 0
        if natural:
            g, info, _ = precondition(ansatz, n, layers, th, q, g, damping)
        theta.grad = torch.as_tensor(g, dtype=torch.float32)
        gn = torch.nn.utils.clip_grad_norm_([theta], clip)
        opt.step()
        h["loss_elbo"].append(loss)
        h["kl"].append(loss + log_evidence)
        h["grad_norm"].append(float(gn))
        h["natgrad_info"].append(info)
        h["theta"].append(theta.detach().clone().numpy())
        if posterior is not None:
            q_now = oc.probs(ansatz, n, layers, theta.detach().to(torch.float64).numpy())
            h["tvd"].append(0.5 * float(np.abs(q_now - posterior).sum()))
    return h


# The recorded Sprinkler run (tests/golden/make_golden_natgrad.py writes it, the host and GPU tests read these settings).
SPRINKLER_CASE = ("hardware_efficient", 3, 4)
SPRINKLER_LR = 0.3
SPRINKLER_EPOCHS = 40
KL_THRESHOLD = 1e-6          # what the GPU trainer test asserts at the end of the run (the ELBO trainer test's threshold)
KL_MARGIN = 100.0            # the mirror alone must end this far below it


def sprinkler_run(natural=True):
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    ansatz, n, L = SPRINKLER_CASE
    log_p, log_ev = em.log_joint(get_sprinkler_network(False), ['C', 'S', 'R'], {'W': 1})
    th0 = em.theta0(oc.num_params(ansatz, n, L))
    h = train(ansatz, n, L, log_p, log_ev, th0, SPRINKLER_LR, SPRINKLER_EPOCHS, natural=natural,
              posterior=np.exp(log_p - log_ev))
    return h, th0
