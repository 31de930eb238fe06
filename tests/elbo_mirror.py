"""Float64 NumPy mirror of the exact-ELBO objective and of one ELBO training run (test infrastructure, not under test).

  l_z = log max(q_z, q_floor);  w_z = l_z - log_p_z + [q_z >= q_floor];
  loss = sum_z q_z (l_z - log_p_z), a term with q_z == 0 exactly 0;  entropy = -sum_z q_z l_z

The gradient is oracle.circuit.paramshift_vjp with dL/dq = w; the epoch is oracle.ksd.EpochTrace's (float32 theta, torch's
CPU Adam, CosineAnnealingLR to lr / 10, clip_grad_norm_) with the loss swapped."""
import math

import numpy as np
import torch

from oracle import circuit as oc
from tensornetworks_amd.bayesian_network import joint_table

Q_FLOOR = 1e-10
P_FLOOR = 1e-30


def weights(q, log_p, q_floor=Q_FLOOR):
    """(loss, entropy, w) of one row q [N] against log_p [N], float64."""
    q = np.asarray(q, dtype=np.float64)
    log_p = np.asarray(log_p, dtype=np.float64)
    l = np.log(np.where(q < q_floor, q_floor, q))
    d = l - log_p
    with np.errstate(invalid="ignore"):
        loss = float(np.where(q == 0.0, 0.0, q * d).sum())
        ent = -float(np.where(q == 0.0, 0.0, q * l).sum())
    return loss, ent, d + (q >= q_floor)


def log_joint(bn, latent, x, p_floor=P_FLOOR):
    """(log max(p(x, z), p_floor) [2^n], log p(x)) by enumeration on the host."""
    pxz = joint_table(bn, latent, x)
    return np.log(np.maximum(pxz, p_floor)), math.log(float(pxz.sum()))


def loss_and_grad(ansatz, n, layers, theta, log_p, q_floor=Q_FLOOR):
    """(loss, entropy, grad [P], q) at theta (float64)."""
    q = oc.probs(ansatz, n, layers, theta)
    loss, ent, w = weights(q, log_p, q_floor)
    return loss, ent, oc.paramshift_vjp(ansatz, n, layers, theta, w), q


def theta0(P, seed=0):
    """0.1 N(0, 1) from numpy.random.default_rng(seed), as float32 (what the trainers hold)."""
    return (0.1 * np.random.default_rng(seed).standard_normal(P)).astype(np.float32)


def train(ansatz, n, layers, log_p, log_evidence, th0, lr, num_epochs, clip=10.0, posterior=None):
    """history {loss_elbo, kl, entropy, grad_norm, tvd, theta}: loss, KL and entropy of q BEFORE the epoch's update, the TVD
    to `posterior` after it (as the trainers record them)."""
    theta = torch.nn.Parameter(torch.as_tensor(th0, dtype=torch.float32).clone())
    opt = torch.optim.Adam([theta], lr=lr, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=num_epochs, eta_min=lr / 10)
    h = {"loss_elbo": [], "kl": [], "entropy": [], "grad_norm": [], "tvd": [], "theta": []}
    for _ in range(num_epochs):
        opt.zero_grad()
        th = theta.detach().to(torch.float64).numpy()
        loss, ent, g, _ = loss_and_grad(ansatz, n, layers, th, log_p)
        theta.grad = torch.as_tensor(g, dtype=torch.float32)
        gn = torch.nn.utils.clip_grad_norm_([theta], clip)
        opt.step()
        sched.step()
        h["loss_elbo"].append(loss)
        h["kl"].append(loss + log_evidence)
        h["entropy"].append(ent)
        h["grad_norm"].append(float(gn))
        h["theta"].append(theta.detach().clone().numpy())
        if posterior is not None:
            q_now = oc.probs(ansatz, n, layers, theta.detach().to(torch.float64).numpy())
            h["tvd"].append(0.5 * float(np.abs(q_now - posterior).sum()))
    return h
