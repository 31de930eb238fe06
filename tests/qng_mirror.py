"""Float64 NumPy mirror of the quantum natural gradient (test infrastructure, not under test).

Every parameter enters exactly one gate exp(-i theta s / 2), so d_a psi = 1/2 phi_a with phi_a = psi(theta + pi e_a), and

  Q_ab = Re<phi_a|phi_b> - Re(conj(c_a) c_b),  c_a = <psi|phi_a>

is the quantum Fisher information, 4 x the Fubini-Study metric.  The states come from oracle.circuit.simulate; the solve
and its status rule are natgrad_mirror.spd_solve's; the training run is natgrad_mirror.train with Q in place of F."""
import numpy as np
import torch

import elbo_mirror as em
import natgrad_mirror as nm
from oracle import circuit as oc

DAMPING = nm.DAMPING


def states(ansatz, n, layers, theta):
    """(psi [2^n], phi [P, 2^n]) complex128: the circuit's state and its pi-shifted states."""
    theta = np.asarray(theta, dtype=np.float64)
    gates = oc.gate_list(ansatz, n, layers)
    psi = oc.simulate(gates, n, theta)
    phi = np.empty((theta.size, 1 << n), dtype=np.complex128)
    for a in range(theta.size):
        t = theta.copy()
        t[a] += np.pi
        phi[a] = oc.simulate(gates, n, t)
    return psi, phi


def real_rows(x):
    """complex [.., N] -> float64 [.., 2 N], (re, im) interleaved: the rows of the real Gram."""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    return x.view(np.float64).reshape(x.shape[:-1] + (2 * x.shape[-1],))


def qfi(phi, psi):
    """Q [P, P] float64 from phi [P, N], psi [N]: a real Gram over 2 N columns minus the projection term."""
    R = real_rows(phi)
    G = R @ R.T
    re = R @ real_rows(psi)                      # Re c_a
    im = R @ real_rows(1j * np.asarray(psi))     # Im c_a
    Q = G - (np.outer(re, re) + np.outer(im, im))
    return 0.5 * (Q + Q.T)                       # (exact: both halves are the same sums up to the order of two products)


def qfi_of_circuit(ansatz, n, layers, theta):
    psi, phi = states(ansatz, n, layers, theta)
    return qfi(phi, psi)


def precondition(ansatz, n, layers, theta, grad, damping=DAMPING):
    Q = qfi_of_circuit(ansatz, n, layers, theta)
    return nm.spd_solve(Q, grad, damping) + (Q,)


def train(ansatz, n, layers, log_p, log_evidence, th0, lr, num_epochs, damping=DAMPING, clip=10.0, posterior=None):
    """natgrad_mirror.train with delta = (Q + damping I)^-1 g.  history {loss_elbo, kl, grad_norm, natgrad_info, tvd, theta}."""
    theta = torch.nn.Parameter(torch.as_tensor(th0, dtype=torch.float32).clone())
    opt = torch.optim.SGD([theta], lr=lr, momentum=0.0)
    h = {"loss_elbo": [], "kl": [], "grad_norm": [], "natgrad_info": [], "tvd": [], "theta": []}
    for _ in range(num_epochs):
        opt.zero_grad()
        th = theta.detach().to(torch.float64).numpy()
        loss, _, g, q = em.loss_and_grad(ansatz, n, layers, th, log_p)
        g, info, _ = precondition(ansatz, n, layers, th, g, damping)
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


def sprinkler_run():
    """The natural-gradient golden run's settings (natgrad_mirror.SPRINKLER_*), with the quantum metric."""
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    ansatz, n, L = nm.SPRINKLER_CASE
    log_p, log_ev = em.log_joint(get_sprinkler_network(False), ['C', 'S', 'R'], {'W': 1})
    th0 = em.theta0(oc.num_params(ansatz, n, L))
    h = train(ansatz, n, L, log_p, log_ev, th0, nm.SPRINKLER_LR, nm.SPRINKLER_EPOCHS, posterior=np.exp(log_p - log_ev))
    return h, th0
