"""Matrix-product-state (tensor-train) Born machine on MI355X: the classical family with a parameter count polynomial in n.

  q(z) = psi(z)^2 / Z,   psi(z) = e0^T A_1[z_1] A_2[z_2] ... A_n[z_n] e0,   Z = sum_z psi(z)^2

with one float64 parameter `cores` of shape [n, 2, D, D] (A_k[s][a][b]: a the left bond, b the right bond; tuple position 0
is the most significant bit of the outcome index).  No reference counterpart: the reference's classical family is the
2^n-entry table.  The surface is born_machine_base.EnumeratedBornMachine's, the one ClassicalBornMachine has, so the
classical trainers take either family; the checks and initialisations of `cores` are born_machine_base's, shared with the
sampled machine.  cores -> q is one `bornvi_mps_probs` call (prefix-doubling sweep), wrapped in a torch.autograd.Function
whose backward is `bornvi_mps_vjp`; both run on backend.compute_device(...) and results come back on the parameter's device.
"""
import torch

from . import backend
from .born_machine_base import EnumeratedBornMachine, EpochForward, MPSCores, new_mps_cores


class _MPSProbs(torch.autograd.Function):
    """q64 = mps_probs(cores); backward: mps_vjp with g = dL/dq.  The backward runs the forward sweep again first: the
    levels live in a workspace shared by every machine of this shape, and another forward may have run in between."""

    @staticmethod
    def forward(ctx, cores):
        _, q64, _, _ = backend.mps_probs(cores, want_q32=False)
        ctx.save_for_backward(cores)
        return q64

    @staticmethod
    def backward(ctx, grad_q):
        cores, = ctx.saved_tensors
        backend.mps_probs(cores, want_q32=False)
        return backend.mps_vjp(cores, grad_q.to(torch.float64).contiguous())


class MPSBornMachine(MPSCores, EnumeratedBornMachine):
    """Born machine over the 2^n latent states whose amplitude is a product of n pairs of D x D matrices."""

    def __init__(self, num_latent_vars, bond_dim=4, init_method='small_random', conditioning_dim=0):
        cores = new_mps_cores("MPSBornMachine", num_latent_vars, bond_dim, init_method, conditioning_dim, backend.MPS_MAX_N)
        super().__init__(num_latent_vars)
        self.cores = cores

    def probabilities64(self, x_condition=None):
        """float64 [2^n], differentiable: q as the kernels compute it, before the float32 cast."""
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")
        cores, home = self.kernel_input()
        return _MPSProbs.apply(cores).to(home)

    def _probabilities(self, x_condition):
        return self.probabilities64(x_condition).to(torch.float32).unsqueeze(0)

    def _entropy(self, x_condition):
        """float64, from the kernels' q (the fixed probabilities' entropy is float32)."""
        probs = self.probabilities64(x_condition)
        return -(probs * torch.log(probs.clamp(min=1e-10))).sum()

    # ---- the two ends of a training epoch: cores -> q, and dL/dq -> the cores' gradient
    def epoch_forward(self, x_condition, want_entropy):
        """state = (cores float64 on the compute device, log max(q, 1e-10) or None); the entropy is float64.  Leaves the
        sweep in the workspace for epoch_backward."""
        cores, _ = self.kernel_input(detach=True)
        q32, q64, _, _ = backend.mps_probs(cores)
        logq = torch.log(q64.clamp(min=1e-10)) if want_entropy else None
        return EpochForward(q32, q64, -(q64 * logq).sum().reshape(1) if want_entropy else None, (cores, logq))

    def epoch_backward(self, fwd, y, ksd2=None, entropy_weight=0.0):
        cores, logq = fwd.state
        loss, g = None, y.reshape(-1)
        if ksd2 is not None:            # the clamp passes no gradient below 1e-12 (bornvi_born_table_vjp's convention)
            loss = torch.sqrt(ksd2.clamp(min=1e-12))
            g = torch.where(ksd2 >= 1e-12, g / loss, torch.zeros_like(g))
        if entropy_weight != 0.0:       # d(-H)/dq = log max(q, 1e-10) + [q >= 1e-10]
            if logq is None:
                logq = torch.log(fwd.q64.clamp(min=1e-10))
            g = g + entropy_weight * (logq + (fwd.q64 >= 1e-10).to(torch.float64))
        grad = backend.mps_vjp(cores, g.contiguous())
        return loss, [(self.cores, grad.to(device=self.cores.device, dtype=self.cores.dtype))]
