"""Matrix-product-state (tensor-train) Born machine on MI355X: the classical family with a parameter count polynomial in n.

  q(z) = psi(z)^2 / Z,   psi(z) = e0^T A_1[z_1] A_2[z_2] ... A_n[z_n] e0,   Z = sum_z psi(z)^2

with one float64 parameter `cores` of shape [n, 2, D, D] (A_k[s][a][b]: a the left bond, b the right bond; tuple position 0
is the most significant bit of the outcome index).  No reference counterpart: the reference's classical family is the
2^n-entry table.  The surface is ClassicalBornMachine's (get_probabilities, probabilities64, sample, get_prob_dict,
get_log_q_z_x, entropy, set_fixed_probs / clear_fixed_probs, the same shapes and messages), so the classical trainers take
either family.  cores -> q is one `bornvi_mps_probs` call (prefix-doubling sweep), wrapped in a torch.autograd.Function
whose backward is `bornvi_mps_vjp`; both run on backend.compute_device(...) and results come back on the parameter's device.
"""
import math

import torch
import torch.nn as nn

from . import backend
from .utils import generate_all_binary_outcomes


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


class MPSBornMachine(nn.Module):
    """Born machine over the 2^n latent states whose amplitude is a product of n pairs of D x D matrices."""

    def __init__(self, num_latent_vars, bond_dim=4, init_method='small_random', conditioning_dim=0):
        super().__init__()
        if conditioning_dim != 0:
            raise ValueError("MPSBornMachine is not conditional: conditioning_dim must be 0.")
        if isinstance(num_latent_vars, bool) or not isinstance(num_latent_vars, int) or not 1 <= num_latent_vars <= backend.MPS_MAX_N:
            raise ValueError(f"num_latent_vars must be an integer in 1 ... {backend.MPS_MAX_N}, got {num_latent_vars!r}")
        if isinstance(bond_dim, bool) or not isinstance(bond_dim, int) or not 1 <= bond_dim <= backend.MPS_MAX_BOND:
            raise ValueError(f"bond_dim must be an integer in 1 ... {backend.MPS_MAX_BOND}, got {bond_dim!r}")
        if init_method not in ('small_random', 'zero', 'random'):
            raise ValueError(f"init_method must be 'small_random', 'zero' or 'random', got {init_method!r}")
        self.num_latent_vars = num_latent_vars
        self.num_outcomes = 2 ** num_latent_vars
        self.bond_dim = bond_dim
        self.conditioning_dim = 0
        self._fixed_probs = None
        self._use_fixed_probs = False
        self._outcomes = None

        n, D = num_latent_vars, bond_dim
        eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
        if init_method == 'zero':            # psi(z) = 2^(-n/2) for every z: the exactly uniform q
            init = eye / math.sqrt(2.0)
        elif init_method == 'small_random':
            init = (eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / math.sqrt(2.0)
        else:
            init = torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(2.0 * D)
        self.cores = nn.Parameter(init.clone().contiguous())

    @property
    def num_parameters(self):
        return self.cores.numel()

    @property
    def all_outcome_tuples(self):
        """generate_all_binary_outcomes(n), built on first use (2^n Python tuples that no hot path needs)."""
        if self._outcomes is None:
            self._outcomes = generate_all_binary_outcomes(self.num_latent_vars)
        return self._outcomes

    def set_fixed_probs(self, prob_tensor):
        """From now on get_probabilities returns (a copy of) this tensor."""
        self._fixed_probs = prob_tensor.detach().clone()
        self._use_fixed_probs = True

    def clear_fixed_probs(self):
        self._fixed_probs = None
        self._use_fixed_probs = False

    @staticmethod
    def _check_unconditioned(x_condition):
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")

    def kernel_input(self):
        """(cores as a contiguous float64 tensor on the compute device -- differentiable --, the parameter's own device)."""
        home = self.cores.device
        return self.cores.to(device=backend.compute_device(home), dtype=torch.float64).contiguous(), home

    def probabilities64(self, x_condition=None):
        """float64 [2^n], differentiable: q as the kernels compute it, before the float32 cast."""
        self._check_unconditioned(x_condition)
        cores, home = self.kernel_input()
        return _MPSProbs.apply(cores).to(home)

    def get_probabilities(self, x_condition=None):
        """float32 [1, 2^n], differentiable; the fixed probabilities when set."""
        if self._use_fixed_probs and self._fixed_probs is not None:
            return self._fixed_probs.unsqueeze(0) if self._fixed_probs.ndim == 1 else self._fixed_probs
        return self.probabilities64(x_condition).to(torch.float32).unsqueeze(0)

    def sample(self, num_samples=1, x_condition=None):
        """float32 bit rows [num, n]."""
        probs = self.get_probabilities(x_condition).detach()
        probs = probs + 1e-10
        probs = probs / probs.sum(dim=-1, keepdim=True)
        idx = torch.multinomial(probs, num_samples, replacement=True)            # [1, num]
        n = self.num_latent_vars
        shifts = torch.arange(n - 1, -1, -1, device=idx.device)
        bits = ((idx.unsqueeze(-1) >> shifts) & 1).to(torch.float32)
        return bits[0]

    def get_prob_dict(self, x_condition=None):
        """{outcome tuple: probability}."""
        probs_1d = self.get_probabilities(x_condition).squeeze().detach().cpu().numpy().reshape(-1)
        return dict(zip(self.all_outcome_tuples, probs_1d))

    def get_log_q_z_x(self, z_samples, x_condition=None):
        """log max(q(z), 1e-10) for a batch of bit rows."""
        if x_condition is not None:
            raise ValueError("x_condition provided but Born machine is not conditional.")
        probs = self.get_probabilities()
        log_probs = torch.log(probs.clamp(min=1e-10))
        bz = z_samples.shape[0]
        z = z_samples.detach().to(log_probs.device).long()      # `.long()` truncates like the table family's
        n = self.num_latent_vars
        if z.dim() == 2 and z.shape[1] == n:
            bad = ((z != 0) & (z != 1)).any(dim=1)
        else:
            bad = torch.ones(bz, dtype=torch.bool, device=z.device)
        if bool(bad.any()):
            row = int(torch.nonzero(bad)[0])
            raise ValueError(f"Sample {tuple(z[row].tolist())} is not a valid outcome.")
        idx = (z * (1 << torch.arange(n - 1, -1, -1, device=z.device))).sum(dim=1)
        return log_probs[0, idx]

    def entropy(self, x_condition=None):
        """-sum q log max(q, 1e-10), differentiable (float64 from the kernels' q; float32 from fixed probabilities)."""
        if self._use_fixed_probs and self._fixed_probs is not None:
            probs = self.get_probabilities(x_condition).squeeze()
        else:
            probs = self.probabilities64(x_condition)
        return -(probs * torch.log(probs.clamp(min=1e-10))).sum()
