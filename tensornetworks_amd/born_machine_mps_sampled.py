"""Matrix-product-state Born machine through samples only: the family of born_machine_mps.py without any 2^n object.

  q(z) = psi(z)^2 / Z,   psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0,   cores float64 [n, 2, D, D],   1 <= n <= 63

An exact draw z ~ q costs O(n D^2) (ancestral sampling against the right environments), and so do log q(z) and
grad log q(z) for a given z (bornvi_mps_environments / bornvi_mps_sample / bornvi_mps_score_vjp).
A sample is an int64 outcome index, idx = sum_k z_k 2^(n-k) (tuple position 0 = the most significant bit), or a float32
bit row.  Same `cores` parameter, initialisations and messages as MPSBornMachine.  For n <= 26 the enumerated q is still
there (probabilities64 / get_probabilities, through backend.mps_probs); above that those raise.
"""
import math

import torch
import torch.nn as nn

from . import backend
from .born_machine_mps import _MPSProbs


class SampledMPSBornMachine(nn.Module):
    """MPS Born machine whose surface is samples, log q of samples and the score-function gradient."""

    def __init__(self, num_latent_vars, bond_dim=4, init_method='small_random', conditioning_dim=0, seed=0):
        super().__init__()
        if conditioning_dim != 0:
            raise ValueError("SampledMPSBornMachine is not conditional: conditioning_dim must be 0.")
        if isinstance(num_latent_vars, bool) or not isinstance(num_latent_vars, int) \
                or not 1 <= num_latent_vars <= backend.MPS_SAMPLED_MAX_N:
            raise ValueError(f"num_latent_vars must be an integer in 1 ... {backend.MPS_SAMPLED_MAX_N}, got {num_latent_vars!r}")
        if isinstance(bond_dim, bool) or not isinstance(bond_dim, int) or not 1 <= bond_dim <= backend.MPS_MAX_BOND:
            raise ValueError(f"bond_dim must be an integer in 1 ... {backend.MPS_MAX_BOND}, got {bond_dim!r}")
        if init_method not in ('small_random', 'zero', 'random'):
            raise ValueError(f"init_method must be 'small_random', 'zero' or 'random', got {init_method!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an integer, got {seed!r}")
        self.num_latent_vars = num_latent_vars
        self.bond_dim = bond_dim
        self.conditioning_dim = 0
        self.seed = seed
        self._draws = 0            # epoch of the next sample() call: successive calls draw fresh samples

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

    def kernel_input(self):
        """(cores detached as a contiguous float64 tensor on the compute device, the parameter's own device)."""
        home = self.cores.device
        return self.cores.detach().to(device=backend.compute_device(home), dtype=torch.float64).contiguous(), home

    # ---- samples ----------------------------------------------------------------------------------------------
    def sample_indices(self, num_samples, seed=None, epoch=0):
        """(idx int64 [num], logq float64 [num]) on the compute device: exact draws z ~ q and their log q.  A pure function
        of (cores, seed, epoch): seed defaults to the machine's own."""
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
            raise ValueError(f"num_samples must be a positive integer, got {num_samples!r}")
        cores, _ = self.kernel_input()
        ep = torch.tensor([int(epoch)], dtype=torch.int64, device=cores.device)
        backend.mps_environments(cores, num_samples)
        idx, logq, _ = backend.mps_sample(cores, num_samples, self.seed if seed is None else seed, ep)
        return idx, logq

    def bits_of(self, idx):
        """float32 bit rows [B, n] of outcome indices."""
        n = self.num_latent_vars
        shifts = torch.arange(n - 1, -1, -1, device=idx.device)
        return ((idx.unsqueeze(-1) >> shifts) & 1).to(torch.float32)

    def indices_of(self, z_samples):
        """int64 outcome indices of bit rows [B, n] (validated like MPSBornMachine.get_log_q_z_x)."""
        n = self.num_latent_vars
        z = z_samples.detach().long()
        if z.dim() == 2 and z.shape[1] == n:
            bad = ((z != 0) & (z != 1)).any(dim=1)
        else:
            bad = torch.ones(z.shape[0], dtype=torch.bool, device=z.device)
        if bool(bad.any()):
            row = int(torch.nonzero(bad)[0])
            raise ValueError(f"Sample {tuple(z[row].tolist())} is not a valid outcome.")
        return (z << torch.arange(n - 1, -1, -1, device=z.device)).sum(dim=1)

    def sample(self, num_samples=1, x_condition=None):
        """float32 bit rows [num, n] on the parameter's device, from the draws of sample_indices (fresh ones every call)."""
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")
        idx, _ = self.sample_indices(num_samples, epoch=self._draws)
        self._draws += 1
        return self.bits_of(idx).to(self.cores.device)

    def score_vjp(self, idx, w):
        """(grad float64 [n, 2, D, D] = sum_b w_b grad log q(idx_b), logq float64 [B]) on the compute device."""
        cores, _ = self.kernel_input()
        idx = idx.to(device=cores.device, dtype=torch.int64).contiguous()
        w = w.to(device=cores.device, dtype=torch.float64).contiguous()
        backend.mps_environments(cores, int(idx.numel()))
        grad, logq, _ = backend.mps_score_vjp(cores, idx, w)
        return grad, logq

    def log_prob(self, idx):
        """log q(idx), float64 [B] (-inf where psi is 0)."""
        idx = idx.reshape(-1)
        return self.score_vjp(idx, torch.zeros(idx.numel(), dtype=torch.float64, device=idx.device))[1]

    def get_log_q_z_x(self, z_samples, x_condition=None):
        """log q(z) for a batch of bit rows, float64 (no floor: it is evaluated per sample, not read from a table)."""
        if x_condition is not None:
            raise ValueError("x_condition provided but Born machine is not conditional.")
        return self.log_prob(self.indices_of(z_samples)).to(z_samples.device)

    # ---- the enumerated distribution, where it exists ------------------------------------------------------------
    def _check_enumerable(self):
        if self.num_latent_vars > backend.MPS_MAX_N:
            raise ValueError(f"the 2^n probabilities exist for num_latent_vars <= {backend.MPS_MAX_N} only "
                             f"(got {self.num_latent_vars}): use sample_indices and log_prob")

    def probabilities64(self, x_condition=None):
        """float64 [2^n], differentiable (n <= 26): backend.mps_probs, as MPSBornMachine."""
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")
        self._check_enumerable()
        home = self.cores.device
        cores = self.cores.to(device=backend.compute_device(home), dtype=torch.float64).contiguous()
        return _MPSProbs.apply(cores).to(home)

    def get_probabilities(self, x_condition=None):
        """float32 [1, 2^n], differentiable (n <= 26)."""
        return self.probabilities64(x_condition).to(torch.float32).unsqueeze(0)
