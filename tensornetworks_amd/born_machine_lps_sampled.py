"""Matrix-product-state Born machine as a LOCALLY PURIFIED STATE, through samples only: the last level
of the hierarchy of Glasser et al. 2019.  Every site carries a second index mu that is summed out:

  cores float64 [n, 2, m, D, D], real;  A_k[s, mu] in R^{D x D}
  psi(z, mu) = e0^T A_1[z_1, mu_1] ... A_n[z_n, mu_n] e0,   T(z) = sum_mu psi(z, mu)^2,   q(z) = T(z) / Z,   Z = sum_z T(z)
  1 <= n <= 63, 1 <= D <= 16, 1 <= m <= 4;  bit order, index word and boundary vectors as in the real family.

The real Born MPS is m = 1 (from_real), the complex Born MPS at bond D is a purified one at bond 2 D with m = 2 at one site
(from_complex); the non-negative MPS / hidden Markov family is contained too.

The training surface is born_machine_sampled's SampledSurface, the one the real and the complex machine have: kernel_input,
sample_indices, score_vjp, log_prob, bits_of, indices_of, sample, get_log_q_z_x, num_parameters, through this file's three
hooks environments, draw and score_gradient (bornvi_lps_environments / _sample / _score_vjp); bond_dim and log_prob are its
own.  For n <= 20 the enumerated q is read out by log_prob over all 2^n indices (probabilities64 / get_probabilities,
detached).  Canonical form, bond spectra, compress_ / expand_, the posterior queries and two-site sweeps exist for the real
family only (SampledMPSBornMachine); here each raises a ValueError that says so.
"""
import math

import torch
import torch.nn as nn

from . import backend
from .born_machine_sampled import SampledSurface, checked_init_method, checked_int, checked_seed, refuse

ENUMERATED_MAX_N = SampledSurface.ENUMERATED_MAX_N          # probabilities64: log_prob over all 2^n indices in one call

@refuse
class PurifiedSampledMPSBornMachine(SampledSurface, nn.Module):
    """Locally purified MPS Born machine whose surface is samples, log q of samples and the score-function gradient."""
    CORES = "purified cores"

    def __init__(self, num_latent_vars, bond_dim=4, purification_dim=2, init_method='small_random', conditioning_dim=0, seed=0):
        if conditioning_dim != 0:
            raise ValueError("PurifiedSampledMPSBornMachine is not conditional: conditioning_dim must be 0.")
        n = checked_int(num_latent_vars, 1, backend.MPS_SAMPLED_MAX_N, "num_latent_vars")
        D = checked_int(bond_dim, 1, backend.LPS_MAX_BOND, "bond_dim (purified cores)")
        m = checked_int(purification_dim, 1, backend.LPS_MAX_PURIFICATION, "purification_dim")
        checked_init_method(init_method)
        checked_seed(seed)
        super().__init__()
        eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
        rest = torch.zeros(n, 2, m - 1, D, D, dtype=torch.float64)
        if init_method == 'zero':            # psi(z, 0) = 2^(-n/2) for every z and nothing else: the exactly uniform q
            first = eye / math.sqrt(2.0)
        elif init_method == 'small_random':  # the real family's draw in mu = 0, then a second one of the same scale in mu >= 1
            first = (eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / math.sqrt(2.0)
            rest = 0.1 * torch.randn(n, 2, m - 1, D, D, dtype=torch.float64) / math.sqrt(2.0)
        else:                                # the real family's variance 1 / (2 D), split between the m matrices
            first = torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(2.0 * D * m)
            rest = torch.randn(n, 2, m - 1, D, D, dtype=torch.float64) / math.sqrt(2.0 * D * m)
        self._init_sampled(n, seed)
        self.cores = nn.Parameter(torch.cat((first.unsqueeze(2), rest), dim=2).contiguous())

    # ---- constructors from other states ---------------------------------------------------------------------------
    @classmethod
    def _of(cls, cores, machine):
        """The machine of purified cores [n, 2, m, D, D] built on the CPU, with `machine`'s seed, on `machine`'s device."""
        out = cls._with_cores(cores, seed=getattr(machine, "seed", 0), bond_dim=int(cores.shape[3]), purification_dim=int(cores.shape[2]))
        return out.to(machine.cores.device)

    @classmethod
    def from_real(cls, machine, purification_dim=1):
        """The machine of the same q as a real MPS machine (cores [n, 2, D, D]): its cores in mu = 0, zeros elsewhere."""
        cores = getattr(machine, "cores", None)
        if not torch.is_tensor(cores) or cores.dim() != 4 or cores.shape[1] != 2 or cores.shape[2] != cores.shape[3]:
            raise ValueError("from_real takes a real MPS machine with cores [n, 2, D, D]")
        if cores.shape[2] > backend.LPS_MAX_BOND:
            raise ValueError(f"purified cores take a bond dimension of at most {backend.LPS_MAX_BOND}, got {int(cores.shape[2])}")
        m = checked_int(purification_dim, 1, backend.LPS_MAX_PURIFICATION, "purification_dim")
        re = cores.detach().to(device="cpu", dtype=torch.float64)
        out = torch.zeros(re.shape[0], 2, m, re.shape[2], re.shape[3], dtype=torch.float64)
        out[:, :, 0] = re
        return cls._of(out, machine)

    @classmethod
    def from_complex(cls, machine):
        """The machine of the same q as a complex MPS machine (cores [n, 2, D, D, 2], 2 D <= 16), at bond 2 D with m = 2.
        A complex row vector x + i y is the real row (x, y), so A = X + iY acts as [[X, Y], [-Y, X]]: that block matrix goes in
        mu = 0 at every site.  mu = 1 is used at the last site only, where it holds the column that selects the imaginary part
        of psi (column D of the block matrix, moved to column 0): T(z) = (Re psi)^2 + (Im psi)^2."""
        cores = getattr(machine, "cores", None)
        if not torch.is_tensor(cores) or cores.dim() != 5 or cores.shape[1] != 2 or cores.shape[2] != cores.shape[3] or cores.shape[4] != 2:
            raise ValueError("from_complex takes a complex MPS machine with cores [n, 2, D, D, 2]")
        n, D = int(cores.shape[0]), int(cores.shape[2])
        if 2 * D > backend.LPS_MAX_BOND:
            raise ValueError(f"from_complex doubles the bond dimension: 2 D <= {backend.LPS_MAX_BOND}, got D = {D}")
        c = cores.detach().to(device="cpu", dtype=torch.float64)
        X, Y = c[..., 0], c[..., 1]
        out = torch.zeros(n, 2, 2, 2 * D, 2 * D, dtype=torch.float64)
        out[:, :, 0, :D, :D] = X
        out[:, :, 0, :D, D:] = Y
        out[:, :, 0, D:, :D] = -Y
        out[:, :, 0, D:, D:] = X
        out[n - 1, :, 1, :, 0] = out[n - 1, :, 0, :, D]
        return cls._of(out, machine)

    # ---- the parameter ---------------------------------------------------------------------------------------------
    @property
    def bond_dim(self):
        return int(self.cores.shape[3])

    @property
    def purification_dim(self):
        return int(self.cores.shape[2])

    # ---- the three calls the shared surface and a trainer need -----------------------------------------------------------
    def environments(self, cores, num_samples):
        return backend.lps_environments(cores, num_samples)

    def draw(self, cores, num_samples, seed, epoch_dev):
        """(idx, logq, status): the sampler's draws, then their log q through the score call without a gradient (the
        sampler's vector carries the norm of the joint (z, mu), not of z); the two status words or-ed."""
        idx, _, st_s = backend.lps_sample(cores, num_samples, seed, epoch_dev)
        _, logq, st_q = backend.lps_score_vjp(cores, idx, out=False)
        return idx, logq, st_s | st_q

    def score_gradient(self, cores, idx, w):
        return backend.lps_score_vjp(cores, idx, w)

    def log_prob(self, idx):
        """log q(idx), float64 [B] (-inf where T is 0): the score call without a gradient."""
        cores, _ = self.kernel_input()
        idx = idx.reshape(-1).to(device=cores.device, dtype=torch.int64).contiguous()
        self.environments(cores, int(idx.numel()))
        return backend.lps_score_vjp(cores, idx, out=False)[1]
