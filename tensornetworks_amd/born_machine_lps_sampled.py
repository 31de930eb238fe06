"""Matrix-product-state Born machine as a LOCALLY PURIFIED STATE, through samples only: the last level
of the hierarchy of Glasser et al. 2019.  Every site carries a second index mu that is summed out:

  cores float64 [n, 2, m, D, D], real;  A_k[s, mu] in R^{D x D}
  psi(z, mu) = e0^T A_1[z_1, mu_1] ... A_n[z_n, mu_n] e0,   T(z) = sum_mu psi(z, mu)^2,   q(z) = T(z) / Z,   Z = sum_z T(z)
  1 <= n <= 63, 1 <= D <= 16, 1 <= m <= 4;  bit order, index word and boundary vectors as in the real family.

The real Born MPS is m = 1 (from_real), the complex Born MPS at bond D is a purified one at bond 2 D with m = 2 at one site
(from_complex); the non-negative MPS / hidden Markov family is contained too.

The training surface is ComplexSampledMPSBornMachine's: kernel_input, environments, draw, score_gradient, sample_indices,
score_vjp, log_prob, bits_of, indices_of, sample, get_log_q_z_x, num_parameters, bond_dim (bornvi_lps_environments / _sample /
_score_vjp).  For n <= 20 the enumerated q is read out by log_prob over all 2^n indices (probabilities64 / get_probabilities,
detached).  Canonical form, bond spectra, compress_ / expand_, the posterior queries and two-site sweeps exist for the real
family only (SampledMPSBornMachine); here each raises a ValueError that says so.
"""
import math

import torch
import torch.nn as nn

from . import backend
from .born_machine_base import bits_to_indices, indices_to_bits
from .born_machine_cmps_sampled import ENUMERATED_MAX_N, ComplexSampledMPSBornMachine


def _refused(name):
    def method(self, *args, **kwargs):
        raise ValueError(f"{name} is not offered for purified cores: it exists for the real family (SampledMPSBornMachine) only")
    method.__name__ = name
    method.__doc__ = f"Not offered for purified cores (SampledMPSBornMachine has {name})."
    return method


def _checked_int(value, lo, hi, what):
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError(f"{what} must be an integer in {lo} ... {hi}, got {value!r}")
    return value


class PurifiedSampledMPSBornMachine(nn.Module):
    """Locally purified MPS Born machine whose surface is samples, log q of samples and the score-function gradient."""

    REFUSED = ComplexSampledMPSBornMachine.REFUSED

    def __init__(self, num_latent_vars, bond_dim=4, purification_dim=2, init_method='small_random', conditioning_dim=0, seed=0):
        if conditioning_dim != 0:
            raise ValueError("PurifiedSampledMPSBornMachine is not conditional: conditioning_dim must be 0.")
        _checked_int(num_latent_vars, 1, backend.MPS_SAMPLED_MAX_N, "num_latent_vars")
        _checked_int(bond_dim, 1, backend.LPS_MAX_BOND, "bond_dim (purified cores)")
        _checked_int(purification_dim, 1, backend.LPS_MAX_PURIFICATION, "purification_dim")
        if init_method not in ('small_random', 'zero', 'random'):
            raise ValueError(f"init_method must be 'small_random', 'zero' or 'random', got {init_method!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an integer, got {seed!r}")
        super().__init__()
        n, D, m = num_latent_vars, bond_dim, purification_dim
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
        self.num_latent_vars = n
        self.conditioning_dim = 0
        self.seed = seed
        self._draws = 0            # epoch of the next sample() call: successive calls draw fresh samples
        self.cores = nn.Parameter(torch.cat((first.unsqueeze(2), rest), dim=2).contiguous())

    # ---- constructors from other states ---------------------------------------------------------------------------
    @classmethod
    def _with_cores(cls, cores, seed=0):
        n, m, D = int(cores.shape[0]), int(cores.shape[2]), int(cores.shape[3])
        machine = cls(n, bond_dim=D, purification_dim=m, init_method='zero', seed=seed)
        with torch.no_grad():
            machine.cores.copy_(cores)
        return machine

    @classmethod
    def from_real(cls, machine, purification_dim=1):
        """The machine of the same q as a real MPS machine (cores [n, 2, D, D]): its cores in mu = 0, zeros elsewhere."""
        cores = getattr(machine, "cores", None)
        if not torch.is_tensor(cores) or cores.dim() != 4 or cores.shape[1] != 2 or cores.shape[2] != cores.shape[3]:
            raise ValueError("from_real takes a real MPS machine with cores [n, 2, D, D]")
        if cores.shape[2] > backend.LPS_MAX_BOND:
            raise ValueError(f"purified cores take a bond dimension of at most {backend.LPS_MAX_BOND}, got {int(cores.shape[2])}")
        m = _checked_int(purification_dim, 1, backend.LPS_MAX_PURIFICATION, "purification_dim")
        re = cores.detach().to(device="cpu", dtype=torch.float64)
        out = torch.zeros(re.shape[0], 2, m, re.shape[2], re.shape[3], dtype=torch.float64)
        out[:, :, 0] = re
        return cls._with_cores(out, seed=getattr(machine, "seed", 0)).to(cores.device)

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
        return cls._with_cores(out, seed=getattr(machine, "seed", 0)).to(cores.device)

    # ---- the parameter ---------------------------------------------------------------------------------------------
    @property
    def bond_dim(self):
        return int(self.cores.shape[3])

    @property
    def purification_dim(self):
        return int(self.cores.shape[2])

    @property
    def num_parameters(self):
        return self.cores.numel()

    def kernel_input(self):
        """(cores detached as a contiguous float64 [n, 2, m, D, D] tensor on the compute device, the parameter's own device)."""
        home = self.cores.device
        return self.cores.detach().to(device=backend.compute_device(home), dtype=torch.float64).contiguous(), home

    # ---- the three calls a trainer needs (the real and the complex machine have the same three) -------------------------
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

    # ---- samples ----------------------------------------------------------------------------------------------
    def sample_indices(self, num_samples, seed=None, epoch=0):
        """(idx int64 [num], logq float64 [num]) on the compute device: exact draws z ~ q and their log q.  A pure function
        of (cores, seed, epoch): seed defaults to the machine's own."""
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
            raise ValueError(f"num_samples must be a positive integer, got {num_samples!r}")
        cores, _ = self.kernel_input()
        ep = torch.tensor([int(epoch)], dtype=torch.int64, device=cores.device)
        self.environments(cores, num_samples)
        idx, logq, _ = self.draw(cores, num_samples, self.seed if seed is None else seed, ep)
        return idx, logq

    def bits_of(self, idx):
        """float32 bit rows [B, n] of outcome indices."""
        return indices_to_bits(idx, self.num_latent_vars)

    def indices_of(self, z_samples):
        """int64 outcome indices of bit rows [B, n]."""
        return bits_to_indices(z_samples, self.num_latent_vars)

    def sample(self, num_samples=1, x_condition=None):
        """float32 bit rows [num, n] on the parameter's device, from the draws of sample_indices (fresh ones every call)."""
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")
        idx, _ = self.sample_indices(num_samples, epoch=self._draws)
        self._draws += 1
        return self.bits_of(idx).to(self.cores.device)

    def score_vjp(self, idx, w):
        """(grad float64 [n, 2, m, D, D] = the gradient of sum_b w_b log q(idx_b) in the parameter, logq float64 [B]) on the
        compute device."""
        cores, _ = self.kernel_input()
        idx = idx.to(device=cores.device, dtype=torch.int64).contiguous()
        w = w.to(device=cores.device, dtype=torch.float64).contiguous()
        self.environments(cores, int(idx.numel()))
        grad, logq, _ = self.score_gradient(cores, idx, w)
        return grad, logq

    def log_prob(self, idx):
        """log q(idx), float64 [B] (-inf where T is 0): the score call without a gradient."""
        cores, _ = self.kernel_input()
        idx = idx.reshape(-1).to(device=cores.device, dtype=torch.int64).contiguous()
        self.environments(cores, int(idx.numel()))
        return backend.lps_score_vjp(cores, idx, out=False)[1]

    def get_log_q_z_x(self, z_samples, x_condition=None):
        """log q(z) for a batch of bit rows, float64."""
        if x_condition is not None:
            raise ValueError("x_condition provided but Born machine is not conditional.")
        return self.log_prob(self.indices_of(z_samples)).to(z_samples.device)

    # ---- the enumerated distribution, where it exists ------------------------------------------------------------
    def probabilities64(self, x_condition=None):
        """float64 [2^n] on the parameter's device, detached (n <= 20): exp(log_prob) of all 2^n indices, one call."""
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")
        if self.num_latent_vars > ENUMERATED_MAX_N:
            raise ValueError(f"the 2^n probabilities exist for num_latent_vars <= {ENUMERATED_MAX_N} only "
                             f"(got {self.num_latent_vars}): use sample_indices and log_prob")
        dev = backend.compute_device(self.cores.device)
        idx = torch.arange(1 << self.num_latent_vars, dtype=torch.int64, device=dev)
        return torch.exp(self.log_prob(idx)).to(self.cores.device)

    def get_probabilities(self, x_condition=None):
        """float32 [1, 2^n], detached (n <= 20)."""
        return self.probabilities64(x_condition).to(torch.float32).unsqueeze(0)


for _name in PurifiedSampledMPSBornMachine.REFUSED:
    setattr(PurifiedSampledMPSBornMachine, _name, _refused(_name))
del _name
