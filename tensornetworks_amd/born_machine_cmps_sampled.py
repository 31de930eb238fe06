"""Matrix-product-state Born machine with COMPLEX cores, through samples only: the classical
counterpart of a QuantumBornMachine state, and a strictly larger family than born_machine_mps_sampled.py's at the same bond.

  cores float64 [n, 2, D, D, 2], (re, im) last: torch.view_as_real of a complex128 [n, 2, D, D];  A_k[s] = X + iY
  psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0 in C (a plain product, no conjugate),  q(z) = |psi(z)|^2 / Z,  Z = sum_z |psi(z)|^2
  1 <= n <= 63, 1 <= D <= 16;  bit order, index word and boundary vectors as in the real family.

The training surface is SampledMPSBornMachine's: kernel_input, sample_indices, score_vjp, log_prob, bits_of, indices_of,
sample, get_log_q_z_x, num_parameters, bond_dim (bornvi_cmps_environments / _sample / _score_vjp).  The gradient is that of
the real function in the 2 . 2 n D^2 real numbers of `cores`: what a torch optimiser steps.  For n <= 20 the enumerated q is
read out by log_prob over all 2^n indices (probabilities64 / get_probabilities, detached).
Canonical form, bond spectra, compress_ / expand_, the posterior queries and two-site sweeps exist for the real family only
(SampledMPSBornMachine); here each raises a ValueError that says so.
"""
import math

import torch
import torch.nn as nn

from . import backend
from .born_machine_base import bits_to_indices, indices_to_bits

ENUMERATED_MAX_N = 20          # probabilities64: log_prob over all 2^n indices in one call
STATEVECTOR_MAX_N = 16         # from_statevector: sequential SVDs on the host


def _refused(name):
    def method(self, *args, **kwargs):
        raise ValueError(f"{name} is not offered for complex cores: it exists for the real family (SampledMPSBornMachine) only")
    method.__name__ = name
    method.__doc__ = f"Not offered for complex cores (SampledMPSBornMachine has {name})."
    return method


class ComplexSampledMPSBornMachine(nn.Module):
    """MPS Born machine with complex cores whose surface is samples, log q of samples and the score-function gradient."""

    REFUSED = ("bond_spectrum", "bond_entropies", "canonical_cores", "canonicalise_", "compress_", "expand_", "two_site_sweep_",
               "fit_two_site", "marginals", "pair_marginals", "log_marginal", "log_marginal_vjp", "sample_given")

    def __init__(self, num_latent_vars, bond_dim=4, init_method='small_random', conditioning_dim=0, seed=0):
        if conditioning_dim != 0:
            raise ValueError("ComplexSampledMPSBornMachine is not conditional: conditioning_dim must be 0.")
        if isinstance(num_latent_vars, bool) or not isinstance(num_latent_vars, int) or not 1 <= num_latent_vars <= backend.MPS_SAMPLED_MAX_N:
            raise ValueError(f"num_latent_vars must be an integer in 1 ... {backend.MPS_SAMPLED_MAX_N}, got {num_latent_vars!r}")
        if isinstance(bond_dim, bool) or not isinstance(bond_dim, int) or not 1 <= bond_dim <= backend.CMPS_MAX_BOND:
            raise ValueError(f"bond_dim must be an integer in 1 ... {backend.CMPS_MAX_BOND} (complex cores), got {bond_dim!r}")
        if init_method not in ('small_random', 'zero', 'random'):
            raise ValueError(f"init_method must be 'small_random', 'zero' or 'random', got {init_method!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an integer, got {seed!r}")
        super().__init__()
        n, D = num_latent_vars, bond_dim
        eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
        if init_method == 'zero':            # psi(z) = 2^(-n/2) for every z: the exactly uniform q
            re, im = eye / math.sqrt(2.0), torch.zeros(n, 2, D, D, dtype=torch.float64)
        elif init_method == 'small_random':  # the real family's draw for the real parts, a second one of the same scale
            re = (eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / math.sqrt(2.0)
            im = 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(2.0)
        else:                                # the real family's variance 1 / (2 D), split between the parts
            re = torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(4.0 * D)
            im = torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(4.0 * D)
        self.num_latent_vars = n
        self.conditioning_dim = 0
        self.seed = seed
        self._draws = 0            # epoch of the next sample() call: successive calls draw fresh samples
        self.cores = nn.Parameter(torch.stack((re, im), dim=-1).contiguous())

    # ---- constructors from other states ---------------------------------------------------------------------------
    @classmethod
    def _with_cores(cls, cores, seed=0):
        n, D = int(cores.shape[0]), int(cores.shape[2])
        m = cls(n, bond_dim=D, init_method='zero', seed=seed)
        with torch.no_grad():
            m.cores.copy_(cores)
        return m

    @classmethod
    def from_real(cls, machine):
        """The machine of the same psi as a real MPS machine (cores [n, 2, D, D]), imaginary parts 0.0."""
        cores = getattr(machine, "cores", None)
        if not torch.is_tensor(cores) or cores.dim() != 4 or cores.shape[1] != 2 or cores.shape[2] != cores.shape[3]:
            raise ValueError("from_real takes a real MPS machine with cores [n, 2, D, D]")
        if cores.shape[2] > backend.CMPS_MAX_BOND:
            raise ValueError(f"complex cores take a bond dimension of at most {backend.CMPS_MAX_BOND}, got {int(cores.shape[2])}")
        re = cores.detach().to(device="cpu", dtype=torch.float64)
        m = cls._with_cores(torch.stack((re, torch.zeros_like(re)), dim=-1), seed=getattr(machine, "seed", 0))
        return m.to(cores.device)

    @classmethod
    def from_statevector(cls, psi, bond_dim, cutoff=0.0, seed=0):
        """(machine, discarded float64 [n - 1]) from a vector of 2^n amplitudes (complex or real; the outcome index is the
        position, tuple position 0 the most significant bit), n <= 16, by sequential torch.linalg.svd on the CPU, left to
        right.  Exact when bond_dim >= 2^floor(n / 2); otherwise every bond keeps its bond_dim largest singular values, then
        drops more from the small end while the dropped squares' sum stays <= cutoff times the sum of all squares (one
        always stays), and discarded[j] is the sum of the dropped squares at bond j (the tail sum of that SVD)."""
        psi = torch.as_tensor(psi)
        if psi.dim() != 1 or psi.numel() < 2 or psi.numel() & (psi.numel() - 1):
            raise ValueError("from_statevector takes a vector of 2^n amplitudes, n >= 1")
        n = psi.numel().bit_length() - 1
        if n > STATEVECTOR_MAX_N:
            raise ValueError(f"from_statevector takes at most 2^{STATEVECTOR_MAX_N} amplitudes, got 2^{n}")
        if isinstance(bond_dim, bool) or not isinstance(bond_dim, int) or not 1 <= bond_dim <= backend.CMPS_MAX_BOND:
            raise ValueError(f"bond_dim must be an integer in 1 ... {backend.CMPS_MAX_BOND} (complex cores), got {bond_dim!r}")
        if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float)) or not 0 <= cutoff < 1:
            raise ValueError(f"cutoff must be a number in [0, 1), got {cutoff!r}")
        if not (psi.is_complex() or psi.is_floating_point()) or not bool(torch.isfinite(torch.view_as_real(psi.to(torch.complex128))).all()):
            raise ValueError("from_statevector takes finite real or complex amplitudes")
        D = bond_dim
        cores = torch.zeros(n, 2, D, D, dtype=torch.complex128)
        discarded = torch.zeros(max(n - 1, 0), dtype=torch.float64)
        rest = psi.detach().to(device="cpu", dtype=torch.complex128).reshape(1, -1)      # [left bond, remaining bits]
        for k in range(n - 1):
            chi = rest.shape[0]
            U, S, Vh = torch.linalg.svd(rest.reshape(chi * 2, -1), full_matrices=False)
            sq = S * S
            keep = min(D, int(S.numel()))
            total = float(sq.sum())
            while keep > 1 and float(sq[keep - 1:].sum()) <= cutoff * total:
                keep -= 1
            discarded[k] = sq[keep:].sum()
            cores[k, :, :chi, :keep] = U[:, :keep].reshape(chi, 2, keep).permute(1, 0, 2)
            rest = S[:keep, None] * Vh[:keep]
        cores[n - 1, :, :rest.shape[0], 0] = rest.reshape(rest.shape[0], 2).permute(1, 0)
        return cls._with_cores(torch.view_as_real(cores), seed=seed), discarded

    # ---- the parameter ---------------------------------------------------------------------------------------------
    @property
    def bond_dim(self):
        return int(self.cores.shape[2])

    @property
    def num_parameters(self):
        return self.cores.numel()

    @property
    def complex_cores(self):
        """complex128 [n, 2, D, D]: a view of the parameter (detached)."""
        return torch.view_as_complex(self.cores.detach())

    def kernel_input(self):
        """(cores detached as a contiguous float64 [n, 2, D, D, 2] tensor on the compute device, the parameter's own device)."""
        home = self.cores.device
        return self.cores.detach().to(device=backend.compute_device(home), dtype=torch.float64).contiguous(), home

    # ---- the three calls a trainer needs (SampledMPSBornMachine has the same three) --------------------------------------
    def environments(self, cores, num_samples):
        return backend.cmps_environments(cores, num_samples)

    def draw(self, cores, num_samples, seed, epoch_dev):
        return backend.cmps_sample(cores, num_samples, seed, epoch_dev)

    def score_gradient(self, cores, idx, w):
        return backend.cmps_score_vjp(cores, idx, w)

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
        """(grad float64 [n, 2, D, D, 2] = the gradient of sum_b w_b log q(idx_b) in the parameter, logq float64 [B]) on the
        compute device."""
        cores, _ = self.kernel_input()
        idx = idx.to(device=cores.device, dtype=torch.int64).contiguous()
        w = w.to(device=cores.device, dtype=torch.float64).contiguous()
        self.environments(cores, int(idx.numel()))
        grad, logq, _ = self.score_gradient(cores, idx, w)
        return grad, logq

    def log_prob(self, idx):
        """log q(idx), float64 [B] (-inf where psi is 0)."""
        idx = idx.reshape(-1)
        return self.score_vjp(idx, torch.zeros(idx.numel(), dtype=torch.float64, device=idx.device))[1]

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


for _name in ComplexSampledMPSBornMachine.REFUSED:
    setattr(ComplexSampledMPSBornMachine, _name, _refused(_name))
del _name
