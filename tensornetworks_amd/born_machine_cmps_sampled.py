"""Matrix-product-state Born machine with COMPLEX cores, through samples only: the classical
counterpart of a QuantumBornMachine state, and a strictly larger family than born_machine_mps_sampled.py's at the same bond.

  cores float64 [n, 2, D, D, 2], (re, im) last: torch.view_as_real of a complex128 [n, 2, D, D];  A_k[s] = X + iY
  psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0 in C (a plain product, no conjugate),  q(z) = |psi(z)|^2 / Z,  Z = sum_z |psi(z)|^2
  1 <= n <= 63, 1 <= D <= 16;  bit order, index word and boundary vectors as in the real family.

The training surface is born_machine_sampled's SampledSurface, the one SampledMPSBornMachine has: kernel_input,
sample_indices, score_vjp, log_prob, bits_of, indices_of, sample, get_log_q_z_x, num_parameters, bond_dim, through this
file's three hooks (bornvi_cmps_environments / _sample / _score_vjp).  The gradient is that of
the real function in the 2 . 2 n D^2 real numbers of `cores`: what a torch optimiser steps.  For n <= 20 the enumerated q is
read out by log_prob over all 2^n indices (probabilities64 / get_probabilities, detached).
Canonical form, bond spectra, compress_ / expand_, the posterior queries and two-site sweeps exist for the real family only
(SampledMPSBornMachine); here each raises a ValueError that says so.
"""
import math

import torch
import torch.nn as nn

from . import backend
from .born_machine_sampled import SampledSurface, checked_init_method, checked_int, checked_seed, refuse

ENUMERATED_MAX_N = SampledSurface.ENUMERATED_MAX_N          # probabilities64: log_prob over all 2^n indices in one call
STATEVECTOR_MAX_N = 16         # from_statevector: sequential SVDs on the host


@refuse
class ComplexSampledMPSBornMachine(SampledSurface, nn.Module):
    """MPS Born machine with complex cores whose surface is samples, log q of samples and the score-function gradient."""
    CORES = "complex cores"

    def __init__(self, num_latent_vars, bond_dim=4, init_method='small_random', conditioning_dim=0, seed=0):
        if conditioning_dim != 0:
            raise ValueError("ComplexSampledMPSBornMachine is not conditional: conditioning_dim must be 0.")
        n = checked_int(num_latent_vars, 1, backend.MPS_SAMPLED_MAX_N, "num_latent_vars")
        D = checked_int(bond_dim, 1, backend.CMPS_MAX_BOND, "bond_dim", " (complex cores)")
        checked_init_method(init_method)
        checked_seed(seed)
        super().__init__()
        eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
        if init_method == 'zero':            # psi(z) = 2^(-n/2) for every z: the exactly uniform q
            re, im = eye / math.sqrt(2.0), torch.zeros(n, 2, D, D, dtype=torch.float64)
        elif init_method == 'small_random':  # the real family's draw for the real parts, a second one of the same scale
            re = (eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / math.sqrt(2.0)
            im = 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(2.0)
        else:                                # the real family's variance 1 / (2 D), split between the parts
            re = torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(4.0 * D)
            im = torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(4.0 * D)
        self._init_sampled(n, seed)
        self.cores = nn.Parameter(torch.stack((re, im), dim=-1).contiguous())

    # ---- constructors from other states ---------------------------------------------------------------------------
    @classmethod
    def from_real(cls, machine):
        """The machine of the same psi as a real MPS machine (cores [n, 2, D, D]), imaginary parts 0.0."""
        cores = getattr(machine, "cores", None)
        if not torch.is_tensor(cores) or cores.dim() != 4 or cores.shape[1] != 2 or cores.shape[2] != cores.shape[3]:
            raise ValueError("from_real takes a real MPS machine with cores [n, 2, D, D]")
        if cores.shape[2] > backend.CMPS_MAX_BOND:
            raise ValueError(f"complex cores take a bond dimension of at most {backend.CMPS_MAX_BOND}, got {int(cores.shape[2])}")
        re = cores.detach().to(device="cpu", dtype=torch.float64)
        m = cls._with_cores(torch.stack((re, torch.zeros_like(re)), dim=-1), seed=getattr(machine, "seed", 0), bond_dim=int(re.shape[2]))
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
        D = checked_int(bond_dim, 1, backend.CMPS_MAX_BOND, "bond_dim", " (complex cores)")
        if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float)) or not 0 <= cutoff < 1:
            raise ValueError(f"cutoff must be a number in [0, 1), got {cutoff!r}")
        if not (psi.is_complex() or psi.is_floating_point()) or not bool(torch.isfinite(torch.view_as_real(psi.to(torch.complex128))).all()):
            raise ValueError("from_statevector takes finite real or complex amplitudes")
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
        return cls._with_cores(torch.view_as_real(cores), seed=seed, bond_dim=D), discarded

    @property
    def complex_cores(self):
        """complex128 [n, 2, D, D]: a view of the parameter (detached)."""
        return torch.view_as_complex(self.cores.detach())

    # ---- the three calls the shared surface and a trainer need -----------------------------------------------------------
    def environments(self, cores, num_samples):
        return backend.cmps_environments(cores, num_samples)

    def draw(self, cores, num_samples, seed, epoch_dev):
        return backend.cmps_sample(cores, num_samples, seed, epoch_dev)

    def score_gradient(self, cores, idx, w):
        return backend.cmps_score_vjp(cores, idx, w)
