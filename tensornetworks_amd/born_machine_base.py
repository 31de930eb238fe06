"""What the classical Born-machine families have in common: the table / MLP machine (born_machine_classical_sim.py), the MPS
machine (born_machine_mps.py) and the sampled MPS machine (born_machine_mps_sampled.py).

  indices_to_bits / bits_to_indices   outcome index <-> bit row (tuple position 0 = the most significant bit), with the
                                      validation of bit rows and its message; exact up to n = 63 (shifts reach 1 << 62)
  pack_evidence                       a partial assignment {position: value} -> the (mask, value) words of the sampled MPS's
                                      queries, in the same bit layout
  EnumeratedBornMachine               the surface over the 2^n table of q that the classical trainers use: fixed
                                      probabilities, all_outcome_tuples, sample, get_prob_dict, get_log_q_z_x, entropy.
                                      A family supplies how q is computed (_probabilities, _entropy) and its two ends of a
                                      training epoch: epoch_forward -> EpochForward, epoch_backward -> (loss, grads)
  new_mps_cores / MPSCores            the MPS families' constructor checks, initialisations and move to the compute device
                                      and, on MPSCores, the canonical-form surface: bond_spectrum,
                                      bond_entropies, canonical_cores, canonicalise_, compress_, expand_
"""
import math
from typing import Any, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import backend
from .utils import generate_all_binary_outcomes


def indices_to_bits(idx, n):
    """float32 bit rows [..., n] of int64 outcome indices [...]."""
    shifts = torch.arange(n - 1, -1, -1, device=idx.device)
    return ((idx.unsqueeze(-1) >> shifts) & 1).to(torch.float32)


def bits_to_indices(z_samples, n, device=None):
    """int64 outcome indices [B] (on `device`; default: where the rows are) of bit rows [B, n].  `.long()` truncates like
    the reference's; a row with an entry other than 0 or 1, or an input that is not [B, n], raises."""
    z = z_samples.detach().to(device=device).long()
    row = None
    if z.dim() != 2 or z.shape[1] != n:
        row = z[0] if z.dim() >= 2 else z.reshape(-1)
    else:
        bad = ((z != 0) & (z != 1)).any(dim=1)
        if bool(bad.any()):
            row = z[int(torch.nonzero(bad)[0])]
    if row is not None:
        raise ValueError(f"Sample {tuple(row.tolist())} is not a valid outcome.")
    return (z << torch.arange(n - 1, -1, -1, device=z.device)).sum(dim=1)


MAX_EVIDENCE_QUERIES = backend.MPS_QUERY_MAX_QUERIES      # what one bornvi_mps_log_marginals call takes


def pack_evidence(evidence, n):
    """(mask, value): int64 tensors [Q] of the evidence words of the sampled MPS's queries, in the outcome index's own layout:
    tuple position p is bit n - 1 - p; a set mask bit clamps that position to the value's bit.  `evidence` is a dict
    {position: 0 or 1} (Q = 1), a non-empty sequence of such dicts, or a (mask, value) pair of int64 tensors (kept where
    they are; checked where the host can see them: on the CPU).  Every error is a ValueError raised on the host."""
    if isinstance(evidence, (tuple, list)) and len(evidence) == 2 and all(torch.is_tensor(e) for e in evidence):
        mask, value = evidence
        if mask.dtype != torch.int64 or value.dtype != torch.int64 or mask.shape != value.shape or mask.dim() > 1:
            raise ValueError("evidence (mask, value): two int64 tensors of one shape [Q]")
        mask, value = mask.reshape(-1), value.reshape(-1)
        if not 1 <= mask.numel() <= MAX_EVIDENCE_QUERIES:
            raise ValueError(f"evidence: 1 ... 2^16 queries per call, got {mask.numel()}")
        if mask.device.type == "cpu" and bool((((mask | value) >> n) != 0).any()):
            raise ValueError(f"evidence (mask, value): bits at or above n = {n} must be 0")
        return mask.contiguous(), value.contiguous()
    queries = [evidence] if isinstance(evidence, dict) else evidence
    if isinstance(queries, (str, bytes)) or not hasattr(queries, "__len__") or not hasattr(queries, "__iter__"):
        raise ValueError(f"evidence: a dict {{position: 0 or 1}}, a sequence of such dicts or a (mask, value) pair, got {evidence!r}")
    if not 1 <= len(queries) <= MAX_EVIDENCE_QUERIES:
        raise ValueError(f"evidence: 1 ... 2^16 queries per call, got {len(queries)}")
    masks, values = [], []
    for q in queries:
        if not isinstance(q, dict):
            raise ValueError(f"evidence: every query is a dict {{position: 0 or 1}}, got {q!r}")
        m = v = 0
        for pos, val in q.items():
            if isinstance(pos, bool) or not isinstance(pos, (int, np.integer)) or not 0 <= int(pos) < n:
                raise ValueError(f"evidence: position {pos!r} is outside 0 ... {n - 1}")
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or int(val) not in (0, 1):
                raise ValueError(f"evidence: the value at position {pos!r} must be 0 or 1, got {val!r}")
            m |= 1 << (n - 1 - int(pos))
            v |= int(val) << (n - 1 - int(pos))
        masks.append(m)
        values.append(v)
    return torch.tensor(masks, dtype=torch.int64), torch.tensor(values, dtype=torch.int64)


class EpochForward(NamedTuple):
    """What a family's epoch_forward hands the trainer, and the trainer hands back to epoch_backward."""
    q32: torch.Tensor                   # [2^n] float32
    q64: torch.Tensor                   # [2^n] float64, on the compute device: what the objective contracts
    entropy: Optional[torch.Tensor]     # [1] = -sum q log max(q, 1e-10), or None when not asked for
    state: Any                          # the family's own: what its backward needs


class EnumeratedBornMachine(nn.Module):
    """Born machine whose q is a table over the 2^n latent states."""
    draws_in_forward = False            # True: a forward draws random numbers (Dropout), so two forwards differ

    def __init__(self, num_latent_vars, conditioning_dim=0):
        super().__init__()
        self.num_latent_vars = num_latent_vars
        self.num_outcomes = 2 ** num_latent_vars
        self.conditioning_dim = conditioning_dim
        self._fixed_probs = None
        self._use_fixed_probs = False
        self._outcomes = None

    # ---- what a family supplies ------------------------------------------------------------------------------
    def _probabilities(self, x_condition):
        """float32 [B, 2^n] on the parameters' device, differentiable."""
        raise NotImplementedError

    def _entropy(self, x_condition):
        raise NotImplementedError

    def epoch_forward(self, x_condition, want_entropy):
        """-> EpochForward of the current parameters; nothing is read back to the host."""
        raise NotImplementedError

    def epoch_backward(self, fwd, y, ksd2=None, entropy_weight=0.0):
        """(loss, grads) of L = sqrt(max(ksd2, 1e-12)) - entropy_weight * H with y = K_p q (no gradient below the clamp),
        or, with ksd2 = None, of a loss whose dL/dq is y (loss = None): backend.born_table_vjp's arguments.  grads =
        [(tensor, its gradient), ...] for the trainers' apply_grads."""
        raise NotImplementedError

    # ---- the shared surface --------------------------------------------------------------------------------------
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

    def get_probabilities(self, x_condition=None):
        """float32 [B, 2^n] ([1, 2^n] unconditioned), differentiable; the fixed probabilities when set."""
        if self._use_fixed_probs and self._fixed_probs is not None:
            return self._fixed_probs.unsqueeze(0) if self._fixed_probs.ndim == 1 else self._fixed_probs
        return self._probabilities(x_condition)

    def sample(self, num_samples=1, x_condition=None):
        """float32 bit rows [num, n], or [B, num, n] for a batch of conditions."""
        probs = self.get_probabilities(x_condition).detach()
        probs = probs + 1e-10
        probs = probs / probs.sum(dim=-1, keepdim=True)
        batched = probs.shape[0] > 1 or (x_condition is not None and x_condition.ndim > 1)
        bits = indices_to_bits(torch.multinomial(probs, num_samples, replacement=True), self.num_latent_vars)
        return bits if batched else bits[0]

    def get_prob_dict(self, x_condition=None):
        """{outcome tuple: probability} of a single distribution."""
        probs_tensor = self.get_probabilities(x_condition)
        if probs_tensor.shape[0] > 1 and not (probs_tensor.ndim == 1 and self.conditioning_dim == 0):
            raise ValueError("get_prob_dict is for a single distribution.")
        probs_1d = probs_tensor.squeeze().detach().cpu().numpy().reshape(-1)
        return dict(zip(self.all_outcome_tuples, probs_1d))

    def get_log_q_z_x(self, z_samples, x_condition=None):
        """log max(q(z|x), 1e-10) for a batch of bit rows: one x for all rows, or one per row."""
        if self.conditioning_dim > 0 and x_condition is None:
            raise ValueError("x_condition must be provided for conditional Born machine.")
        if self.conditioning_dim == 0 and x_condition is not None:
            raise ValueError("x_condition provided but Born machine is not conditional.")
        probs = self.get_probabilities(x_condition)
        log_probs = torch.log(probs.clamp(min=1e-10))
        bz, bx = z_samples.shape[0], probs.shape[0]
        if bx != 1 and bx != bz:
            raise ValueError(f"Batch size mismatch: x_condition ({bx}) vs z_samples ({bz}).")
        idx = bits_to_indices(z_samples, self.num_latent_vars, log_probs.device)
        if bx == 1:
            return log_probs[0, idx]
        return log_probs[torch.arange(bz, device=idx.device), idx]

    def entropy(self, x_condition=None):
        """-sum q log max(q, 1e-10) (a forward of its own, as in the reference), differentiable."""
        if self._use_fixed_probs and self._fixed_probs is not None:
            probs = self.get_probabilities(x_condition).squeeze()
            return -(probs * torch.log(probs.clamp(min=1e-10))).sum()
        return self._entropy(x_condition)


def new_mps_cores(owner, num_latent_vars, bond_dim, init_method, conditioning_dim, max_n):
    """The float64 parameter [n, 2, D, D] of an MPS machine after its constructor checks (`owner`: the class name in the
    messages).  'small_random' and 'random' make one torch.randn(n, 2, D, D, dtype=float64) draw, 'zero' none."""
    if conditioning_dim != 0:
        raise ValueError(f"{owner} is not conditional: conditioning_dim must be 0.")
    if isinstance(num_latent_vars, bool) or not isinstance(num_latent_vars, int) or not 1 <= num_latent_vars <= max_n:
        raise ValueError(f"num_latent_vars must be an integer in 1 ... {max_n}, got {num_latent_vars!r}")
    if isinstance(bond_dim, bool) or not isinstance(bond_dim, int) or not 1 <= bond_dim <= backend.MPS_MAX_BOND:
        raise ValueError(f"bond_dim must be an integer in 1 ... {backend.MPS_MAX_BOND}, got {bond_dim!r}")
    if init_method not in ('small_random', 'zero', 'random'):
        raise ValueError(f"init_method must be 'small_random', 'zero' or 'random', got {init_method!r}")
    n, D = num_latent_vars, bond_dim
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    if init_method == 'zero':            # psi(z) = 2^(-n/2) for every z: the exactly uniform q
        init = eye / math.sqrt(2.0)
    elif init_method == 'small_random':
        init = (eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / math.sqrt(2.0)
    else:
        init = torch.randn(n, 2, D, D, dtype=torch.float64) / math.sqrt(2.0 * D)
    return nn.Parameter(init.clone().contiguous())


class MPSCores:
    """Mixin of the two MPS machines: `cores` [n, 2, D, D] float64 (from new_mps_cores) and its way to the kernels."""

    @property
    def bond_dim(self):
        return int(self.cores.shape[2])

    @property
    def num_parameters(self):
        return self.cores.numel()

    def kernel_input(self, detach=False):
        """(cores as a contiguous float64 tensor on the compute device -- differentiable unless detach --, the parameter's
        own device)."""
        home = self.cores.device
        cores = self.cores.detach() if detach else self.cores
        return cores.to(device=backend.compute_device(home), dtype=torch.float64).contiguous(), home

    # ---- canonical form, bond spectra, truncation and growth (backend.mps_canonicalise) ----------
    # Everything returned is detached and on the compute device; every argument error is raised before any GPU call.
    @staticmethod
    def _check_cut(bond_dim, cutoff, D):
        if bond_dim is not None and (isinstance(bond_dim, bool) or not isinstance(bond_dim, int) or not 1 <= bond_dim <= D):
            raise ValueError(f"bond_dim must be None or an integer in 1 ... {D} (the current bond dimension), got {bond_dim!r}")
        if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float)) or not math.isfinite(cutoff) or cutoff < 0:
            raise ValueError(f"cutoff must be a finite number >= 0, got {cutoff!r}")

    def _canonical(self, bond_dim, cutoff):
        self._check_cut(bond_dim, cutoff, self.bond_dim)
        out, schmidt, discarded, rank, log_norm, status = backend.mps_canonicalise(MPSCores.kernel_input(self, detach=True)[0], bond_dim,
                                                                                  float(cutoff))
        return out, schmidt, {"rank": rank, "discarded": discarded, "log_norm": log_norm, "status": status}

    def bond_spectrum(self):
        """float64 [n - 1, D]: the Schmidt values of every bond of the current cores, descending, zero-padded; the squares
        of a bond sum to 1.  A value the factorisation's rank rule found null is exactly 0.0."""
        return self._canonical(None, 0.0)[1]

    def bond_entropies(self):
        """float64 [n - 1]: -sum s^2 log s^2 over a bond's Schmidt values, a zero value contributing 0."""
        p = self.bond_spectrum() ** 2
        return -(p * torch.log(torch.where(p > 0, p, torch.ones_like(p)))).sum(dim=1)

    def canonical_cores(self, bond_dim=None, cutoff=0.0):
        """(cores_out float64 [n, 2, D', D'], report) with D' = bond_dim (default: the current D): the same q in canonical
        form (sites 2 .. n right-canonical, Z = 1), each bond cut to its bond_dim largest Schmidt values and then further
        from the small end while the dropped squares sum to <= cutoff.  report = {'rank' int32 [n - 1], 'discarded' float64
        [n - 1], 'log_norm' float64 [1] (log Z of the current cores), 'status' int32 [1]: 0, 1 (non-finite cores or Z) or 4
        (a factorisation did not converge)}.  The machine is not changed."""
        out, _, report = self._canonical(bond_dim, cutoff)
        return out, report

    def canonicalise_(self):
        """Replaces the parameter's data by its canonical form, in place (the same nn.Parameter, the same D): q is unchanged,
        Z = 1.  Returns canonical_cores' report."""
        out, _, report = self._canonical(None, 0.0)
        with torch.no_grad():
            self.cores.data.copy_(out.to(device=self.cores.device, dtype=self.cores.dtype))
        return report

    def compress_(self, bond_dim=None, cutoff=0.0):
        """Cuts the bonds as canonical_cores does and makes `cores` a NEW nn.Parameter [n, 2, D', D']: D' = bond_dim when
        given (at most the current D; D itself cuts by `cutoff` alone), else the largest kept rank.  Returns the report.  An optimiser built on the
        old parameter is stale: build a new one (the trainers build theirs inside train(), so train -> compress_ -> train
        works as it stands).  The same holds after SampledMPSBornMachine.two_site_sweep_ / fit_two_site and
        AmortisedMPSInference.train_two_site, which keep the parameter but rewrite its data in another gauge: the Adam moments
        of an optimiser built earlier mean nothing afterwards."""
        out, _, report = self._canonical(bond_dim, cutoff)
        if bond_dim is None:
            rank = report["rank"]
            bond_dim = int(rank.max().item()) if rank.numel() else 1
        new = out[:, :, :bond_dim, :bond_dim].contiguous()
        self.cores = nn.Parameter(new.to(device=self.cores.device, dtype=self.cores.dtype))
        return report

    def expand_(self, bond_dim, noise=0.0, seed=0):
        """Grows the bond dimension to bond_dim (current D < bond_dim <= 32) on the host: `cores` becomes a NEW nn.Parameter
        whose leading [D, D] blocks are the old cores and whose other entries are noise * torch.randn of a CPU generator
        seeded by seed -- except the first core's rows >= 1 and the last core's columns >= 1, which stay 0.  With noise =
        0.0 psi is unchanged as a function.  As after compress_, an optimiser built on the old parameter is stale."""
        D, n = self.bond_dim, int(self.cores.shape[0])
        if isinstance(bond_dim, bool) or not isinstance(bond_dim, int) or not D < bond_dim <= backend.MPS_MAX_BOND:
            raise ValueError(f"expand_: bond_dim must be an integer in {D + 1} ... {backend.MPS_MAX_BOND}, got {bond_dim!r}")
        if isinstance(noise, bool) or not isinstance(noise, (int, float)) or not math.isfinite(noise) or noise < 0:
            raise ValueError(f"noise must be a finite number >= 0, got {noise!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an integer, got {seed!r}")
        new = torch.zeros(n, 2, bond_dim, bond_dim, dtype=torch.float64)
        new[:, :, :D, :D] = self.cores.detach().to(device="cpu", dtype=torch.float64)
        if noise != 0.0:
            gen = torch.Generator().manual_seed(seed)
            fresh = torch.ones(n, 2, bond_dim, bond_dim, dtype=torch.bool)
            fresh[:, :, :D, :D] = False
            fresh[0, :, 1:, :] = False
            fresh[n - 1, :, :, 1:] = False
            new = new + noise * torch.randn(n, 2, bond_dim, bond_dim, dtype=torch.float64, generator=gen) * fresh
        self.cores = nn.Parameter(new.to(device=self.cores.device, dtype=self.cores.dtype).contiguous())
