"""Matrix-product-state Born machine through samples only: the family of born_machine_mps.py without any 2^n object.

  q(z) = psi(z)^2 / Z,   psi(z) = e0^T A_1[z_1] ... A_n[z_n] e0,   cores float64 [n, 2, D, D],   1 <= n <= 63

An exact draw z ~ q costs O(n D^2) (ancestral sampling against the right environments), and so do log q(z) and
grad log q(z) for a given z (bornvi_mps_environments / bornvi_mps_sample / bornvi_mps_score_vjp).
A sample is an int64 outcome index, idx = sum_k z_k 2^(n-k) (tuple position 0 = the most significant bit), or a float32
bit row; the conversion, like the `cores` parameter, its checks, initialisations and messages, is born_machine_base's, shared
with MPSBornMachine.  The sample surface (sample_indices, score_vjp, log_prob, sample, ...) is born_machine_sampled's
SampledSurface, shared with the complex-cores and the locally purified family: this file states the three hooks it goes
through (environments, draw, score_gradient) and what the real family alone has.  The fitted q is read out exactly, at any n, by marginals / pair_marginals / log_marginal / sample_given (DESIGN.md section
6l): an evidence is a partial assignment {tuple position: 0 or 1}.
two_site_sweep_ / fit_two_site train the cores on given samples by two-site (DMRG-style) sweeps that set every bond's rank from
its spectrum.
For n <= 26 the enumerated q is still there (probabilities64 / get_probabilities, through
backend.mps_probs); above that those raise.
"""
import math

import torch
import torch.nn as nn

from . import backend
from .born_machine_base import MPSCores, new_mps_cores, pack_evidence
from .born_machine_mps import _MPSProbs
from .born_machine_sampled import SampledSurface, checked_seed


def append_sweep(history, report):
    """One two-site sweep's report appended to a history {'loss', 'bond_loss', 'rank', 'discarded', 'status'} of lists: the
    sweep's one read-back."""
    loss = report["loss"].cpu().tolist()
    history["loss"].append(loss[-1])
    history["bond_loss"].append(loss)
    history["rank"].append(report["rank"].cpu().tolist())
    history["discarded"].append(report["discarded"].cpu().tolist())
    history["status"].append(int(report["status"].item()))


class SampledMPSBornMachine(SampledSurface, MPSCores, nn.Module):
    """MPS Born machine whose surface is samples, log q of samples and the score-function gradient."""
    ENUMERATED_MAX_N = backend.MPS_MAX_N       # probabilities64: backend.mps_probs
    NATURAL_GRADIENT = True

    def __init__(self, num_latent_vars, bond_dim=4, init_method='small_random', conditioning_dim=0, seed=0):
        cores = new_mps_cores("SampledMPSBornMachine", num_latent_vars, bond_dim, init_method, conditioning_dim,
                              backend.MPS_SAMPLED_MAX_N)
        checked_seed(seed)
        super().__init__()
        self._init_sampled(num_latent_vars, seed)
        self.cores = cores

    # ---- the three calls the shared surface and a trainer need -----------------------------------------------------------
    def environments(self, cores, num_samples):
        return backend.mps_environments(cores, num_samples)

    def draw(self, cores, num_samples, seed, epoch_dev):
        return backend.mps_sample(cores, num_samples, seed, epoch_dev)

    def score_gradient(self, cores, idx, w):
        return backend.mps_score_vjp(cores, idx, w)

    # ---- two-site sweeps (backend.mps_twosite_sweep): bond ranks set by the data -------------------
    def _samples_as_indices(self, idx_or_bits):
        """int64 [B] outcome indices of an index vector or of [B, n] rows of 0 / 1, on the host's side of any GPU call."""
        x = torch.as_tensor(idx_or_bits)
        if x.dim() == 2:
            return self.indices_of(x)
        if x.dim() != 1 or x.dtype not in (torch.int64, torch.int32):
            raise ValueError("samples: an integer index vector [B] or [B, n] rows of 0 / 1")
        x = x.to(torch.int64)
        n = self.num_latent_vars
        if x.numel() and (int(x.min()) < 0 or (n < 63 and int(x.max()) >= (1 << n))):
            raise ValueError(f"samples: an outcome index lies outside 0 ... 2^{n} - 1")
        return x

    def _check_two_site(self, num, weights, lr, steps, cutoff, max_rank):
        D = self.bond_dim
        if self.num_latent_vars < 2:
            raise ValueError("two-site sweeps need at least two sites")
        if D > backend.MPS_TWOSITE_MAX_BOND:
            raise ValueError(f"two-site sweeps take a bond dimension of at most {backend.MPS_TWOSITE_MAX_BOND}, got {D}")
        if not 1 <= num <= backend.MPS_TWOSITE_MAX_BATCH:
            raise ValueError(f"two-site sweeps take 1 ... 2^20 samples, got {num}")
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not math.isfinite(lr) or lr < 0:
            raise ValueError(f"lr must be a finite number >= 0, got {lr!r}")
        if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= backend.MPS_TWOSITE_MAX_STEPS:
            raise ValueError(f"steps must be an integer in 1 ... {backend.MPS_TWOSITE_MAX_STEPS}, got {steps!r}")
        self._check_cut(max_rank, cutoff, D)
        if not cutoff < 1:
            raise ValueError(f"cutoff must be < 1, got {cutoff!r}")
        if weights is not None:
            w = torch.as_tensor(weights)
            if w.dim() != 1 or w.numel() != num or not w.dtype.is_floating_point or bool((w < 0).any()) \
                    or not bool(torch.isfinite(w).all()):
                raise ValueError(f"weights: {num} finite numbers >= 0, one per sample")

    def two_site_sweep_(self, idx_or_bits, weights=None, lr=0.05, steps=5, cutoff=1e-4, max_rank=None, canonicalise=True):
        """One round trip of two-site (DMRG-style) updates on the given samples, in place: every pair of neighbouring cores
        is merged, takes `steps` plain descent steps of size lr on the samples' weighted negative log-likelihood, and is
        split again by an SVD that keeps at most max_rank (default: the bond dimension) values and drops from the small end
        while the dropped squares sum to <= cutoff.  Each bond so takes the rank the data supports, inside the fixed
        [n, 2, D, D] storage (compress_ shrinks it, expand_ raises the cap).  canonicalise: bring the cores to canonical form
        first (canonicalise_()); pass False only for cores a sweep or canonicalise_() has just written.  Returns
        {'loss' float64 [2 (n - 1)] (per bond visited), 'schmidt' float64 [n - 1, D], 'discarded' float64 [n - 1], 'rank'
        int32 [n - 1], 'status' int32 [1]}, detached, on the compute device.  Like compress_, a sweep rewrites the cores in
        another gauge: the Adam moments of an optimiser built earlier mean nothing afterwards; build a new one."""
        idx = self._samples_as_indices(idx_or_bits)
        self._check_two_site(int(idx.numel()), weights, lr, steps, cutoff, max_rank)
        if canonicalise:
            self.canonicalise_()
        cores, home = MPSCores.kernel_input(self, detach=True)
        if cores.data_ptr() == self.cores.data_ptr():
            cores = cores.clone()
        dev = cores.device
        idx = idx.to(device=dev, dtype=torch.int64).contiguous()
        w = None if weights is None else torch.as_tensor(weights).to(device=dev, dtype=torch.float64).contiguous()
        loss, schmidt, discarded, rank, status = backend.mps_twosite_sweep(cores, idx, w, float(lr), steps, max_rank, float(cutoff))
        with torch.no_grad():
            self.cores.data.copy_(cores.to(device=home, dtype=self.cores.dtype))
        return {"loss": loss, "schmidt": schmidt, "discarded": discarded, "rank": rank, "status": status}

    def fit_two_site(self, data, num_sweeps, weights=None, lr=0.05, steps=5, cutoff=1e-4, max_rank=None):
        """Maximum-likelihood training on a data set by two-site sweeps: data is [B, n] rows of 0 / 1 or an index vector [B];
        num_sweeps round trips of two_site_sweep_ on it (the first from the canonical form of the current cores).  Returns the
        history {'loss' (the last bond's, per sweep), 'bond_loss', 'rank', 'discarded', 'status'}: lists of num_sweeps entries."""
        if isinstance(num_sweeps, bool) or not isinstance(num_sweeps, int) or num_sweeps < 1:
            raise ValueError(f"num_sweeps must be a positive integer, got {num_sweeps!r}")
        idx = self._samples_as_indices(data)
        self._check_two_site(int(idx.numel()), weights, lr, steps, cutoff, max_rank)
        history = {"loss": [], "bond_loss": [], "rank": [], "discarded": [], "status": []}
        for _ in range(num_sweeps):
            append_sweep(history, self.two_site_sweep_(idx, weights, lr, steps, cutoff, max_rank))
        return history

    # ---- exact queries: detached, on the compute device -----------------------------------
    def _evidence(self, evidence, single=False):
        """(mask, value) int64 [Q] on the compute device; every argument error is raised before any GPU call."""
        mask, value = pack_evidence(evidence, self.num_latent_vars)
        if single and mask.numel() != 1:
            raise ValueError(f"sample_given takes one evidence, got {mask.numel()}")
        dev = backend.compute_device(self.cores.device)
        return mask.to(dev), value.to(dev)

    def marginals(self):
        """float64 [n]: q(z_k = 1), exact."""
        return backend.mps_marginals(self.kernel_input()[0])[0]

    def pair_marginals(self):
        """(float64 [n], float64 [n, n]): q(z_i = 1) and q(z_i = 1, z_j = 1), exact; the matrix is symmetric bit for bit and
        its diagonal is the first result."""
        return backend.mps_marginals(self.kernel_input()[0], want_pairs=True)

    def log_marginal(self, evidence):
        """float64 [Q]: the log probability of each partial assignment (-inf where it is impossible under q).  evidence: a
        dict {position: 0 or 1}, a sequence of such dicts (at most 2^16), or a (mask, value) pair of int64 tensors."""
        mask, value = self._evidence(evidence)
        return backend.mps_log_marginals(self.kernel_input()[0], mask, value)[0]

    def log_marginal_vjp(self, evidence, weights):
        """(grad float64 [n, 2, D, D] = sum_j weights_j grad log q(evidence_j), logm float64 [Q]) on the compute device: the
        counterpart of score_vjp for partial assignments.  evidence as log_marginal takes it; an
        impossible evidence contributes nothing and has logm -inf."""
        mask, value = self._evidence(evidence)
        cores, _ = self.kernel_input()
        if not torch.is_tensor(weights) or weights.numel() != mask.numel():
            raise ValueError(f"weights: a tensor of {mask.numel()} numbers, one per evidence")
        w = weights.reshape(-1).to(device=cores.device, dtype=torch.float64).contiguous()
        grad, logm, _ = backend.mps_log_marginals_vjp(cores, mask, value, w)
        return grad, logm

    def sample_given(self, evidence, num_samples, seed=None, epoch=0):
        """(idx int64 [num], logq_cond float64 [num] = log q(idx | evidence), log_marginal float64 [1] of the evidence):
        exact draws from q(. | evidence).  A pure function of (cores, evidence, seed, epoch); a free position gets the
        uniform it gets in sample_indices."""
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
            raise ValueError(f"num_samples must be a positive integer, got {num_samples!r}")
        if isinstance(epoch, bool) or not isinstance(epoch, int):
            raise ValueError(f"epoch must be an integer, got {epoch!r}")
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
            raise ValueError(f"seed must be an integer, got {seed!r}")
        mask, value = self._evidence(evidence, single=True)
        cores, _ = self.kernel_input()
        ep = torch.tensor([epoch], dtype=torch.int64, device=cores.device)
        idx, logq, logm, _ = backend.mps_sample_clamped(cores, num_samples, mask, value, self.seed if seed is None else seed, ep)
        return idx, logq, logm

    # ---- the enumerated distribution, where it exists ------------------------------------------------------------
    def probabilities64(self, x_condition=None):
        """float64 [2^n], differentiable (n <= 26): backend.mps_probs, as MPSBornMachine."""
        self._check_enumerated(x_condition)
        cores, home = MPSCores.kernel_input(self)
        return _MPSProbs.apply(cores).to(home)
