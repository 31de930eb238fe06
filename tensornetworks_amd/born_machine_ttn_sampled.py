"""Born machine on a binary TREE TENSOR NETWORK, through samples only (Cheng et al. 2019): any two of
the n variables are 2 ceil(log2 n) bonds apart, where a chain carries them through |i - j|.

  h = max(1, ceil(log2 n)), L = 2^h leaf positions; position j < n holds tuple position j, positions j >= n are padding (value 0)
  nodes v = 1 .. L - 1 (heap numbering, children 2 v and 2 v + 1; the children of a bottom node v >= L / 2 are positions)
  cores float64 [L - 1, D, D, D]: cores[v - 1] = T_v[p, a, b], p the parent bond, a, b the child bonds; a leaf is e_z in R^D
  x_v[p] = sum_{a,b} T_v[p, a, b] x_{2v}[a] x_{2v+1}[b],  psi(z) = x_1[0],  q(z) = psi(z)^2 / Z,  Z = sum_z psi(z)^2
  1 <= n <= 63, 2 <= D <= 8;  bit order and index word as in the real family.
  Dead entries (never read, initialised 0.0, gradient exactly 0.0): the root at p >= 1, a bottom node at a >= 2 or b >= 2 or at
  the value 1 of a padding child.  live_mask() is the others; num_parameters counts them.

The training surface is born_machine_sampled's SampledSurface, the one the MPS machines have: kernel_input, sample_indices,
score_vjp, log_prob, bits_of, indices_of, sample, get_log_q_z_x, bond_dim, through this file's three hooks
(bornvi_ttn_environments / _sample / _score_vjp).  For n <= 20 the enumerated q is read out by log_prob over all 2^n indices
(probabilities64 / get_probabilities, detached).  Canonical form, bond spectra, compress_ / expand_, the posterior queries and
two-site sweeps exist for the real family only (SampledMPSBornMachine); here each raises a ValueError that says so.
"""
import torch
import torch.nn as nn

from . import backend
from .born_machine_sampled import SampledSurface, checked_init_method, checked_int, checked_seed, refuse

ENUMERATED_MAX_N = SampledSurface.ENUMERATED_MAX_N          # probabilities64: log_prob over all 2^n indices in one call


def live_mask(num_latent_vars, bond_dim):
    """bool [L - 1, D, D, D]: the entries of the cores that enter psi."""
    n, D = num_latent_vars, bond_dim
    _, L = backend.ttn_tree_shape(n)
    live = torch.ones(L - 1, D, D, D, dtype=torch.bool)
    live[0, 1:] = False                                      # the root's parent bond is the scalar psi
    for v in range(L // 2, L):
        j = 2 * v - L                                        # the left child's position
        live[v - 1, :, 2:, :] = False
        live[v - 1, :, :, 2:] = False
        if j >= n:
            live[v - 1, :, 1, :] = False
        if j + 1 >= n:
            live[v - 1, :, :, 1] = False
    return live


@refuse
class TreeSampledBornMachine(SampledSurface, nn.Module):
    """Tree-tensor-network Born machine whose surface is samples, log q of samples and the score-function gradient."""
    CORES = "tree cores"

    def __init__(self, num_latent_vars, bond_dim=4, init_method='small_random', conditioning_dim=0, seed=0):
        if conditioning_dim != 0:
            raise ValueError("TreeSampledBornMachine is not conditional: conditioning_dim must be 0.")
        n = checked_int(num_latent_vars, 1, backend.MPS_SAMPLED_MAX_N, "num_latent_vars")
        D = checked_int(bond_dim, 2, backend.TTN_MAX_BOND, "bond_dim", " (tree cores)")
        checked_init_method(init_method)
        checked_seed(seed)
        super().__init__()
        _, L = backend.ttn_tree_shape(n)
        live = live_mask(n, D)
        uniform = torch.zeros(L - 1, D, D, D, dtype=torch.float64)      # psi(z) = 2^(-n/2) for every z: the exactly uniform q
        uniform[:, 0, 0, 0] = 1.0
        for v in range(L // 2, L):
            j = 2 * v - L
            c = (j < n) + (j + 1 < n)                                    # the node's real children
            uniform[v - 1, 0][live[v - 1, 0]] = 2.0 ** (-c / 2.0)
        if init_method == 'zero':
            cores = uniform
        elif init_method == 'small_random':
            cores = uniform + 0.1 * torch.randn(L - 1, D, D, D, dtype=torch.float64) * live
        else:
            cores = torch.randn(L - 1, D, D, D, dtype=torch.float64) / (2.0 * D) ** 0.5 * live
        self._init_sampled(n, seed)
        self.cores = nn.Parameter(cores.contiguous())

    @classmethod
    def _with_cores(cls, cores, seed=0, num_latent_vars=None, **shape):
        """The machine of the given cores [L - 1, D, D, D] over num_latent_vars variables (L - 1 does not say n)."""
        machine = cls(num_latent_vars, bond_dim=int(cores.shape[1]), init_method='zero', seed=seed, **shape)
        if tuple(cores.shape) != tuple(machine.cores.shape):
            raise ValueError(f"tree cores over {num_latent_vars} variables are {tuple(machine.cores.shape)}, got {tuple(cores.shape)}")
        with torch.no_grad():
            machine.cores.copy_(cores)
        return machine

    # ---- the parameter ---------------------------------------------------------------------------------------------
    @property
    def bond_dim(self):
        return int(self.cores.shape[1])

    @property
    def tree_shape(self):
        """(h, L): the levels of nodes and the leaf positions."""
        return backend.ttn_tree_shape(self.num_latent_vars)

    def live_mask(self):
        """bool [L - 1, D, D, D] on the parameter's device: the entries that enter psi (the others stay 0.0)."""
        return live_mask(self.num_latent_vars, self.bond_dim).to(self.cores.device)

    @property
    def num_parameters(self):
        return int(live_mask(self.num_latent_vars, self.bond_dim).sum())

    # ---- the three calls the shared surface and a trainer need -----------------------------------------------------------
    def environments(self, cores, num_samples):
        return backend.ttn_environments(cores, self.num_latent_vars, num_samples)

    def draw(self, cores, num_samples, seed, epoch_dev):
        return backend.ttn_sample(cores, self.num_latent_vars, num_samples, seed, epoch_dev)

    def score_gradient(self, cores, idx, w):
        return backend.ttn_score_vjp(cores, self.num_latent_vars, idx, w)

    def log_prob(self, idx):
        """log q(idx), float64 [B] (-inf where psi is 0): the score call without a gradient."""
        cores, _ = self.kernel_input()
        idx = idx.reshape(-1).to(device=cores.device, dtype=torch.int64).contiguous()
        self.environments(cores, int(idx.numel()))
        return backend.ttn_score_vjp(cores, self.num_latent_vars, idx, out=False)[1]
