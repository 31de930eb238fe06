"""What the sampled MPS Born-machine families have in common: the real one (born_machine_mps_sampled.py), the one with complex
cores (born_machine_cmps_sampled.py) and the locally purified one (born_machine_lps_sampled.py).

  SampledSurface       mixin over an nn.Module with a float64 parameter `cores`: kernel_input, sample_indices, bits_of,
                       indices_of, sample, score_vjp, log_prob, get_log_q_z_x, probabilities64 / get_probabilities, all
                       through the family's three hooks (what a trainer's epoch calls too):
                         environments(cores, num_samples)          the sweeps the two calls after it read
                         draw(cores, num_samples, seed, epoch_dev) -> (idx, logq, status)
                         score_gradient(cores, idx, w)             -> (grad, logq, status)
  checked_int / checked_init_method / checked_seed    the constructors' argument checks and their messages
  refuse               the methods a family does not offer (REFUSED: they exist for the real family only), in its own wording

A family states its cores (shape, limits, initialisation), its constructors from other states, its hooks, and the class
attributes ENUMERATED_MAX_N, NATURAL_GRADIENT and CORES (the word its refusals use).
"""
import torch

from . import backend
from .born_machine_base import bits_to_indices, indices_to_bits

REFUSED = ("bond_spectrum", "bond_entropies", "canonical_cores", "canonicalise_", "compress_", "expand_", "two_site_sweep_",
           "fit_two_site", "marginals", "pair_marginals", "log_marginal", "log_marginal_vjp", "sample_given")


def checked_int(value, lo, hi, what, note=""):
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise ValueError(f"{what} must be an integer in {lo} ... {hi}{note}, got {value!r}")
    return value


def checked_init_method(init_method):
    if init_method not in ('small_random', 'zero', 'random'):
        raise ValueError(f"init_method must be 'small_random', 'zero' or 'random', got {init_method!r}")
    return init_method


def checked_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    return seed


def refuse(cls):
    """Gives `cls` every method of REFUSED as one that raises, and the list itself as cls.REFUSED."""
    def refused(name):
        def method(self, *args, **kwargs):
            raise ValueError(f"{name} is not offered for {cls.CORES}: it exists for the real family (SampledMPSBornMachine) only")
        method.__name__ = name
        method.__doc__ = f"Not offered for {cls.CORES} (SampledMPSBornMachine has {name})."
        return method
    cls.REFUSED = REFUSED
    for name in REFUSED:
        setattr(cls, name, refused(name))
    return cls


class SampledSurface:
    """Mixin of the three sampled machines: samples, log q of samples and the score-function gradient of `cores`."""
    ENUMERATED_MAX_N = 20          # probabilities64: log_prob over all 2^n indices in one call
    NATURAL_GRADIENT = False       # the Fisher estimates (natural_gradient.py) exist for the real family only
    CORES = None                   # "complex cores", "purified cores": the family's word in its refusals

    def _init_sampled(self, num_latent_vars, seed):
        self.num_latent_vars = num_latent_vars
        self.conditioning_dim = 0
        self.seed = seed
        self._draws = 0            # epoch of the next sample() call: successive calls draw fresh samples

    @classmethod
    def _with_cores(cls, cores, seed=0, **shape):
        """The machine of the given cores [n, 2, ...]; shape: the constructor's own view of them (bond_dim, ...)."""
        machine = cls(int(cores.shape[0]), init_method='zero', seed=seed, **shape)
        with torch.no_grad():
            machine.cores.copy_(cores)
        return machine

    # ---- the parameter ---------------------------------------------------------------------------------------------
    @property
    def bond_dim(self):
        return int(self.cores.shape[2])

    @property
    def num_parameters(self):
        return self.cores.numel()

    def kernel_input(self):
        """(cores detached as a contiguous float64 tensor on the compute device, the parameter's own device)."""
        home = self.cores.device
        return self.cores.detach().to(device=backend.compute_device(home), dtype=torch.float64).contiguous(), home

    # ---- the three calls a trainer needs: the family's ---------------------------------------------------------------
    def environments(self, cores, num_samples):
        raise NotImplementedError

    def draw(self, cores, num_samples, seed, epoch_dev):
        raise NotImplementedError

    def score_gradient(self, cores, idx, w):
        raise NotImplementedError

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
        """int64 outcome indices of bit rows [B, n] (validated like MPSBornMachine.get_log_q_z_x)."""
        return bits_to_indices(z_samples, self.num_latent_vars)

    def sample(self, num_samples=1, x_condition=None):
        """float32 bit rows [num, n] on the parameter's device, from the draws of sample_indices (fresh ones every call)."""
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")
        idx, _ = self.sample_indices(num_samples, epoch=self._draws)
        self._draws += 1
        return self.bits_of(idx).to(self.cores.device)

    def score_vjp(self, idx, w):
        """(grad float64, of the cores' shape = the gradient of sum_b w_b log q(idx_b) in the parameter, logq float64 [B]) on
        the compute device."""
        cores, _ = self.kernel_input()
        idx = idx.to(device=cores.device, dtype=torch.int64).contiguous()
        w = w.to(device=cores.device, dtype=torch.float64).contiguous()
        self.environments(cores, int(idx.numel()))
        grad, logq, _ = self.score_gradient(cores, idx, w)
        return grad, logq

    def log_prob(self, idx):
        """log q(idx), float64 [B] (-inf where q is 0)."""
        idx = idx.reshape(-1)
        return self.score_vjp(idx, torch.zeros(idx.numel(), dtype=torch.float64, device=idx.device))[1]

    def get_log_q_z_x(self, z_samples, x_condition=None):
        """log q(z) for a batch of bit rows, float64 (no floor: it is evaluated per sample, not read from a table)."""
        if x_condition is not None:
            raise ValueError("x_condition provided but Born machine is not conditional.")
        return self.log_prob(self.indices_of(z_samples)).to(z_samples.device)

    # ---- the enumerated distribution, where it exists ------------------------------------------------------------
    def _check_enumerated(self, x_condition):
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")
        if self.num_latent_vars > self.ENUMERATED_MAX_N:
            raise ValueError(f"the 2^n probabilities exist for num_latent_vars <= {self.ENUMERATED_MAX_N} only "
                             f"(got {self.num_latent_vars}): use sample_indices and log_prob")

    def probabilities64(self, x_condition=None):
        """float64 [2^n] on the parameter's device, detached (n <= ENUMERATED_MAX_N): exp(log_prob) of all 2^n indices, one
        call."""
        self._check_enumerated(x_condition)
        dev = backend.compute_device(self.cores.device)
        idx = torch.arange(1 << self.num_latent_vars, dtype=torch.int64, device=dev)
        return torch.exp(self.log_prob(idx)).to(self.cores.device)

    def get_probabilities(self, x_condition=None):
        """float32 [1, 2^n] of probabilities64 (n <= ENUMERATED_MAX_N)."""
        return self.probabilities64(x_condition).to(torch.float32).unsqueeze(0)
