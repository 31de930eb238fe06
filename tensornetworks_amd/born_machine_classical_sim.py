"""Classical Born machine on MI355X: drop-in for the reference's ClassicalBornMachine (born_machine_classical_sim.py).

Same constructor, attributes, initialisation (the same draws from torch's CPU generator in the same order, so
torch.manual_seed(s) gives the reference's starting parameters bit for bit), methods and error messages.  What changed
is where logits -> q happens: one `bornvi_born_table_probs` launch (softmax with the row maximum subtracted, or
|w| / sum |w|, plus the entropy when asked for), wrapped in a torch.autograd.Function whose backward is
`bornvi_born_table_vjp`.  In MLP mode (conditioning_dim > 0) the network itself stays stock torch.nn; only its logits
go through the kernels.  The kernels run on backend.compute_device(...) and results come back on the parameters'
device.  Sampling is torch.multinomial plus bit unpacking, log q a vectorised gather: no lookups in 2^n tuples.
"""
import torch
import torch.nn as nn

from . import backend
from .utils import generate_all_binary_outcomes


class _TableProbs(torch.autograd.Function):
    """q32 = born_table_probs(w); backward: born_table_vjp with y = dL/dq (no KSD scaling, no entropy term)."""

    @staticmethod
    def forward(ctx, w, mode):
        q32, q64, _ = backend.born_table_probs(w, mode, want_entropy=False)
        ctx.save_for_backward(w, q64)
        ctx.mode = mode
        return q32

    @staticmethod
    def backward(ctx, grad_q):
        w, q64 = ctx.saved_tensors
        return backend.born_table_vjp(w, q64, ctx.mode, y=grad_q.to(torch.float64).contiguous()), None


class _TableEntropy(torch.autograd.Function):
    """H = -sum q log max(q, 1e-10) over every row of the table (the reference's entropy() of the squeezed table);
    backward: the entropy term of born_table_vjp."""

    @staticmethod
    def forward(ctx, w, mode):
        _, q64, H = backend.born_table_probs(w, mode, want_entropy=True)
        ctx.save_for_backward(w, q64)
        ctx.mode = mode
        return H.sum()

    @staticmethod
    def backward(ctx, grad_h):
        w, q64 = ctx.saved_tensors
        # the kernel differentiates L = -lambda H: lambda = -1 gives dH/dw
        g = backend.born_table_vjp(w, q64, ctx.mode, entropy_weight=-1.0)
        return g * grad_h.to(g.dtype), None


class ClassicalBornMachine(nn.Module):
    """Softmax (use_logits) or abs-normalised probability table over the 2^n latent states, or, with
    conditioning_dim > 0, an MLP of x producing its logits (reference born_machine_classical_sim.py:7-181)."""

    def __init__(self, num_latent_vars, use_logits=True, conditioning_dim=0,
                 init_method='small_random', hidden_dims=None, use_layer_norm=False):
        super().__init__()
        self.num_latent_vars = num_latent_vars
        self.num_outcomes = 2 ** num_latent_vars
        self.use_logits = use_logits
        self.conditioning_dim = conditioning_dim
        self.use_layer_norm = use_layer_norm
        self._fixed_probs = None
        self._use_fixed_probs = False
        self._outcomes = None

        if self.conditioning_dim > 0:
            if hidden_dims is None:
                hidden_dims = [max(self.conditioning_dim * 4, 64), max(self.conditioning_dim * 2, 32)]
            layers, width = [], self.conditioning_dim
            for h_dim in hidden_dims:
                layers.append(nn.Linear(width, h_dim))
                if use_layer_norm:
                    layers.append(nn.LayerNorm(h_dim))
                layers.append(nn.ReLU())
                layers.append(nn.Dropout(0.1))
                width = h_dim
            layers.append(nn.Linear(width, self.num_outcomes))
            self.param_generator_net = nn.Sequential(*layers)
            for m in self.param_generator_net.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_uniform_(m.weight)
                    nn.init.zeros_(m.bias)
        else:
            N = self.num_outcomes
            if init_method == 'zero':
                init = torch.zeros(N)
            elif init_method == 'small_random':
                init = 0.1 * torch.randn(N)
            elif init_method == 'uniform':
                init = torch.log(torch.ones(N) / N) + 0.01 * torch.randn(N)
            else:
                init = torch.randn(N)
            self.params = nn.Parameter(init)

    @property
    def born_mode(self):
        """Kernel mode of the table: 0 = softmax of logits, 1 = |w| / sum |w|."""
        return 0 if self.use_logits else 1

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

    def raw_params(self, x_condition=None):
        """The table [1, 2^n] or the network's logits [B, 2^n], with the reference's x_condition checks."""
        if self.conditioning_dim > 0:
            if x_condition is None:
                raise ValueError("x_condition must be provided for conditional Born machine.")
            x_batched = x_condition.unsqueeze(0) if x_condition.ndim == 1 else x_condition
            return self.param_generator_net(x_batched)
        if x_condition is not None:
            raise ValueError("x_condition provided but conditioning_dim is 0.")
        return self.params.unsqueeze(0)

    @staticmethod
    def kernel_input(raw):
        """(raw as a contiguous float32 tensor on the compute device -- differentiable --, raw's own device)."""
        home = raw.device
        return raw.to(device=backend.compute_device(home), dtype=torch.float32).contiguous(), home

    def get_probabilities(self, x_condition=None):
        """float32 [B, 2^n] ([1, 2^n] unconditioned), differentiable; the fixed probabilities when set."""
        if self._use_fixed_probs and self._fixed_probs is not None:
            return self._fixed_probs.unsqueeze(0) if self._fixed_probs.ndim == 1 else self._fixed_probs
        w, home = self.kernel_input(self.raw_params(x_condition))
        return _TableProbs.apply(w, self.born_mode).to(home)

    def sample(self, num_samples=1, x_condition=None):
        """float32 bit rows [num, n], or [B, num, n] for a batch of conditions."""
        probs = self.get_probabilities(x_condition).detach()
        probs = probs + 1e-10
        probs = probs / probs.sum(dim=-1, keepdim=True)
        batched = probs.shape[0] > 1 or (x_condition is not None and x_condition.ndim > 1)
        idx = torch.multinomial(probs, num_samples, replacement=True)            # [B, num]
        n = self.num_latent_vars
        shifts = torch.arange(n - 1, -1, -1, device=idx.device)
        bits = ((idx.unsqueeze(-1) >> shifts) & 1).to(torch.float32)
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
        z = z_samples.detach().to(log_probs.device).long()      # `.long()` truncates like the reference's
        n = self.num_latent_vars
        if z.dim() == 2 and z.shape[1] == n:
            bad = ((z != 0) & (z != 1)).any(dim=1)
        else:
            bad = torch.ones(bz, dtype=torch.bool, device=z.device)
        if bool(bad.any()):
            row = int(torch.nonzero(bad)[0])
            raise ValueError(f"Sample {tuple(z[row].tolist())} is not a valid outcome.")
        idx = (z * (1 << torch.arange(n - 1, -1, -1, device=z.device))).sum(dim=1)
        if bx == 1:
            return log_probs[0, idx]
        return log_probs[torch.arange(bz, device=idx.device), idx]

    def entropy(self, x_condition=None):
        """-sum q log max(q, 1e-10) (a second forward, as in the reference), differentiable."""
        if self._use_fixed_probs and self._fixed_probs is not None:
            probs = self.get_probabilities(x_condition).squeeze()
            return -(probs * torch.log(probs.clamp(min=1e-10))).sum()
        w, home = self.kernel_input(self.raw_params(x_condition))
        return _TableEntropy.apply(w, self.born_mode).to(home)
