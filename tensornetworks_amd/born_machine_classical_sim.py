"""Classical Born machine on MI355X: drop-in for the reference's ClassicalBornMachine (born_machine_classical_sim.py).

Same constructor, attributes, initialisation (the same draws from torch's CPU generator in the same order, so
torch.manual_seed(s) gives the reference's starting parameters bit for bit), methods and error messages.  What changed
is where logits -> q happens: one `bornvi_born_table_probs` launch (softmax with the row maximum subtracted, or
|w| / sum |w|, plus the entropy when asked for), wrapped in a torch.autograd.Function whose backward is
`bornvi_born_table_vjp`.  In MLP mode (conditioning_dim > 0) the network itself stays stock torch.nn; only its logits
go through the kernels.  The kernels run on backend.compute_device(...) and results come back on the parameters'
device.  The surface the trainers use (fixed probabilities, sampling by torch.multinomial plus bit unpacking, log q as a
vectorised gather, the probability dict) is born_machine_base.EnumeratedBornMachine's, shared with the MPS family; this
file supplies logits -> q and the table's two ends of a training epoch (epoch_forward, epoch_backward).
"""
import torch
import torch.nn as nn

from . import backend
from .born_machine_base import EnumeratedBornMachine, EpochForward


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


class ClassicalBornMachine(EnumeratedBornMachine):
    """Softmax (use_logits) or abs-normalised probability table over the 2^n latent states, or, with
    conditioning_dim > 0, an MLP of x producing its logits (reference born_machine_classical_sim.py:7-181)."""

    def __init__(self, num_latent_vars, use_logits=True, conditioning_dim=0,
                 init_method='small_random', hidden_dims=None, use_layer_norm=False):
        super().__init__(num_latent_vars, conditioning_dim)
        self.use_logits = use_logits
        self.use_layer_norm = use_layer_norm

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
    def draws_in_forward(self):
        """The MLP's Dropout layers draw in every forward: two forwards are two different samples."""
        return self.conditioning_dim > 0

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

    def _probabilities(self, x_condition):
        w, home = self.kernel_input(self.raw_params(x_condition))
        return _TableProbs.apply(w, self.born_mode).to(home)

    def _entropy(self, x_condition):
        w, home = self.kernel_input(self.raw_params(x_condition))
        return _TableEntropy.apply(w, self.born_mode).to(home)

    # ---- the two ends of a training epoch: parameters -> q, and dL/dq -> the gradient of the table or of the logits
    def epoch_forward(self, x_condition, want_entropy):
        """state = (leaf: the table parameter or the network's logits on the compute device, w: the detached kernel input
        [1, 2^n], q64 [1, 2^n], home: the table parameter's device or None); the entropy is float32."""
        if self.conditioning_dim == 0:
            leaf, home = self.params, self.params.device
            w = leaf.detach().to(backend.compute_device(home)).reshape(1, -1)
        else:
            leaf, home = self.kernel_input(self.raw_params(x_condition))[0], None
            if leaf.shape[0] != 1:
                raise ValueError(f"Probabilities shape mismatch: {tuple(leaf.shape)}")
            w = leaf.detach()
        q32, q64, H = backend.born_table_probs(w, self.born_mode, want_entropy=want_entropy)
        return EpochForward(q32[0], q64[0], H, (leaf, w, q64, home))

    def epoch_backward(self, fwd, y=None, ksd2=None, entropy_weight=0.0):
        leaf, w, q64, home = fwd.state
        loss = torch.empty(1, dtype=torch.float64, device=w.device) if ksd2 is not None else None
        g = backend.born_table_vjp(w, q64, self.born_mode, y=y.reshape(1, -1) if y is not None else None, ksd2=ksd2,
                                   entropy_weight=entropy_weight, loss_out=loss)
        return loss, [(leaf, g if home is None else g.reshape(leaf.shape).to(home))]
