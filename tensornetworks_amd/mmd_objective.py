"""The MMD side of training from data, independent of the variational family.

  MMD^2(q, p^) = (q - p^)^T K (q - p^),   K[z, z'] = kappa[d_H(z, z')]  (hamming_kernel.HammingMixtureKernel)

Enumerated families (quantum circuit, table, MLP, enumerated MPS) hold q for all 2^n states: `weights(q)` is the loss and
w = d loss / d q = 2 K (q - p^) by two Walsh-Hadamard transforms (backend.mmd_weights), the vector their gradient engines
consume.  Sampled families (n <= 63) hold draws z_1 .. z_B: `sample_weights(idx)` is the unbiased estimate

  U = Txx / (B (B - 1)) - 2 Txy / (B N) + Tyy / N^2

from integer pair counts (backend.hamming_pairs_rowsum) and the score-function weights w_b with leave-one-out baselines,

  w_b = (2 / B) [ (rxx_b / (B - 1) - m_b) - (rxy_b / N - c_b) ],   m_b = (Txx - 2 rxx_b) / ((B - 1)(B - 2)),
  c_b = (Txy - rxy_b) / ((B - 1) N),   sum_b w_b = 0,   grad U ~ sum_b w_b grad log q(z_b),   B >= 3."""
import numpy as np
import torch

from . import backend
from .hamming_kernel import HammingMixtureKernel

ENUMERATED_MAX_N = 30        # include/bornvi.h: BORNVI_TABLE_MAX_N


def mmd_u_and_weights(rxx, Txx, rxy, Txy, Tyy, B, N):
    """(U, w_b) of the module docstring from the row sums and totals, the same expression for torch tensors and NumPy arrays."""
    U = Txx / (B * (B - 1)) - 2.0 * Txy / (B * N) + Tyy / (N * N)
    m = (Txx - 2.0 * rxx) / ((B - 1) * (B - 2))
    c = (Txy - rxy) / ((B - 1) * N)
    w = (2.0 / B) * ((rxx / (B - 1) - m) - (rxy / N - c))
    return U, w


class MMDObjective:
    def __init__(self, num_vars, length_scales=(0.25, 1.0, 4.0), device='cpu'):
        """Touches neither the GPU nor the library."""
        self.kernel = HammingMixtureKernel(num_vars, length_scales)
        self.num_vars = self.kernel.num_vars
        self._device = device
        self.target = None           # p^ float64 [2^n] on the GPU (n <= 30), what weights() reads
        self.data_indices = None     # int64 [N] on the GPU, what sample_weights() reads (None after a probability table)
        self.Tyy = None              # float64 [1] on the GPU: sum_{j, j'} kappa[d(y_j, y_j')], the diagonal included
        self.num_data = 0

    # ---- the data --------------------------------------------------------------------------------------------------
    def _indices_of(self, data):
        """Bit rows [N, n] or indices [N] -> int64 [N] on the host, checked."""
        n = self.num_vars
        t = torch.as_tensor(data)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            if t.dim() != 2:
                raise ValueError("data: bit rows [N, n], int64 indices [N] or a probability table [2^n]")
            if not bool(((t == 0) | (t == 1)).all()):
                raise ValueError("data: bit rows must hold 0 and 1 only")
            t = t.to(torch.int64)
        t = t.to(torch.int64).cpu()
        if t.dim() == 2:
            if t.shape[1] != n:
                raise ValueError(f"data: bit rows of {n} entries expected, got {tuple(t.shape)}")
            if t.numel() and (int(t.min()) < 0 or int(t.max()) > 1):
                raise ValueError("data: bit rows must hold 0 and 1 only")
            weights = (1 << torch.arange(n - 1, -1, -1, dtype=torch.int64))      # tuple position p is bit n - 1 - p
            t = (t * weights).sum(dim=1)
        elif t.dim() != 1:
            raise ValueError("data: bit rows [N, n], int64 indices [N] or a probability table [2^n]")
        if t.numel() == 0:
            raise ValueError("data: at least one data point is needed (N = 0)")
        if t.numel() > backend.HAMMING_PAIRS_MAX_B:
            raise ValueError(f"data: at most 2^20 data points, got {t.numel()}")
        if int(t.min()) < 0 or int(t.max()) >= (1 << n):
            raise ValueError(f"data: indices must lie in 0 ... 2^{n} - 1")
        return t.contiguous()

    def prepare(self, data):
        """data: bit rows [N, n], int64 indices [N], or (n <= 30) a floating-point probability table [2^n].  Keeps target
        (n <= 30), data_indices and Tyy.  Argument errors are raised before any GPU call."""
        n = self.num_vars
        t = torch.as_tensor(data)
        table = t.dim() == 1 and t.dtype.is_floating_point
        if table:
            if n > ENUMERATED_MAX_N or t.numel() != (1 << n):
                raise ValueError(f"data: a probability table needs n <= {ENUMERATED_MAX_N} and 2^n entries, got {t.numel()} at n = {n}")
            if not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
                raise ValueError("data: a probability table must be finite and non-negative")
            idx = None
        else:
            idx = self._indices_of(t)
        dev = backend.compute_device(self._device)
        lam = self.kernel.spectrum_on(dev)
        if table:
            self.target = t.to(device=dev, dtype=torch.float64).contiguous().clone()
            self.data_indices, self.num_data = None, 0
            self.Tyy = backend.mmd_weights(self.target, None, lam, want_w=False)[0]      # p^T K p
            return
        self.data_indices = idx.to(dev)
        self.num_data = int(idx.numel())
        self.target = None
        if n <= ENUMERATED_MAX_N:
            self.target = torch.bincount(self.data_indices, minlength=1 << n).to(torch.float64) / self.num_data
        self.Tyy = backend.hamming_pairs_rowsum(self.data_indices, self.data_indices, self.kernel.kappa_on(dev))[1]

    # ---- enumerated families ---------------------------------------------------------------------------------------
    def weights(self, q, want_w=True, out=None):
        """q float64 [2^n] on the GPU -> (loss [1] = MMD^2(q, p^), w [2^n] = d loss / d q or None)."""
        if self.target is None:
            raise ValueError("MMDObjective.weights before prepare(data), or n > 30 (use sample_weights)")
        return backend.mmd_weights(q, self.target, self.kernel.spectrum_on(q.device), want_w=want_w, out=out)

    # ---- sampled families ------------------------------------------------------------------------------------------
    def sample_weights(self, idx):
        """idx int64 [B] on the GPU, B >= 3 -> (U [] float64, w_b [B] float64): two pair-count calls and elementwise
        operations on B doubles, nothing read back."""
        if self.data_indices is None:
            raise ValueError("MMDObjective.sample_weights before prepare(data) with data points (a probability table has none)")
        if not torch.is_tensor(idx) or idx.dim() != 1 or int(idx.numel()) < 3:
            raise ValueError("sample_weights: idx must be an int64 [B] tensor with B >= 3")
        B, N = int(idx.numel()), self.num_data
        kappa = self.kernel.kappa_on(idx.device)
        rxx, Txx, _ = backend.hamming_pairs_rowsum(idx, idx, kappa, skip_same_index=True)
        rxy, Txy, _ = backend.hamming_pairs_rowsum(idx, self.data_indices, kappa)
        U, w = mmd_u_and_weights(rxx, Txx, rxy, Txy, self.Tyy, B, N)
        return U.reshape(()), w
