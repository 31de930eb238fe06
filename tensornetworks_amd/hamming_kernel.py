"""A mixture of the project's base kernel over several length scales, as a function of the Hamming distance.

  kappa[d] = sum_c a_c rho_c^d,  rho_c = exp(-1 / (n l_c)),  a_c = 1 / C,  d = 0 .. n

(the Gaussian mixture of the circuit-Born-machine literature: on bit vectors ||z - z'||^2 is the Hamming distance).  For one
length scale it is stein_utils.base_hamming_kernel_torch.  A kernel of the Hamming distance alone is diagonal under the
Walsh-Hadamard transform H = [[1, 1], [1, -1]]^(x n):  K = 2^-n H diag(lam[popcount k]) H with

  lam[j] = sum_c a_c (1 + rho_c)^(n - j) (1 - rho_c)^j > 0,    2^-n sum_k lam[popcount k] = kappa[0] = 1.

Both tables are computed once on the host, in np.longdouble where the platform's is wider than double and otherwise with
math.fsum over double terms, and rounded to float64."""
import math

import numpy as np
import torch

MAX_SCALES = 8          # include/bornvi_mmd.h: BORNVI_MMD_MAX_SCALES
MAX_VARS = 63


def _tables(n, scales):
    C = len(scales)
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        ld = np.longdouble
        rho = [np.exp(-ld(1) / (ld(n) * ld(l))) for l in scales]
        kappa = [sum(r ** d for r in rho) / ld(C) for d in range(n + 1)]
        lam = [sum((1 + r) ** (n - j) * (1 - r) ** j for r in rho) / ld(C) for j in range(n + 1)]
        return np.array(kappa, dtype=np.float64), np.array(lam, dtype=np.float64)
    rho = [math.exp(-1.0 / (n * l)) for l in scales]
    kappa = [math.fsum(r ** d / C for r in rho) for d in range(n + 1)]
    lam = [math.fsum((1 + r) ** (n - j) * (1 - r) ** j / C for r in rho) for j in range(n + 1)]
    return np.array(kappa, dtype=np.float64), np.array(lam, dtype=np.float64)


class HammingMixtureKernel:
    def __init__(self, num_vars, length_scales=(0.25, 1.0, 4.0)):
        """Touches neither the GPU nor the library."""
        if isinstance(num_vars, bool) or not isinstance(num_vars, (int, np.integer)) or not 1 <= int(num_vars) <= MAX_VARS:
            raise ValueError(f"num_vars must be an integer in 1 ... {MAX_VARS}, got {num_vars!r}")
        if isinstance(length_scales, (int, float)) and not isinstance(length_scales, bool):
            length_scales = (length_scales,)
        try:
            scales = tuple(length_scales)
        except TypeError:
            raise ValueError(f"length_scales must be a sequence of positive numbers, got {length_scales!r}") from None
        if not 1 <= len(scales) <= MAX_SCALES:
            raise ValueError(f"length_scales: 1 ... {MAX_SCALES} entries, got {len(scales)}")
        for l in scales:
            if isinstance(l, bool) or not isinstance(l, (int, float, np.integer, np.floating)) or not math.isfinite(l) or not l > 0:
                raise ValueError(f"length_scales must be positive finite numbers, got {l!r}")
        self.num_vars = int(num_vars)
        self.length_scales = tuple(float(l) for l in scales)
        self.kappa, self.spectrum = _tables(self.num_vars, self.length_scales)      # float64 [n + 1], host
        self._dev = {}

    def tables_on(self, device):
        """(kappa, spectrum) as float64 [n + 1] tensors on `device`, made once per device."""
        dev = torch.device(device)
        key = (dev.type, dev.index)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.kappa).to(dev), torch.from_numpy(self.spectrum).to(dev))
        return self._dev[key]

    def kappa_on(self, device):
        return self.tables_on(device)[0]

    def spectrum_on(self, device):
        return self.tables_on(device)[1]

    def __call__(self, z1, z2):
        """kappa of the Hamming distance of bit rows z1, z2 [..., n] (broadcast over the leading dimensions): the torch
        reference, the mean over the length scales of base_hamming_kernel_torch, float64, differentiable in neither."""
        from .stein_utils import base_hamming_kernel_torch
        z1, z2 = torch.as_tensor(z1), torch.as_tensor(z2)
        if z1.shape[-1] != self.num_vars or z2.shape[-1] != self.num_vars:
            raise ValueError(f"bit rows of {self.num_vars} entries expected, got shapes {tuple(z1.shape)} and {tuple(z2.shape)}")
        z1, z2 = z1.to(torch.float64), z2.to(torch.float64)
        out = None
        for l in self.length_scales:
            k = base_hamming_kernel_torch(z1, z2, self.num_vars, l)
            out = k if out is None else out + k
        return out / len(self.length_scales)

    def dense(self, device="cpu"):
        """K [2^n, 2^n] float64 through __call__ on all bit rows (tuple position p is bit n - 1 - p), for small n."""
        n = self.num_vars
        if n > 12:
            raise ValueError("dense(): n <= 12")
        idx = torch.arange(1 << n, device=device)
        bits = ((idx[:, None] >> torch.arange(n - 1, -1, -1, device=device)) & 1).to(torch.float64)
        return self(bits[:, None, :], bits[None, :, :])
