"""Natural-gradient preconditioning for the quantum Born-machine trainers on MI355X.

The classical Fisher information matrix of the Born distribution,

  F_ab(theta) = sum_z d_a q_z d_b q_z / q_z,   d_a q = 1/2 (q(theta + pi/2 e_a) - q(theta - pi/2 e_a)),

is a [P, P] Gram of the rows the stored-rows parameter-shift route already leaves in device memory for one step
(backend.paramshift_probs), weighted by 1/q.  The natural-gradient step delta = (F + damping I)^-1 g follows distances
between distributions, not between parameter vectors.  Both quantum trainers (ksd_vi_quantum.py, elbo_vi_quantum.py) hold
one `FisherPreconditioner`, as both ELBO trainers share `ElboObjective`: the matrix is backend.fisher_gram (fp64 matrix
cores, bitwise reproducible), the solve backend.spd_solve (one-workgroup Cholesky); neither allocates or synchronises
once its workspace exists, so a step stays a graph replay.  When the factorisation fails (info != 0) delta is the plain
gradient: the trainers' NaN/Inf guard looks at the loss only.
"""
import numpy as np

from . import backend

MAX_PARAMS = backend.FISHER_MAX_PARAMS


class FisherPreconditioner:
    def __init__(self, damping=1e-3, q_floor=1e-10):
        for name, v, zero_ok in (("damping", damping, True), ("q_floor", q_floor, False)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) \
                    or not (v >= 0 if zero_ok else v > 0):
                raise ValueError(f"{name} must be a finite number {'>= 0' if zero_ok else '> 0'}, got {v!r}")
        self.damping, self.q_floor = float(damping), float(q_floor)
        self._F = None            # [P, P] of the last call, reused (a captured step writes into the same tensor)

    @classmethod
    def coerce(cls, spec):
        """What the trainers' `natural_gradient` keyword accepts: None / False -> None, True -> the defaults, a number ->
        that damping, a FisherPreconditioner -> itself."""
        if spec is None or spec is False:
            return None
        if spec is True:
            return cls()
        if isinstance(spec, cls):
            return spec
        if isinstance(spec, (int, float, np.integer, np.floating)):
            return cls(damping=spec)
        raise ValueError(f"natural_gradient must be None, True, a damping or a FisherPreconditioner, got {spec!r}")

    def fisher(self, shifted, q, out=None):
        """F float64 [P, P] from the stored rows shifted [2 P, 2^n] and q [2^n] (device tensors)."""
        return backend.fisher_gram(shifted, q, self.q_floor, out=out)

    def precondition(self, shifted, q, grad64):
        """-> (delta [P] float64 = (F + damping I)^-1 grad64, info int32 [1]); delta = grad64 where info != 0."""
        P = grad64.numel()
        if self._F is None or self._F.shape[0] != P or self._F.device != grad64.device:
            self._F = None
        self._F = self.fisher(shifted, q, out=self._F)
        return backend.spd_solve(self._F, grad64.reshape(-1), self.damping)
