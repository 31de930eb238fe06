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

`QuantumFisherPreconditioner` preconditions with the quantum Fisher information instead (4 x the Fubini-Study metric, the
real part of the quantum geometric tensor; 4 x PennyLane's `metric_tensor`):

  Q_ab(theta) = Re<phi_a|phi_b> - Re(conj(c_a) c_b),   phi_a = psi(theta + pi e_a) = 2 d_a psi,   c_a = <psi|phi_a>.

It needs the P + 1 statevectors (backend.paramshift_states) and neither the parameter-shift rows nor 1/q, so the trainers
keep whichever gradient route they would take without it (fused dot, stored rows, adjoint), and no state is dropped at a
floor.  Q >= F in the Loewner order, so a given damping weighs no more against Q than against F.  The matrix is
backend.qfi_gram, the solve the same backend.spd_solve.
"""
import numpy as np

from . import backend

MAX_PARAMS = backend.FISHER_MAX_PARAMS


class FisherPreconditioner:
    quantum = False           # True: precondition(theta64, grad64) builds its own matrix (QuantumFisherPreconditioner)

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
        that damping, a FisherPreconditioner -> itself; "quantum" -> QuantumFisherPreconditioner(), an instance of it ->
        itself."""
        if spec is None or spec is False:
            return None
        if spec is True:
            return cls()
        if isinstance(spec, (FisherPreconditioner, QuantumFisherPreconditioner)):
            return spec
        if isinstance(spec, str):
            if spec == "quantum":
                return QuantumFisherPreconditioner()
            raise ValueError(f"natural_gradient: the only string accepted is 'quantum', got {spec!r}")
        if isinstance(spec, (int, float, np.integer, np.floating)):
            return cls(damping=spec)
        raise ValueError("natural_gradient must be None, True, a damping, 'quantum', a FisherPreconditioner or a "
                         f"QuantumFisherPreconditioner, got {spec!r}")

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


class QuantumFisherPreconditioner:
    """delta = (Q + damping I)^-1 grad with Q the quantum Fisher information of the circuit (module docstring).  The
    trainers bind it to their circuit (`bind`); it owns the states workspace, 16 (P + 1) 2^n bytes, and refuses a circuit
    whose workspace exceeds backend.WORKSPACE_CAP."""
    quantum = True

    def __init__(self, damping=1e-3):
        if isinstance(damping, bool) or not isinstance(damping, (int, float, np.integer, np.floating)) \
                or not np.isfinite(damping) or not damping >= 0:
            raise ValueError(f"damping must be a finite number >= 0, got {damping!r}")
        self.damping = float(damping)
        self.circuit = None       # (ansatz_type, n, layers)
        self._states = None       # complex128 [P + 1, 2^n], reused (a captured step writes into the same tensor)
        self._Q = None

    def bind(self, ansatz_type, n, layers, num_params=None):
        """The circuit whose metric this is.  ValueError when P > MAX_PARAMS or the states exceed the workspace cap."""
        n, layers = int(n), int(layers)
        P = int(num_params) if num_params is not None else backend.num_params(ansatz_type, n, layers)
        if P > MAX_PARAMS:
            raise ValueError(f"natural_gradient: {P} parameters; the device solve holds at most {MAX_PARAMS}")
        need = backend.paramshift_states_bytes(n, P)
        if need > backend.WORKSPACE_CAP:
            raise ValueError(f"natural_gradient='quantum': the {P} + 1 statevectors of {n} qubits take {need} bytes, more "
                             f"than the workspace cap of {backend.WORKSPACE_CAP}")
        if self.circuit != (ansatz_type, n, layers):
            self._states = self._Q = None
        self.circuit = (ansatz_type, n, layers)
        return self

    def qfi(self, theta64):
        """Q float64 [P, P] at theta64 (device tensor)."""
        if self.circuit is None:
            raise ValueError("QuantumFisherPreconditioner used before bind(ansatz_type, n, layers)")
        at, n, L = self.circuit
        P = theta64.numel()
        if self._states is not None and (self._states.shape[0] != P + 1 or self._states.device != theta64.device):
            self._states = self._Q = None
        self._states = backend.paramshift_states(at, n, L, theta64.reshape(-1), 0, P, include_base=True, out=self._states)
        self._Q = backend.qfi_gram(self._states[1:], self._states[0], out=self._Q)
        return self._Q

    def precondition(self, theta64, grad64):
        """-> (delta [P] float64 = (Q + damping I)^-1 grad64, info int32 [1]); delta = grad64 where info != 0."""
        return backend.spd_solve(self.qfi(theta64), grad64.reshape(-1), self.damping)
