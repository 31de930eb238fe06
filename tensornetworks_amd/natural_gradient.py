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

`SampledFisherPreconditioner` is the natural gradient of the sampled MPS trainers (sampled_trainer.py), where no 2^n row
exists: the Fisher matrix of the family is estimated from the epoch's own samples as the Gram of their centred score rows
(stochastic reconfiguration),

  F^ = (1/B) sum_b o_b o_b^T,   o_b[k, s, a, c] = 2 [z_bk = s] l_b,k-1[a] r_b,k[c] / psi_b - mu[k, s, a, c],

mu the exact mean of the first term under q (backend.mps_score_rows: E_q[o] = 0, so no sample-mean correction), on the
same SYRK core (backend.score_fisher_gram) and the same Cholesky body, one workgroup per block
(backend.spd_solve_batched).  blocks='site' keeps the n diagonal blocks of 2 D^2 x 2 D^2, blocks='full' the whole matrix
of P = 2 n D^2.  F is singular (scale and gauge of every core leave q unchanged): the damping is what makes the solve
succeed, and a block whose factorisation fails keeps its plain gradient.  DESIGN.md section 6i.

`SampleSpaceFisherPreconditioner` is the same full-matrix step solved in sample space (minSR).  The
trainers' gradient is O^T w with O the B x P matrix of the score rows, and

  (O^T O / B + damping I)^-1 O^T w = O^T u,   (T + damping I) u = w,   T = O O^T / B,

so the exact blocks='full' step needs a B x B Gram (backend.mps_score_sample_gram, from the samples' left and right vectors:
no row is formed), one backend.spd_solve of size B <= 1024 and one more backend.mps_score_vjp with the weights u.  P is not
limited.  Duplicate samples make T singular: the damping must be positive.

`CGFisherPreconditioner` solves the same full-matrix system with no matrix at all: conjugate
gradients on (O^T O / B + damping I) delta = g, one product p -> O^T (O p) / B per iteration, O p from
backend.mps_score_jvp (a tangent sweep, one sample per lane) and O^T t from backend.mps_score_vjp, the recurrence on the
device (backend.cg_init / cg_step / cg_finish).  Neither P nor B is limited by a factorisation: every (n, D, B) the sampler
accepts.  It always launches max_iters iterations; those after convergence write nothing.
"""
import numpy as np
import torch

from . import backend

MAX_PARAMS = backend.FISHER_MAX_PARAMS
SAMPLED_ROWS_BUDGET = min(2 << 30, backend.WORKSPACE_CAP)      # bytes of score rows held at once (SampledFisherPreconditioner)


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


class SampledFisherPreconditioner:
    """delta = (F^ + damping I)^-1 grad with F^ the sampled Fisher estimate of an MPS Born machine (module docstring), per
    site (blocks='site', 2 D^2 <= 1024) or for all P = 2 n D^2 <= 1024 parameters at once (blocks='full').  It owns the rows
    buffer, F, delta and the infos, reused across calls (a captured step writes into the same tensors).  In 'site' mode
    the sites go through in chunks whose score rows fit rows_budget_bytes."""
    BLOCKS = ("site", "full")

    def __init__(self, damping=1e-3, blocks='site', rows_budget_bytes=SAMPLED_ROWS_BUDGET):
        if isinstance(damping, bool) or not isinstance(damping, (int, float, np.integer, np.floating)) \
                or not np.isfinite(damping) or not damping >= 0:
            raise ValueError(f"damping must be a finite number >= 0, got {damping!r}")
        if blocks not in self.BLOCKS:
            raise ValueError(f"blocks must be 'site' or 'full', got {blocks!r}")
        rb = rows_budget_bytes
        if isinstance(rb, bool) or not isinstance(rb, (int, np.integer)) or not 1 <= rb <= backend.WORKSPACE_CAP:
            raise ValueError(f"rows_budget_bytes must be an integer in 1 ... {backend.WORKSPACE_CAP} (the workspace cap), got {rb!r}")
        self.damping, self.blocks, self.rows_budget_bytes = float(damping), blocks, int(rb)
        self.info = None          # int32 [nblocks] of the last call
        self.status = None        # int32 [1]: the rows' status word of the last call (2: some psi(z_b) was 0 or not finite)
        self._key = None
        self._rows = self._F = self._delta = None

    @classmethod
    def coerce(cls, spec):
        """What the sampled trainers' `natural_gradient` keyword accepts: None / False -> None, True -> the defaults, a
        number -> that damping, 'site' / 'full' -> that block structure, a SampledFisherPreconditioner -> itself;
        'sample' -> SampleSpaceFisherPreconditioner(), 'cg' -> CGFisherPreconditioner(), an instance of either -> itself."""
        if spec is None or spec is False:
            return None
        if spec is True:
            return cls()
        if isinstance(spec, (cls, SampleSpaceFisherPreconditioner, CGFisherPreconditioner)):
            return spec
        if isinstance(spec, str):
            if spec in cls.BLOCKS:
                return cls(blocks=spec)
            if spec == "sample":
                return SampleSpaceFisherPreconditioner()
            if spec == "cg":
                return CGFisherPreconditioner()
            raise ValueError(f"natural_gradient: the strings accepted are 'site', 'full', 'sample' and 'cg', got {spec!r}")
        if isinstance(spec, (int, float, np.integer, np.floating)):
            return cls(damping=spec)
        raise ValueError("natural_gradient must be None, True, a damping, 'site', 'full', 'sample', 'cg', a "
                         "SampledFisherPreconditioner, a SampleSpaceFisherPreconditioner or a CGFisherPreconditioner, "
                         f"got {spec!r}")

    def plan(self, n, D, B):
        """(block size R, number of blocks, sites per chunk) for cores [n, 2, D, D] and B samples; every ValueError of the
        shape is raised here, without touching the GPU."""
        n, D, B = int(n), int(D), int(B)
        if not 1 <= n <= backend.MPS_SAMPLED_MAX_N:
            raise ValueError(f"natural_gradient: 1 ... {backend.MPS_SAMPLED_MAX_N} sites, got {n}")
        if not backend.SCORE_ROWS_MIN_BATCH <= B <= backend.MPS_SAMPLED_MAX_BATCH:
            raise ValueError(f"natural_gradient: {backend.SCORE_ROWS_MIN_BATCH} ... 2^24 samples, got {B}")
        site = 2 * D * D
        site_bytes = site * backend.score_rows_ld(B) * 8
        if self.blocks == "full":
            P = n * site
            if D < 1 or P > MAX_PARAMS:
                raise ValueError(f"natural_gradient blocks='full': {P} parameters (2 n D^2 at n = {n}, D = {D}); the device "
                                 f"solve holds at most {MAX_PARAMS} (use blocks='site')")
            if n * site_bytes > self.rows_budget_bytes:
                raise ValueError(f"natural_gradient blocks='full': the score rows take {n * site_bytes} bytes, more than "
                                 f"rows_budget_bytes = {self.rows_budget_bytes}")
            return P, 1, n
        if D < 1 or site > MAX_PARAMS:
            raise ValueError(f"natural_gradient blocks='site': {site} parameters per site (2 D^2 at D = {D}); the device solve "
                             f"holds at most {MAX_PARAMS} (D <= 22)")
        if site_bytes > self.rows_budget_bytes:
            raise ValueError(f"natural_gradient blocks='site': the score rows of one site take {site_bytes} bytes, more than "
                             f"rows_budget_bytes = {self.rows_budget_bytes}")
        return site, n, min(n, self.rows_budget_bytes // site_bytes)

    def precondition(self, cores, idx, grad):
        """After backend.mps_environments(cores, len(idx)): -> (delta float64 [n, 2, D, D], info int32 [nblocks]); block j of
        delta is (F^_j + damping I)^-1 grad_j, or grad_j bit for bit where info[j] != 0 (backend.spd_solve's codes)."""
        n, D, B = backend._mps_args(cores, int(idx.numel()))
        R, nblocks, chunk = self.plan(n, D, B)
        dev = cores.device
        if tuple(grad.shape) != tuple(cores.shape) or grad.dtype != cores.dtype or grad.device != dev:
            raise ValueError(f"grad: expected float64 {tuple(cores.shape)} on {dev}, got {grad.dtype} {tuple(grad.shape)} on {grad.device}")
        ld = backend.score_rows_ld(B)
        if self.blocks == "site":     # the Gram's partial tiles of a chunk stay within the same budget
            per_site = backend.score_fisher_workspace_bytes(dev, R, 1, ld)
            chunk = max(1, min(chunk, self.rows_budget_bytes // per_site))
        key = (n, D, B, chunk, dev)
        if self._key != key:
            self._rows = torch.empty((chunk, 2 * D * D, ld), dtype=torch.float64, device=dev)
            held = 1 if self.blocks == "full" else chunk
            self._F = torch.empty((held, R, R), dtype=torch.float64, device=dev)
            self._delta = torch.empty((nblocks, R), dtype=torch.float64, device=dev)
            self.info = torch.empty(nblocks, dtype=torch.int32, device=dev)
            self.status = torch.empty(1, dtype=torch.int32, device=dev)
            self._status_chunk = torch.empty(1, dtype=torch.int32, device=dev)
            self._key = key
        g = grad.contiguous().reshape(nblocks, R)
        if self.blocks == "full":
            backend.mps_score_rows(cores, idx, 0, n, out=self._rows, status=self.status)
            backend.score_fisher_gram(self._rows.reshape(1, R, ld), B, out=self._F)
            backend.spd_solve_batched(self._F, g, self.damping, out=self._delta, info=self.info)
        else:
            for k0 in range(0, n, chunk):
                cnt = min(chunk, n - k0)
                st = self.status if k0 == 0 else self._status_chunk
                backend.mps_score_rows(cores, idx, k0, cnt, out=self._rows[:cnt], status=st)
                if k0:
                    self.status |= st
                backend.score_fisher_gram(self._rows[:cnt], B, out=self._F[:cnt])
                backend.spd_solve_batched(self._F[:cnt], g[k0:k0 + cnt], self.damping, out=self._delta[k0:k0 + cnt],
                                          info=self.info[k0:k0 + cnt])
        return self._delta.reshape(cores.shape), self.info


class SampleSpaceFisherPreconditioner:
    """delta = (F^ + damping I)^-1 O^T w for ALL P = 2 n D^2 parameters at once, solved as a B x B system in sample space
    (module docstring): what SampledFisherPreconditioner(blocks='full') computes, at any P, for B <= 1024 samples.  It
    takes the weights w of the gradient, not the gradient.  It owns T, u, delta, info and status, reused across calls (a
    captured step writes into the same tensors)."""
    MAX_SAMPLES = backend.SAMPLE_GRAM_MAX_BATCH

    def __init__(self, damping=1e-3):
        if isinstance(damping, bool) or not isinstance(damping, (int, float, np.integer, np.floating)) \
                or not np.isfinite(damping) or not damping > 0:
            raise ValueError(f"damping must be a finite number > 0 (repeated samples make the sample-space Gram singular), "
                             f"got {damping!r}")
        self.damping = float(damping)
        self.info = None          # int32 [1] of the last call (backend.spd_solve's codes)
        self.status = None        # int32 [1]: the Gram's and the second score_vjp's status words or-ed
        self._key = None
        self._T = self._u = self._delta = self._logq = self._status_vjp = None

    def plan(self, n, D, B):
        """(B, 1, n): the size of the system, one block, every site at once; every ValueError of the shape is raised here,
        without touching the GPU."""
        n, D, B = int(n), int(D), int(B)
        if not 1 <= n <= backend.MPS_SAMPLED_MAX_N:
            raise ValueError(f"natural_gradient: 1 ... {backend.MPS_SAMPLED_MAX_N} sites, got {n}")
        if not 1 <= D <= backend.MPS_MAX_BOND:
            raise ValueError(f"natural_gradient: bond dimension 1 ... {backend.MPS_MAX_BOND}, got {D}")
        if B < backend.SCORE_ROWS_MIN_BATCH:
            raise ValueError(f"natural_gradient='sample': at least {backend.SCORE_ROWS_MIN_BATCH} samples, got {B}")
        if B > self.MAX_SAMPLES:
            raise ValueError(f"natural_gradient='sample': {B} samples; the device solve holds at most {self.MAX_SAMPLES} "
                             f"(the system is B x B)")
        return B, 1, n

    def precondition_weights(self, cores, idx, w):
        """After backend.mps_environments(cores, len(idx)): -> (delta float64 [n, 2, D, D], info int32 [1]) for the weights
        w float64 [B] of the gradient sum_b w_b grad log q(z_b); where info != 0 the solve left u = w and delta is that
        plain gradient bit for bit."""
        n, D, B = backend._mps_args(cores, int(idx.numel()))
        self.plan(n, D, B)
        dev = cores.device
        if tuple(w.shape) != (B,) or w.dtype != torch.float64 or w.device != dev:
            raise ValueError(f"w: expected float64 ({B},) on {dev}, got {w.dtype} {tuple(w.shape)} on {w.device}")
        key = (n, D, B, dev)
        if self._key != key:
            self._T = torch.empty((B, B), dtype=torch.float64, device=dev)
            self._u = torch.empty(B, dtype=torch.float64, device=dev)
            self._delta = torch.empty(tuple(cores.shape), dtype=torch.float64, device=dev)
            self._logq = torch.empty(B, dtype=torch.float64, device=dev)
            self.info = torch.empty(1, dtype=torch.int32, device=dev)
            self.status = torch.empty(1, dtype=torch.int32, device=dev)
            self._status_vjp = torch.empty(1, dtype=torch.int32, device=dev)
            self._key = key
        backend.mps_score_sample_gram(cores, idx, out=self._T, status=self.status)
        backend.spd_solve(self._T, w.contiguous(), self.damping, out=self._u, info=self.info)
        backend.mps_score_vjp(cores, idx, self._u, out=self._delta, out_logq=self._logq, status=self._status_vjp)
        self.status |= self._status_vjp
        return self._delta, self.info


class CGFisherPreconditioner:
    """delta ~ (F^ + damping I)^-1 grad for ALL P = 2 n D^2 parameters at once by conjugate gradients, F^ never formed
    (module docstring): what SampledFisherPreconditioner(blocks='full') solves, at any P and any number of samples.
    precondition always launches max_iters iterations of mps_score_jvp -> mps_score_vjp -> cg_step, so a captured epoch
    replays; the iterations after rr <= rel_tol^2 rr0 write nothing.  An unconverged delta is returned as it is (info 0:
    every CG iterate from 0 is a descent direction; `relres` says how far it got); info 1 means delta is the plain gradient
    (a non-finite gradient or iterate, or no positive curvature at the first step).  It owns x, r, p, F p, t and the
    scalars, reused across calls (a captured step writes into the same tensors)."""
    MAX_ITERS = 32
    REL_TOL = 1e-6

    def __init__(self, damping=1e-3, max_iters=MAX_ITERS, rel_tol=REL_TOL):
        if isinstance(damping, bool) or not isinstance(damping, (int, float, np.integer, np.floating)) \
                or not np.isfinite(damping) or not damping > 0:
            raise ValueError(f"damping must be a finite number > 0 (F^ is singular along every gauge direction), got {damping!r}")
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or max_iters < 1:
            raise ValueError(f"max_iters must be an integer >= 1, got {max_iters!r}")
        if isinstance(rel_tol, bool) or not isinstance(rel_tol, (int, float, np.integer, np.floating)) \
                or not np.isfinite(rel_tol) or not rel_tol >= 0:
            raise ValueError(f"rel_tol must be a finite number >= 0, got {rel_tol!r}")
        self.damping, self.max_iters, self.rel_tol = float(damping), int(max_iters), float(rel_tol)
        self.info = None          # int32 [1] of the last call: 0, or 1 where delta is the plain gradient
        self.iters = None         # int32 [1]: the iterations the last call took
        self.relres = None        # float64 [1]: sqrt(r^T r / g^T g) of the recurrence at the end of the last call
        self.status = None        # int32 [1]: the jvp's and the vjp's status words or-ed
        self._key = None
        self._x = self._r = self._p = self._Fp = self._t = self._logq = self._state = self._status_vjp = None

    def plan(self, n, D, B):
        """(P, 1, n): the size of the system, one block, every site at once; every ValueError of the shape is raised here,
        without touching the GPU."""
        n, D, B = int(n), int(D), int(B)
        if not 1 <= n <= backend.MPS_SAMPLED_MAX_N:
            raise ValueError(f"natural_gradient: 1 ... {backend.MPS_SAMPLED_MAX_N} sites, got {n}")
        if not 1 <= D <= backend.MPS_MAX_BOND:
            raise ValueError(f"natural_gradient: bond dimension 1 ... {backend.MPS_MAX_BOND}, got {D}")
        if not backend.SCORE_ROWS_MIN_BATCH <= B <= backend.MPS_SAMPLED_MAX_BATCH:
            raise ValueError(f"natural_gradient='cg': {backend.SCORE_ROWS_MIN_BATCH} ... 2^24 samples, got {B}")
        return 2 * n * D * D, 1, n

    def precondition(self, cores, idx, grad):
        """After backend.mps_environments(cores, len(idx)): -> (delta float64 [n, 2, D, D], info int32 [1])."""
        n, D, B = backend._mps_args(cores, int(idx.numel()))
        self.plan(n, D, B)
        dev = cores.device
        if tuple(grad.shape) != tuple(cores.shape) or grad.dtype != cores.dtype or grad.device != dev:
            raise ValueError(f"grad: expected float64 {tuple(cores.shape)} on {dev}, got {grad.dtype} {tuple(grad.shape)} on {grad.device}")
        key = (n, D, B, dev)
        if self._key != key:
            self._x, self._r, self._p, self._Fp = (torch.empty(tuple(cores.shape), dtype=torch.float64, device=dev) for _ in range(4))
            self._t = torch.empty(B, dtype=torch.float64, device=dev)
            self._logq = torch.empty(B, dtype=torch.float64, device=dev)
            self._state = torch.empty(backend.CG_STATE_DOUBLES, dtype=torch.float64, device=dev)
            self.info = torch.empty(1, dtype=torch.int32, device=dev)
            self.iters = torch.empty(1, dtype=torch.int32, device=dev)
            self.relres = torch.empty(1, dtype=torch.float64, device=dev)
            self.status = torch.empty(1, dtype=torch.int32, device=dev)
            self._status_vjp = torch.empty(1, dtype=torch.int32, device=dev)
            self._key = key
        g = grad.contiguous()
        backend.cg_init(g, self._x, self._r, self._p, self._state, self.info)
        for _ in range(self.max_iters):
            backend.mps_score_jvp(cores, idx, self._p, scale=1.0 / B, out=self._t, status=self.status)
            backend.mps_score_vjp(cores, idx, self._t, out=self._Fp, out_logq=self._logq, status=self._status_vjp)
            backend.cg_step(self._Fp, self._x, self._r, self._p, self._state, self.damping, self.rel_tol)
        backend.cg_finish(g, self._x, self._state, self.info, self.iters, self.relres)
        self.status |= self._status_vjp           # both words depend on the samples only: the last iteration's are every one's
        return self._x, self.info
