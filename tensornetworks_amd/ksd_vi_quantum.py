"""KSD variational inference with the quantum Born machine on MI355X.

Drop-in for the reference trainer (ksd_vi_quantum.py:18-191): same constructor and `train`
signatures, attributes, history keys, printed messages and update rule.  What changed is where the
arithmetic happens:

  reference epoch body (ksd_vi_quantum.py:110-161)          here
  ------------------------------------------------          -------------------------------------------
  q = pqc(theta)                    1 PennyLane circuit     \\
  N^2 get_stein_kernel_kp_value calls (K_p rebuilt every     } one batched HIP launch sequence:
     epoch although it does not depend on theta)            /  base + 2P shifted circuits (LDS-tiled),
  loss = sqrt(clamp(sum, 1e-12)); loss.backward()              y = K_p q (dense GEMV or Kronecker mat-vec),
     -> autograd over N^2 terms, then 2P PennyLane circuits    loss, grad_p = 1/2 (y/loss).(q+_p - q-_p)
  clip_grad_norm_, optimizer.step(), scheduler.step()       same torch.optim objects

S (scores) and K_p are computed once per `train()` call on the GPU.  With a torch.distributed
process group the 2P shifted circuits are sharded over the ranks (paramshift_shard.py).

Finite shots (qbm_shots=S): the base and the 2P shifted distributions of a step are replaced by histograms of S draws
each (backend.shots_histogram, every row its own draws) before the contraction; loss sqrt(max(q^T K_p q^, 1e-12)) and
gradient 1/2 dL/dq^ . (q^+_p - q^-_p) are the plug-in estimates PennyLane's parameter-shift rule gives under shots.
"""
from functools import partial

from .quantum_trainer import DeviceAdam, QuantumTrainer, cosine_annealing_lr      # noqa: F401  (exported from here too)
from .stein_operator import DENSE_GRAM_MAX_N, SteinOperator      # noqa: F401  (DENSE_GRAM_MAX_N: exported from here too)
from .stein_utils import base_hamming_kernel_torch


class KSDVariationalInference(QuantumTrainer, SteinOperator):
    """The KSD objective on quantum_trainer.QuantumTrainer's routes and epoch loop; a SteinOperator itself (scores, K_p)."""
    _loss_name = "KSD"           # in the log lines and warnings
    _loss_key = 'loss_ksd'       # history key of the loss
    _extra_keys = ()             # history keys of further per-epoch device scalars (_step_extras)

    def __init__(self,
                 bayesian_network,
                 latent_vars_names: list,
                 observed_vars_names: list,
                 qbm_num_latent_vars: int,
                 qbm_ansatz_layers: int = 1,
                 qbm_conditioning_dim: int = 0,
                 qbm_pennylane_device_name: str = "default.qubit",
                 qbm_ansatz_type: str = "hardware_efficient",
                 qbm_init_method: str = "small_random",
                 base_kernel_length_scale: float = 1.0,
                 pytorch_device: str = 'cpu',
                 *, gram_mode: str = "auto", process_group=None, qbm_shots=None, shot_seed=None, natural_gradient=None):
        """Arguments up to `pytorch_device` are the reference's (ksd_vi_quantum.py:19-30).
        Keyword-only extras: gram_mode in {"auto", "dense", "kron"} (dense Gram matrix vs matrix-free
        Kronecker mat-vec; "auto" = dense up to n = 16); process_group = torch.distributed group over
        which the parameter-shift circuits are sharded (None = default group if initialised;
        paramshift_shard.SOLO = never shard); qbm_shots = S: finite-shot training (every circuit evaluation of a step
        is a histogram of S draws; QuantumBornMachine(shots=...)), shot_seed = the draws' seed (None: one draw from
        torch's global CPU generator; pass the same seed, or seed torch alike, on every rank).  With shots the step
        always runs the un-fused path (fused_dot does not apply: the fused dot has no probabilities to sample); the
        TVD and best-parameter snapshot of train() use the exact q_theta.
        natural_gradient = True, a damping, or a natural_gradient.FisherPreconditioner: the step hands the optimiser
        delta = (F + damping I)^-1 grad, F the classical Fisher matrix of q_theta built from the stored parameter-shift
        rows (always the un-fused path: the fused dot never writes the rows); history['grad_norm'] is then the norm of
        delta and history['natgrad_info'] the solve's status per epoch (0: solved; otherwise delta is the plain
        gradient).  Not with the adjoint engine, finite shots, more than one rank or more than 1024 parameters.
        natural_gradient = "quantum" or a natural_gradient.QuantumFisherPreconditioner: delta = (Q + damping I)^-1 grad
        with Q the quantum Fisher information (4 x the Fubini-Study metric) built from the P + 1 statevectors; the step
        keeps the gradient route it would take otherwise (fused dot, stored rows or the adjoint engine).  Not with
        finite shots, more than one rank, more than 1024 parameters or statevectors beyond the workspace cap."""
        QuantumTrainer.__init__(self, latent_vars_names, observed_vars_names, qbm_num_latent_vars, qbm_ansatz_layers,
                                qbm_conditioning_dim, qbm_pennylane_device_name, qbm_ansatz_type, qbm_init_method,
                                pytorch_device, process_group, qbm_shots, shot_seed, natural_gradient)
        SteinOperator.__init__(self, bayesian_network, latent_vars_names, base_kernel_length_scale, pytorch_device, gram_mode,
                               process_group)
        self.base_kernel_func = partial(base_hamming_kernel_torch,
                                        num_vars=self.num_latent_vars,
                                        length_scale=base_kernel_length_scale)

    def _prepare_observation(self, x_dict):
        self._precompute_all_s_p(x_dict)

    def _objective_device(self):
        return self._S.device        # (requires _prepare_stein: train() calls it)

    def _contract(self, q):
        with self._timed("stein"):
            ksd2, y = self._stein_contract(q)
        return y, ksd2, None

    def _objective_and_grad(self, **kw):
        """The device part of one epoch -> (loss [1] float64, grad [P] float64, q [2^n])."""
        return self.ksd_and_grad(**kw)

    def _step_extras(self):
        """Device scalars of the step just enqueued, one per _extra_keys entry."""
        return self._natgrad_extras()

    ksd_and_grad = QuantumTrainer.loss_and_grad
