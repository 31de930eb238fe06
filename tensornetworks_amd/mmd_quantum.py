"""MMD training of the quantum Born machine from data on MI355X.

  L(theta) = MMD^2(q_theta, p^) = (q_theta - p^)^T K (q_theta - p^),   K a mixture kernel of the Hamming distance

exact in O(n 2^n) per epoch: the circuit engine holds q_theta for all 2^n states, and K is diagonal under the Walsh-Hadamard
transform (mmd_objective.MMDObjective, bornvi_mmd_weights).  An epoch is the ELBO trainer's epoch with the objective
swapped: w = dL/dq = 2 K (q - p^) is the weight vector the gradient routes consume (fused parameter-shift dot, stored rows,
adjoint); the routes, the epoch loop, host_sync=False and the HIP-graph replay are quantum_trainer.QuantumTrainer's.  There is
no Bayesian network: the data are bit rows, indices or a probability table.  Finite shots and natural gradients are not
offered with this objective yet."""
from .mmd_objective import MMDObjective
from .quantum_trainer import QuantumTrainer


class QuantumMMDTrainer(QuantumTrainer):
    _loss_name = "MMD2"
    _loss_key = 'loss_mmd2'
    _extra_keys = ()

    def __init__(self, num_vars: int, qbm_ansatz_layers: int = 1, qbm_ansatz_type: str = "hardware_efficient",
                 qbm_init_method: str = "small_random", pytorch_device: str = 'cpu', *, length_scales=(0.25, 1.0, 4.0),
                 process_group=None, qbm_shots=None, natural_gradient=None):
        """num_vars qubits, the circuit arguments of the other quantum trainers, the kernel's length scales.  Touches neither
        the GPU nor the library."""
        if qbm_shots is not None:
            raise ValueError("qbm_shots is not offered with the MMD objective: the exact q_theta is used")
        if natural_gradient is not None:
            raise ValueError("natural_gradient is not offered with the MMD objective")
        objective = MMDObjective(num_vars, length_scales, pytorch_device)       # (checks num_vars and the length scales)
        if objective.num_vars > 30:
            raise ValueError(f"num_vars must be in 1 ... 30 for an enumerated machine, got {num_vars!r}")
        names = [f"z{i}" for i in range(objective.num_vars)]
        super().__init__(names, [], objective.num_vars, qbm_ansatz_layers, 0, "default.qubit", qbm_ansatz_type, qbm_init_method,
                         pytorch_device, process_group)
        self.objective = objective

    # ---- the objective's side of QuantumTrainer's step and epoch loop ----------------------------------------
    def _prepare_observation(self, data):
        self.objective.prepare(data)

    def _objective_device(self):
        if self.objective.target is None:
            raise ValueError("loss_and_grad before objective.prepare(data) (train() calls it)")
        return self.objective.target.device

    def _contract(self, q):
        with self._timed("mmd"):
            loss, w = self.objective.weights(q)
        return w, None, loss

    def _objective_and_grad(self, **kw):
        return self.loss_and_grad(**kw)

    def _step_extras(self):
        return ()

    def train(self, data, num_epochs, lr_born_machine, verbose=True, target_for_tvd=None, use_lr_scheduler=True,
              gradient_clip_norm=10.0, optimizer_type="adam", adam_betas=(0.9, 0.999), *, host_sync=True):
        """QuantumTrainer.train() with the data in place of the observation: bit rows [N, n], int64 indices [N] or a
        probability table [2^n].  target_for_tvd: a table [2^n] (or the reference's dict) the TVD is reported against.
        History: loss_mmd2 (before the epoch's update), tvd, grad_norm."""
        return super().train(data, num_epochs, lr_born_machine, verbose, target_for_tvd, use_lr_scheduler, gradient_clip_norm,
                             optimizer_type, adam_betas, host_sync=host_sync)
