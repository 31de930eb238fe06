"""MMD training of the classical Born machines from data on MI355X: the probability table, the MLP-conditioned machine and
the enumerated MPS ({'family': 'mps'}).  DESIGN.md section 6q.

  L = MMD^2(q, p^) = (q - p^)^T K (q - p^),   K a mixture kernel of the Hamming distance

An epoch is the classical ELBO trainer's with the objective swapped:

  the machine's epoch_forward: q32, float64 q64 and the entropy
  objective.weights(q64): L and w = dL/dq = 2 K (q - p^)     two Walsh-Hadamard transforms of 2^n doubles (bornvi_mmd_weights)
  the machine's epoch_backward(y = w, ksd2 = None)           y is then dL/dq itself (born_table_vjp or mps_vjp)

train() -- optimiser, clip, guard, early stopping, restore of the best probabilities -- is the classical KSD trainer's own
code; its Stein side is never prepared.  There is no Bayesian network: the data are bit rows, indices or a probability table, and
the MLP machine's input is one fixed `condition` given at construction."""
from .ksd_vi import KSDVariationalInference
from .mmd_objective import MMDObjective


class ClassicalMMDTrainer(KSDVariationalInference):
    _loss_name = "MMD2"
    _loss_key = 'loss_mmd2'

    def __init__(self, num_vars, born_machine_config, device='cpu', *, length_scales=(0.25, 1.0, 4.0), condition=None):
        """born_machine_config: the classical KSD trainer's (table modes, the MLP, {'family': 'mps', 'bond_dim': D}).
        condition: the MLP's input, conditioning_dim numbers (required exactly when conditioning_dim > 0): one fixed
        context, the place the observation has in the other trainers."""
        objective = MMDObjective(num_vars, length_scales, device)        # (checks num_vars and the length scales)
        if objective.num_vars > 30:
            raise ValueError(f"num_vars must be in 1 ... 30 for an enumerated machine, got {num_vars!r}")
        cdim = dict(born_machine_config).get('conditioning_dim', 0)
        cond = [] if condition is None else [float(c) for c in condition]
        if len(cond) != cdim:
            raise ValueError(f"condition: conditioning_dim = {cdim} numbers expected, got {len(cond)}")
        names = [f"z{i}" for i in range(objective.num_vars)]
        super().__init__(None, names, [f"x{i}" for i in range(cdim)], dict(born_machine_config), device=device)
        self.objective = objective
        self.condition = dict(zip(self.observed_vars_names, cond))
        self._data = None

    def _prepare_observation(self, x_dict):
        self.objective.prepare(self._data)

    def loss_and_grads(self, x_condition, entropy_weight=0.0):
        """Device part of one epoch: -> (loss [1] float64 = L, entropy [1], q [2^n] float32, grads): the gradient is that of
        L - entropy_weight * H.  Nothing is read back to the host.  One forward per epoch."""
        fwd = self.born_machine.epoch_forward(x_condition, want_entropy=True)
        loss, dldq = self.objective.weights(fwd.q64)
        return loss, fwd.entropy, fwd.q32, self.born_machine.epoch_backward(fwd, dldq, None, entropy_weight)[1]

    def train(self, data, num_epochs, lr_born_machine, verbose=True, target_for_tvd=None, use_lr_scheduler=True,
              gradient_clip_norm=10.0, optimizer_type="adam", adam_betas=(0.9, 0.999), entropy_weight=0.0, patience=200):
        """The classical KSD trainer's train() with the data in place of the observation.  History: loss_mmd2, entropy,
        tvd (against target_for_tvd, a table [2^n] or the reference's dict), grad_norm."""
        self._data = data
        return super().train(self.condition, num_epochs, lr_born_machine, verbose, target_for_tvd, use_lr_scheduler, gradient_clip_norm,
                             optimizer_type, adam_betas, entropy_weight, patience)
