"""Exact-ELBO (reverse-KL) variational inference with the quantum Born machine on MI355X.

  L(theta) = sum_z q_theta(z) [log q_theta(z) - log p(x, z)] = KL(q_theta || p(.|x)) - log p(x)

evaluated and differentiated exactly in O(2^n) per epoch: the circuit engine already holds q_theta for all 2^n states and
the score kernel p(x, z) for all of them (elbo_objective.ElboObjective).  No reference counterpart: the reference reaches
the same quantity through a classifier and REINFORCE (adversarial_vi.py).  An epoch is the KSD trainer's epoch with the
K_p contraction replaced by one pass over 2^n doubles (bornvi_elbo_weights: loss, entropy, w = dL/dq): no Gram matrix,
no scores.  The gradient routes and the epoch loop are quantum_trainer.QuantumTrainer's; this class is the objective.
Finite shots are not offered: a plug-in log of a histogram is biased and unbounded at empty bins (the sample-based
route to KL is the adversarial trainer).
"""
from .elbo_objective import ElboObjective
from .quantum_trainer import QuantumTrainer


class ELBOVariationalInference(QuantumTrainer):
    _loss_name = "ELBO"
    _loss_key = 'loss_elbo'
    _extra_keys = ('entropy',)

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
                 pytorch_device: str = 'cpu',
                 *, p_floor: float = 1e-30, process_group=None, natural_gradient=None):
        """The KSD quantum trainer's arguments without the kernel's length scale, the Gram mode and the shots.
        p_floor: log p(x, z) is log max(p(x, z), p_floor) (states the network gives probability zero stay finite);
        process_group: as there (the shifted circuits are sharded over its ranks); natural_gradient: as there (the step
        is (F + damping I)^-1 grad, the textbook optimiser for the KL; always the stored-rows route -- or, with "quantum",
        (Q + damping I)^-1 grad on whichever route the step takes)."""
        super().__init__(latent_vars_names, observed_vars_names, qbm_num_latent_vars, qbm_ansatz_layers,
                         qbm_conditioning_dim, qbm_pennylane_device_name, qbm_ansatz_type, qbm_init_method,
                         pytorch_device, process_group, natural_gradient=natural_gradient)
        self.bn = bayesian_network
        self.objective = ElboObjective(bayesian_network, latent_vars_names, pytorch_device, p_floor=p_floor)
        self._entropy = None         # entropy [1] of the last elbo_and_grad (device)

    # ---- the objective's side of QuantumTrainer's step and epoch loop ----------------------------------------
    def _prepare_observation(self, x_dict):
        print("Precomputing log p(x,z)...")
        self.objective.prepare(x_dict)
        print("log p(x,z) precomputed.")

    def _objective_device(self):
        if self.objective.log_p is None:
            raise ValueError("elbo_and_grad before objective.prepare(x_dict) (train() calls it)")
        return self.objective.log_p.device

    def _contract(self, q):
        with self._timed("elbo"):
            loss, self._entropy, w = self.objective.weights(q)
        return w, None, loss

    def _objective_and_grad(self, **kw):
        return self.elbo_and_grad(**kw)

    def _step_extras(self):
        return (self._entropy,) + self._natgrad_extras()

    elbo_and_grad = QuantumTrainer.loss_and_grad
    elbo_and_grad_local = QuantumTrainer.loss_and_grad_local

    def train(self, x_observation_dict, num_epochs, lr_born_machine,
              verbose=True, true_posterior_for_tvd=None,
              use_lr_scheduler=True, gradient_clip_norm=10.0,
              optimizer_type="adam", adam_betas=(0.9, 0.999), *, host_sync=True):
        """QuantumTrainer.train(): the KSD quantum trainer's arguments, messages (the loss is labelled ELBO) and read-back
        modes.  History: loss_elbo (= L), kl (= L + log p(x) = KL(q || p(.|x)) before the epoch's update), entropy (of
        that q), tvd, grad_norm; with natural_gradient also natgrad_info."""
        history = super().train(x_observation_dict, num_epochs, lr_born_machine, verbose, true_posterior_for_tvd,
                                use_lr_scheduler, gradient_clip_norm, optimizer_type, adam_betas, host_sync=host_sync)
        history['kl'] = [v + self.objective.log_evidence for v in history['loss_elbo']]
        return history
