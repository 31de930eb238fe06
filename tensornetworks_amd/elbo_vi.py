"""Exact-ELBO (reverse-KL) variational inference with the classical Born machine on MI355X.

  L = sum_z q(z) [log q(z) - log p(x, z)] = KL(q || p(.|x)) - log p(x)

for both table modes and the MLP-conditioned machine, exact in O(2^n) per epoch (elbo_objective.ElboObjective holds the
log-joint table).  No reference counterpart: the reference's classical route to KL is the adversarial trainer.  An epoch:

  the machine's epoch_forward: q32 and float64 q64         (as the KSD trainer; born_table_probs or mps_probs)
  objective.weights(q64): L, entropy, w = dL/dq           one pass over 2^n doubles, in place of the K_p contraction
  the machine's epoch_backward(y = w, ksd2 = None)        y is then dL/dq itself (born_table_vjp or mps_vjp)

train() -- optimiser, clip, guard, early stopping, restore of the best probabilities -- is the classical KSD trainer's
own code (this class derives from it and overrides the objective hooks); its Stein side is never prepared.
"""
from .elbo_objective import ElboObjective
from .ksd_vi import KSDVariationalInference


class ELBOVariationalInference(KSDVariationalInference):
    _loss_name = "ELBO"
    _loss_key = 'loss_elbo'

    def __init__(self, bayesian_network, latent_vars_names, observed_vars_names, born_machine_config, device='cpu',
                 *, p_floor=1e-30):
        """The classical KSD trainer's arguments without the kernel's length scale.  p_floor: log p(x, z) is
        log max(p(x, z), p_floor)."""
        super().__init__(bayesian_network, latent_vars_names, observed_vars_names, born_machine_config, device=device)
        self.objective = ElboObjective(bayesian_network, latent_vars_names, device, p_floor=p_floor)

    def _prepare_observation(self, x_dict):
        print("Precomputing log p(x,z)...")
        self.objective.prepare(x_dict)
        print("log p(x,z) precomputed.")

    def loss_and_grads(self, x_condition, entropy_weight=0.0):
        """Device part of one epoch: -> (loss [1] float64 = L, entropy [1] float64 = -sum q log max(q, 1e-10), q [2^n]
        float32, grads): grads = [(tensor, its gradient), ...] for apply_grads.  The gradient is that of
        L - entropy_weight * H (the KSD trainer's entropy bonus; L carries the entropy itself, so 0 is the ELBO).
        Nothing is read back to the host.  One forward per epoch, in MLP mode too."""
        fwd = self.born_machine.epoch_forward(x_condition, want_entropy=False)
        loss, entropy, dldq = self.objective.weights(fwd.q64)
        return loss, entropy, fwd.q32, self.born_machine.epoch_backward(fwd, dldq, None, entropy_weight)[1]

    def train(self, x_observation_dict, num_epochs, lr_born_machine,
              verbose=True, true_posterior_for_tvd=None,
              use_lr_scheduler=True, gradient_clip_norm=10.0,
              optimizer_type="adam", adam_betas=(0.9, 0.999),
              entropy_weight=0.0, patience=200):
        """The classical KSD trainer's train(): same arguments, messages (the loss is labelled ELBO), early stopping and
        restore of the best probabilities.  entropy_weight defaults to 0: the ELBO has its entropy term already.
        History: loss_elbo (= L), kl (= L + log p(x)), entropy, tvd, grad_norm."""
        history = super().train(x_observation_dict, num_epochs, lr_born_machine, verbose, true_posterior_for_tvd,
                                use_lr_scheduler, gradient_clip_norm, optimizer_type, adam_betas, entropy_weight, patience)
        history['kl'] = [v + self.objective.log_evidence for v in history['loss_elbo']]
        return history
