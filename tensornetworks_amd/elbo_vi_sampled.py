"""Sampled reverse-KL (negative ELBO) variational inference with the MPS Born machine: no 2^n object at any n <= 63.

  L = E_{z ~ q} [log q(z) - log p(x, z)] = KL(q || p(.|x)) - log p(x)

estimated from B exact samples per epoch, with the score-function gradient
  grad L = E[(f - b) grad log q],  f = log q - log p,  b the leave-one-out mean (unbiased):  w_b = (f_b - mean f) / (B - 1).
An epoch (sampled_trainer.SampledTrainer owns it): mps_environments, mps_sample (idx, log q), bn_logjoint_samples (log p),
the mean and w as torch elementwise ops on B doubles, mps_score_vjp -> cores.grad; then the guarded update.
born_machine_config['cores'] = 'complex' trains a ComplexSampledMPSBornMachine through the cmps_* calls instead (bond_dim <= 16;
the enumerated report then covers n <= 20).

log p floors every CPT FACTOR at p_floor, where elbo_objective.ElboObjective floors the product p(x, z): at n = 60 a
legitimate joint lies far below 1e-30.  The two agree whenever no factor is below the floor and the product is >= p_floor.
Networks with summed-out nodes are refused (the enumerated trainers handle them).
"""
from . import backend
from .sampled_trainer import SampledTrainer


class SampledELBOVariationalInference(SampledTrainer):
    """History: loss_elbo (the estimate of L), grad_norm, logq_mean, status, and for n <= 26 with a posterior: tvd and kl."""
    LOSS_KEYS = ('loss_elbo',)

    def log_joint(self, idx):
        """log p(x, z_b) of outcome indices, every factor floored at p_floor: float64 [B] on the compute device."""
        return backend.bn_logjoint_samples(self._desc[1], self.num_latent_vars, idx, self.p_floor)

    def sample_weights(self, idx, logq):
        """(loss [] = mean f, w [B])."""
        B = self.num_samples
        logp = self.log_joint(idx)
        f = logq - logp
        loss = f.mean()
        w = (f - loss) / (B - 1) if B > 1 else f.clone()
        return loss, w

    def record_loss(self, history, loss):
        history['loss_elbo'].append(loss)

    def describe(self, loss):
        return f"ELBO (sampled): {loss:.6f}"
