"""Sampled KSD variational inference with the MPS Born machine: the Stein objective with no 2^n object at any n <= 63.

z_1 ... z_B are the epoch's exact i.i.d. draws from q_theta, kappa_bb' = k_p(z_b, z_b' | x) the reference's Stein kernel
(stein_utils.get_stein_kernel_kp_value):

  r_b = sum_{b' != b} kappa_bb'            b' != b by SAMPLE INDEX: a duplicate state z_b' = z_b is included with k_p(z, z)
  T   = sum_b r_b
  U   = T / (B (B - 1))                    the U-statistic: unbiased for q^T K_p q, the diagonal of K_p included
  m_b = (T - 2 r_b) / ((B - 1)(B - 2))     leave-one-out baseline: the mean of kappa over the pairs without b, independent of z_b
  w_b = (2 / B) (r_b / (B - 1) - m_b)      sum_b w_b = 0
  grad U ~ sum_b w_b grad log q_theta(z_b)    k_p does not depend on theta: the score-function term is the whole gradient

(dropping pairs at Hamming distance 0 instead of by index would bias U).  B >= 3.
An epoch (sampled_trainer.SampledTrainer owns it): mps_environments, mps_sample, bn_score_samples (the Stein score of p at
the samples), stein_pairs_rowsum (r and T: the B^2 n hot path, on the fp64 matrix cores), U, m and w as torch elementwise
ops on B doubles, mps_score_vjp -> cores.grad; then the guarded update.  DESIGN.md section 6h.

objective='ksd2' descends U.  objective='ksd' descends sqrt(U) the way the enumerated trainers do: w is multiplied by
1 / (2 sqrt(U)), and by 0 where U < 1e-12 (their clamp).  That gradient is BIASED (a nonlinear function of an unbiased
estimate, and U may be negative at a small B); 'ksd2' is the unbiased one.

The scores floor every CPT FACTOR at p_floor and have no "p(x, z) < 1e-12 -> zero row" rule (backend.bn_score_samples).
"""
import math

import torch

from . import backend
from .sampled_trainer import SampledTrainer


class SampledKSDVariationalInference(SampledTrainer):
    """History: loss_ksd2 (U: may be negative, not clamped), loss_ksd = sqrt(max(U, 1e-12)), grad_norm, logq_mean, status,
    and for n <= 26 with a posterior: tvd and kl."""
    LOSS_KEYS = ('loss_ksd2', 'loss_ksd')
    MIN_SAMPLES = 3
    MAX_SAMPLES = backend.STEIN_PAIRS_MAX_BATCH
    SAMPLES_RANGE = "3 ... 2^17"

    def __init__(self, bayesian_network, latent_vars_names, observed_vars_names, born_machine_config,
                 base_kernel_length_scale=1.0, device='cpu', p_floor=1e-30, objective='ksd2', natural_gradient=None):
        if objective not in ('ksd2', 'ksd'):
            raise ValueError(f"objective must be 'ksd2' or 'ksd', got {objective!r}")
        ls = base_kernel_length_scale
        if isinstance(ls, bool) or not isinstance(ls, (int, float)) or not math.isfinite(ls) or not ls > 0:
            raise ValueError(f"base_kernel_length_scale must be a positive finite number, got {ls!r}")
        n = len(latent_vars_names)
        if not float(n) * float(ls) >= 1.0:
            raise ValueError(f"the sampled Stein kernel needs num_latent_vars * base_kernel_length_scale >= 1, got {n} * {ls!r}")
        super().__init__(bayesian_network, latent_vars_names, observed_vars_names, born_machine_config, device=device,
                         p_floor=p_floor, natural_gradient=natural_gradient)
        self.base_kernel_length_scale = float(ls)
        self.objective = objective

    def scores(self, idx):
        """Stein score rows of p at outcome indices: float64 [B, n] on the compute device."""
        return backend.bn_score_samples(self._desc[1], self.num_latent_vars, idx, self.p_floor)

    def sample_weights(self, idx, logq):
        """(loss [] = U, w [B])."""
        B = self.num_samples
        S = self.scores(idx)
        r, T = backend.stein_pairs_rowsum(idx, S, self.num_latent_vars, self.base_kernel_length_scale)
        U = T[0] / (B * (B - 1))
        m = (T - 2.0 * r) / ((B - 1) * (B - 2))
        w = (2.0 / B) * (r / (B - 1) - m)
        if self.objective == 'ksd':
            scale = torch.where(U < 1e-12, torch.zeros_like(U), 0.5 / torch.sqrt(U.clamp(min=1e-12)))
            w = w * scale
        return U, w

    def record_loss(self, history, loss):
        history['loss_ksd2'].append(loss)
        history['loss_ksd'].append(math.sqrt(max(loss, 1e-12)))

    def describe(self, loss):
        return f"KSD^2 (sampled): {loss:.6e}"
