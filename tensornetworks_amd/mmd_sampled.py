"""Sampled MMD training of the MPS Born machines from data: no 2^n object at any n <= 63.

  U = Txx / (B (B - 1)) - 2 Txy / (B N) + Tyy / N^2,   unbiased for MMD^2(q, p^) at the machine's q and the data's p^,

from B exact samples per epoch, with score-function weights w_b whose baselines leave the sample out (mmd_objective.py).
An epoch is sampled_trainer.SampledTrainer's: environments, the draw, two pair-count calls (bornvi_hamming_pairs_rowsum:
xor + popcount per pair, integer counts, bitwise reproducible whatever the order of the pairs), elementwise operations on B
doubles, the score gradient, the guarded update.  The epoch names no family: born_machine_config['cores'] = 'complex' trains
the complex-cores machine through the same code.  There is no Bayesian network: the data are bit rows or indices."""
import torch

from . import backend
from .mmd_objective import MMDObjective
from .sampled_trainer import SampledTrainer


class SampledMMDTrainer(SampledTrainer):
    """History: loss_mmd2 (the estimate U), grad_norm, logq_mean, status; with target_for_tvd and n within the enumerated
    limit (26; complex cores 20) also tvd, kl and mmd2_exact = MMD^2(q, p^) of the enumerated q after the epoch's update."""
    LOSS_KEYS = ('loss_mmd2',)
    MIN_SAMPLES = 3
    MAX_SAMPLES = backend.HAMMING_PAIRS_MAX_A
    SAMPLES_RANGE = "3 ... 2^17"

    def __init__(self, num_vars, born_machine_config, device='cpu', *, length_scales=(0.25, 1.0, 4.0), natural_gradient=None):
        """born_machine_config: bond_dim, num_samples (3 ... 2^17), seed, init_method, cores ('real', 'complex', 'purified' with purification_dim, or 'tree')."""
        objective = MMDObjective(num_vars, length_scales, device)        # (checks num_vars and the length scales)
        names = [f"z{i}" for i in range(objective.num_vars)]
        super().__init__(None, names, [], born_machine_config, device=device, natural_gradient=natural_gradient)
        self.objective = objective
        self._mmd2_exact = []

    def _prepare_observation(self, data):
        self.objective.prepare(data)
        if self.objective.data_indices is None:
            raise ValueError("the sampled trainer needs data points (bit rows or indices), not a probability table")
        self._epoch_dev = torch.zeros(1, dtype=torch.int64, device=self.objective.data_indices.device)

    def sample_weights(self, idx, logq):
        return self.objective.sample_weights(idx)

    def record_loss(self, history, loss):
        history['loss_mmd2'].append(loss)

    def describe(self, loss):
        return f"MMD2 (sampled): {loss:.6f}"

    def exact_report(self, posterior):
        if self.objective.target is not None:
            q = self.born_machine.probabilities64().detach().contiguous()
            self._mmd2_exact.append(float(self.objective.weights(q, want_w=False)[0].item()))
        return super().exact_report(posterior)

    def train(self, data, num_epochs, lr_born_machine, verbose=True, target_for_tvd=None, use_lr_scheduler=True,
              gradient_clip_norm=10.0, optimizer_type="adam", adam_betas=(0.9, 0.999), sgd_momentum=0.9):
        """SampledTrainer.train() with the data in place of the observation: bit rows [N, n] or int64 indices [N]."""
        self._mmd2_exact = []
        history = super().train(data, num_epochs, lr_born_machine, verbose, target_for_tvd, use_lr_scheduler, gradient_clip_norm,
                                optimizer_type, adam_betas, sgd_momentum)
        if 'tvd' in history and len(self._mmd2_exact) == len(history['tvd']):
            history['mmd2_exact'] = list(self._mmd2_exact)
        return history
