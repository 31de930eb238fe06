"""KSD variational inference with the classical Born machine on MI355X.

Drop-in for the reference trainer ksd_vi.py: same constructor and `train` signatures, attributes, history keys
(loss_ksd, tvd, grad_norm, entropy), printed messages, early stopping and restore of the best probabilities through
set_fixed_probs.  What changed is where the arithmetic happens:

  reference epoch (ksd_vi.py:102-157)                       here
  ---------------------------------------------------       ---------------------------------------------------------
  q = get_probabilities(); 4^n get_stein_kernel_kp_value    the machine's epoch_forward: q32, q64 and the entropy
     calls in a Python double loop; entropy() forward       y = K_p q, ksd2 = q.y: the quantum trainer's contraction
  loss.backward() through 4^n autograd nodes                the machine's epoch_backward -> the parameters' gradients
  clip_grad_norm_, optimizer.step(), scheduler.step()       the same torch objects (make_optimizer, guarded_update)

The two ends of an epoch belong to the family (born_table_probs / born_table_vjp for the table and the MLP, mps_probs /
mps_vjp for the MPS machine: born_machine_base.EnumeratedBornMachine); the trainer knows the objective only.

S and K_p are built once per train() call by a `stein_operator.SteinOperator` of this trainer's own, the one the quantum
trainer derives from (scores on the GPU; dense Gram up to DENSE_GRAM_MAX_N, matrix-free Kronecker mat-vec beyond).  MLP mode
(conditioning_dim > 0): the network stays stock torch.nn and makes the reference's forwards in its order and number
(loss, entropy, TVD, best-probabilities snapshot: the same Dropout draws); logits -> q and the VJP back onto the logits
are the kernels, once per term, and torch.autograd carries the two logit gradients into the network.  make_optimizer,
apply_grads and guarded_update are plain functions: the sampled trainer (elbo_vi_sampled.py) uses the same ones.
"""
from functools import partial

import numpy as np
import torch
import torch.nn.utils as nn_utils
import torch.optim as optim

from . import paramshift_shard as shard
from .born_machine_classical_sim import ClassicalBornMachine
from .born_machine_mps import MPSBornMachine
from .stein_operator import DENSE_GRAM_MAX_N, SteinOperator      # noqa: F401  (DENSE_GRAM_MAX_N: exported from here too)
from .stein_utils import base_hamming_kernel_torch, tvd_table
from .utils import calculate_tvd


def make_optimizer(parameters, lr_born_machine, num_epochs, use_lr_scheduler=True, optimizer_type="adam",
                   adam_betas=(0.9, 0.999)):
    """The optimiser and scheduler the reference builds (ksd_vi.py:84-93)."""
    if optimizer_type == "adam":
        optimizer_born = optim.Adam(parameters, lr=lr_born_machine, betas=adam_betas)
    else:
        optimizer_born = optim.SGD(parameters, lr=lr_born_machine, momentum=0.9)
    scheduler = None
    if use_lr_scheduler:
        scheduler = optim.lr_scheduler.CosineAnnealingLR(optimizer_born, T_max=num_epochs, eta_min=lr_born_machine / 10)
    return optimizer_born, scheduler


def apply_grads(grads):
    """Puts the epoch's gradients into the parameters' .grad (what loss.backward() does in the reference)."""
    if len(grads) == 1 and grads[0][0].is_leaf:
        p, g = grads[0]
        p.grad = g
    else:
        torch.autograd.backward([t for t, _ in grads], [g for _, g in grads])


def guarded_update(born_machine, optimizer, scheduler, guard_value, grads, gradient_clip_norm, last_grad_norm):
    """An epoch's update (ksd_vi.py:140-157): skipped with the reference's warning when the guarded loss is NaN or Inf,
    else gradients, clip, optimiser and scheduler step.  -> the clipped-from gradient norm, or the last one when skipped."""
    if np.isnan(guard_value) or np.isinf(guard_value):
        print(f"Warning: NaN or Inf loss: {guard_value}. Skipping update.")
        return last_grad_norm
    apply_grads(grads)
    grad_norm = nn_utils.clip_grad_norm_(born_machine.parameters(), gradient_clip_norm)
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return grad_norm


class KSDVariationalInference:
    def __init__(self, bayesian_network, latent_vars_names, observed_vars_names,
                 born_machine_config, base_kernel_length_scale=1.0, device='cpu'):
        """Arguments as the reference's (ksd_vi.py:20-41)."""
        self.bn = bayesian_network
        self.latent_vars_names = latent_vars_names
        self.observed_vars_names = observed_vars_names
        self.num_latent_vars = len(latent_vars_names)
        self.num_observed_vars = len(observed_vars_names)
        self.device = device

        # the reference forces this initialisation whatever the config says (ksd_vi.py:30)
        born_machine_config = {**born_machine_config, 'init_method': 'small_random'}
        # 'family': 'table' (default: the reference's probability table / MLP) or 'mps' (born_machine_mps.py, with 'bond_dim')
        family = born_machine_config.pop('family', 'table')
        if family == 'mps':
            self.born_machine = MPSBornMachine(num_latent_vars=self.num_latent_vars, **born_machine_config).to(device)
        elif family == 'table':
            self.born_machine = ClassicalBornMachine(num_latent_vars=self.num_latent_vars,
                                                     **born_machine_config).to(device)
        else:
            raise ValueError(f"born_machine_config['family'] must be 'table' or 'mps', got {family!r}")

        self.num_possible_latent_states = 2 ** self.num_latent_vars
        self.base_kernel_func = partial(base_hamming_kernel_torch,
                                        num_vars=self.num_latent_vars,
                                        length_scale=base_kernel_length_scale)
        # scores and K_p of one observation on one GPU, and the contraction (ksd2, y = K_p q)
        self._stein = SteinOperator(bayesian_network, latent_vars_names, base_kernel_length_scale, device,
                                    process_group=shard.SOLO)
        self._score_function_cache = self._stein._score_function_cache

    @property
    def all_latent_states_tuples(self):
        """Reference attribute, built on first use (2^n Python tuples)."""
        return self._stein.all_latent_states_tuples

    def _get_precomputed_s_p(self, z_tuple, x_dict):
        """Score vector of one state (reference :43-53), served from the batched device result."""
        return self._stein._get_precomputed_s_p(z_tuple, x_dict)

    def _precompute_all_s_p(self, x_dict):
        """reference :55-60 -- one kernel launch for the scores, plus K_p (dense) once."""
        self._stein._precompute_all_s_p(x_dict)

    # what train() knows of the objective: a trainer with another loss (elbo_vi.py) overrides these and loss_and_grads
    _loss_name = "KSD"           # in the log lines
    _loss_key = 'loss_ksd'       # history key of the loss

    def _prepare_observation(self, x_dict):
        self._precompute_all_s_p(x_dict)

    def make_optimizer(self, lr_born_machine, num_epochs, use_lr_scheduler=True, optimizer_type="adam",
                       adam_betas=(0.9, 0.999)):
        return make_optimizer(self.born_machine.parameters(), lr_born_machine, num_epochs, use_lr_scheduler, optimizer_type,
                              adam_betas)

    apply_grads = staticmethod(apply_grads)

    def loss_and_grads(self, x_condition, entropy_weight):
        """Device part of one epoch: -> (loss_ksd [1] float64, entropy [1], q [2^n] float32 of the loss forward, grads):
        grads = [(tensor, its gradient), ...] for apply_grads.  The entropy is float32 from the table family's kernel and
        float64 from the MPS family; train() only reads it with .item().  Nothing is read back to the host."""
        bm = self.born_machine
        # a machine whose forward draws (the MLP's Dropout) makes the reference's two forwards, loss then entropy(): two
        # different samples; otherwise one forward serves both terms
        two = bm.draws_in_forward
        fwd = bm.epoch_forward(x_condition, want_entropy=not two)
        ksd2, y = self._stein._stein_contract(fwd.q64)
        loss, grads = bm.epoch_backward(fwd, y, ksd2, 0.0 if two else entropy_weight)
        if not two:
            return loss, fwd.entropy, fwd.q32, grads
        fwd_h = bm.epoch_forward(x_condition, want_entropy=True)
        return loss, fwd_h.entropy, fwd.q32, grads + bm.epoch_backward(fwd_h, None, None, entropy_weight)[1]

    def train(self, x_observation_dict, num_epochs, lr_born_machine,
              verbose=True, true_posterior_for_tvd=None,
              use_lr_scheduler=True, gradient_clip_norm=10.0,
              optimizer_type="adam", adam_betas=(0.9, 0.999),
              entropy_weight=0.01, patience=200):
        """Same signature, history keys, messages and return value as the reference (ksd_vi.py:62-216).
        true_posterior_for_tvd may also be a tensor (stein_utils.true_posterior_table): TVD then by tvd_table on the
        device, no dict of 2^n tuples."""
        if self.num_observed_vars > 0 and set(x_observation_dict.keys()) != set(self.observed_vars_names):
            raise ValueError("Keys in x_observation_dict must match self.observed_vars_names.")

        x_obs_list = [x_observation_dict[name] for name in self.observed_vars_names] if self.num_observed_vars > 0 else []
        x_obs_tensor_for_bm = torch.tensor(x_obs_list, dtype=torch.float32, device=self.device)
        bm = self.born_machine

        born_machine_x_condition = None
        if bm.conditioning_dim > 0:
            if self.num_observed_vars == 0:
                raise ValueError("Born machine is conditional but no observed vars specified.")
            if bm.conditioning_dim != self.num_observed_vars:
                raise ValueError("Born machine conditioning_dim must match num_observed_vars.")
            born_machine_x_condition = x_obs_tensor_for_bm

        self._prepare_observation(x_observation_dict)
        optimizer_born, scheduler = self.make_optimizer(lr_born_machine, num_epochs, use_lr_scheduler, optimizer_type,
                                                        adam_betas)

        history = {self._loss_key: [], 'tvd': [], 'grad_norm': [], 'entropy': []}
        best_tvd = float('inf')
        best_epoch = -1
        best_probs = None
        epochs_without_improvement = 0
        grad_norm = None              # the reference's `'grad_norm' in locals()`: the last value set, 0.0 before
        table = torch.is_tensor(true_posterior_for_tvd)
        has_posterior = true_posterior_for_tvd is not None and len(true_posterior_for_tvd) > 0

        def current_tvd():
            if table:
                with torch.no_grad():
                    q_now = bm.get_probabilities(x_condition=born_machine_x_condition).detach().reshape(-1)
                return float(tvd_table(true_posterior_for_tvd.to(q_now.device), q_now))
            return calculate_tvd(true_posterior_for_tvd, bm.get_prob_dict(x_condition=born_machine_x_condition))

        for epoch in range(num_epochs):
            optimizer_born.zero_grad()
            loss_t, entropy_t, q, grads = self.loss_and_grads(born_machine_x_condition, entropy_weight)
            if q.shape[0] != self.num_possible_latent_states:
                raise ValueError(f"Probabilities shape mismatch: {q.shape}")
            ksd_value = float(loss_t.item())             # the epoch's host synchronisation (reference: loss.item())
            entropy_value = float(entropy_t.item())
            # the guard is on the total loss (ksd_vi.py:140-142)
            total = ksd_value - float(np.float32(entropy_weight) * np.float32(entropy_value))
            grad_norm = guarded_update(bm, optimizer_born, scheduler, total, grads, gradient_clip_norm, grad_norm)

            history[self._loss_key].append(ksd_value)
            history['grad_norm'].append(grad_norm.item() if grad_norm is not None else 0.0)
            history['entropy'].append(entropy_value)

            if true_posterior_for_tvd is not None:
                tvd = current_tvd()
                history['tvd'].append(tvd)
                if tvd < best_tvd:
                    best_tvd = tvd
                    best_epoch = epoch
                    epochs_without_improvement = 0
                    with torch.no_grad():
                        best_probs = bm.get_probabilities(x_condition=born_machine_x_condition).squeeze().clone()
                    if verbose and tvd < 0.05:
                        print(f"  -> New best TVD: {tvd:.6f} at epoch {epoch+1}")
                else:
                    epochs_without_improvement += 1
                if epochs_without_improvement > patience and epoch > 300:
                    if verbose:
                        print(f"\nEarly stopping at epoch {epoch+1} (no improvement for {patience} epochs)")
                    break
            else:
                history['tvd'].append(np.nan)

            if verbose and (epoch % max(1, num_epochs // 20) == 0 or epoch == num_epochs - 1):
                log_msg = f"Epoch {epoch+1}/{num_epochs} | {self._loss_name}: {ksd_value:.6f}"
                if scheduler is not None:
                    log_msg += f" | LR: {scheduler.get_last_lr()[0]:.6f}"
                log_msg += f" | Entropy: {entropy_value:.4f}"
                if has_posterior and not np.isnan(history['tvd'][-1]):
                    log_msg += f" | TVD: {history['tvd'][-1]:.6f}"
                print(log_msg)

        # unlike the quantum trainer, the best probabilities are restored whatever `verbose` is (ksd_vi.py:199-214)
        if best_probs is not None:
            if verbose:
                print(f"\nRestoring best probabilities (TVD: {best_tvd:.6f} from epoch {best_epoch+1})")
            bm.set_fixed_probs(best_probs)
            final_tvd = current_tvd()
            if abs(final_tvd - best_tvd) > 1e-6:
                print(f"WARNING: Still have restoration issue! Expected TVD: {best_tvd:.6f}, Got: {final_tvd:.6f}")
            elif verbose:
                print(f"Successfully restored best probabilities! Final TVD: {final_tvd:.6f}")

        return history
