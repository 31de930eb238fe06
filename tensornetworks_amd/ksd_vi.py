"""KSD variational inference with the classical Born machine on MI355X.

Drop-in for the reference trainer ksd_vi.py: same constructor and `train` signatures, attributes, history keys
(loss_ksd, tvd, grad_norm, entropy), printed messages, early stopping and restore of the best probabilities through
set_fixed_probs.  What changed is where the arithmetic happens:

  reference epoch (ksd_vi.py:102-157)                       here
  ---------------------------------------------------       ---------------------------------------------------------
  q = get_probabilities(); 4^n get_stein_kernel_kp_value    born_table_probs: q32, q64 and the entropy in one launch
     calls in a Python double loop; entropy() forward       y = K_p q, ksd2 = q.y: the quantum trainer's contraction
  loss.backward() through 4^n autograd nodes                born_table_vjp -> params.grad (float32)
  clip_grad_norm_, optimizer.step(), scheduler.step()       the same torch objects

S and K_p are built once per train() call by a `stein_operator.SteinOperator` of this trainer's own, the one the quantum
trainer derives from (scores on the GPU; dense Gram up to DENSE_GRAM_MAX_N, matrix-free Kronecker mat-vec beyond).  MLP mode
(conditioning_dim > 0): the network stays stock torch.nn and makes the reference's forwards in its order and number
(loss, entropy, TVD, best-probabilities snapshot: the same Dropout draws); logits -> q and the VJP back onto the logits
are the kernels, once per term, and torch.autograd carries the two logit gradients into the network.
"""
from functools import partial

import numpy as np
import torch
import torch.nn.utils as nn_utils
import torch.optim as optim

from . import backend
from . import paramshift_shard as shard
from .born_machine_classical_sim import ClassicalBornMachine
from .born_machine_mps import MPSBornMachine
from .stein_operator import DENSE_GRAM_MAX_N, SteinOperator      # noqa: F401  (DENSE_GRAM_MAX_N: exported from here too)
from .stein_utils import base_hamming_kernel_torch, tvd_table
from .utils import calculate_tvd


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
        """The optimiser and scheduler the reference builds (ksd_vi.py:84-93)."""
        if optimizer_type == "adam":
            optimizer_born = optim.Adam(self.born_machine.parameters(), lr=lr_born_machine, betas=adam_betas)
        else:
            optimizer_born = optim.SGD(self.born_machine.parameters(), lr=lr_born_machine, momentum=0.9)
        scheduler = None
        if use_lr_scheduler:
            scheduler = optim.lr_scheduler.CosineAnnealingLR(optimizer_born, T_max=num_epochs, eta_min=lr_born_machine / 10)
        return optimizer_born, scheduler

    def loss_and_grads(self, x_condition, entropy_weight):
        """Device part of one epoch: -> (loss_ksd [1] float64, entropy [1], q [2^n] float32 of the loss forward, grads):
        grads = [(tensor, its gradient), ...] for apply_grads.  The entropy is float32 from the table family's kernel and
        float64 from the MPS family (mps_entropy_term); train() only reads it with .item().  Nothing is read back to the
        host."""
        bm = self.born_machine
        if isinstance(bm, MPSBornMachine):
            cores, q32, q64 = self.mps_forward()
            ksd2, y = self._stein._stein_contract(q64)
            # loss = sqrt(max(ksd2, 1e-12)); the clamp passes no gradient below 1e-12 (bornvi_born_table_vjp's convention)
            loss = torch.sqrt(ksd2.clamp(min=1e-12))
            g = torch.where(ksd2 >= 1e-12, y / loss, torch.zeros_like(y))
            H, dH = self.mps_entropy_term(q64)
            if entropy_weight != 0.0:
                g = g + entropy_weight * dH
            return loss, H, q32, self.mps_backward(cores, g)
        mode = bm.born_mode
        st = self._stein
        if bm.conditioning_dim == 0:
            # table: the forwards draw nothing, so one launch serves the loss and the entropy
            home = bm.params.device
            w = bm.params.detach().to(backend.compute_device(home)).reshape(1, -1)
            q32, q64, H = backend.born_table_probs(w, mode, want_entropy=True)
            ksd2, y = st._stein_contract(q64[0])
            loss = torch.empty(1, dtype=torch.float64, device=w.device)
            g = backend.born_table_vjp(w, q64, mode, y=y.reshape(1, -1), ksd2=ksd2, entropy_weight=entropy_weight,
                                       loss_out=loss)
            return loss, H, q32[0], [(bm.params, g.reshape(bm.params.shape).to(home))]
        # MLP: the reference's two forwards (loss, then entropy()) -- with Dropout active two different samples
        w1, _ = bm.kernel_input(bm.raw_params(x_condition))
        if w1.shape[0] != 1:
            raise ValueError(f"Probabilities shape mismatch: {tuple(w1.shape)}")
        q32, q64, _ = backend.born_table_probs(w1.detach(), mode, want_entropy=False)
        ksd2, y = st._stein_contract(q64[0])
        loss = torch.empty(1, dtype=torch.float64, device=w1.device)
        g1 = backend.born_table_vjp(w1.detach(), q64, mode, y=y.reshape(1, -1), ksd2=ksd2, loss_out=loss)
        w2, _ = bm.kernel_input(bm.raw_params(x_condition))
        _, q64e, H = backend.born_table_probs(w2.detach(), mode, want_entropy=True)
        g2 = backend.born_table_vjp(w2.detach(), q64e, mode, entropy_weight=entropy_weight)
        return loss, H, q32[0], [(w1, g1), (w2, g2)]

    # ---- the MPS family's ends of an epoch (shared with the ELBO trainer): cores -> q, and dL/dq -> the cores' gradient
    def mps_forward(self):
        """(cores float64 on the compute device, q32 [2^n], q64 [2^n]); leaves the sweep in the workspace for mps_backward."""
        bm = self.born_machine
        cores = bm.cores.detach().to(device=backend.compute_device(bm.cores.device), dtype=torch.float64).contiguous()
        q32, q64, _, _ = backend.mps_probs(cores)
        return cores, q32, q64

    @staticmethod
    def mps_entropy_term(q64):
        """(H [1] = -sum q log max(q, 1e-10), the derivative of -H: log max(q, 1e-10) + [q >= 1e-10]) in float64."""
        logq = torch.log(q64.clamp(min=1e-10))
        return -(q64 * logq).sum().reshape(1), logq + (q64 >= 1e-10).to(torch.float64)

    def mps_backward(self, cores, g):
        bm = self.born_machine
        grad = backend.mps_vjp(cores, g.contiguous())
        return [(bm.cores, grad.to(device=bm.cores.device, dtype=bm.cores.dtype))]

    @staticmethod
    def apply_grads(grads):
        """Puts the epoch's gradients into the parameters' .grad (what loss.backward() does in the reference)."""
        if len(grads) == 1 and grads[0][0].is_leaf:
            p, g = grads[0]
            p.grad = g
        else:
            torch.autograd.backward([t for t, _ in grads], [g for _, g in grads])

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
            if np.isnan(total) or np.isinf(total):
                print(f"Warning: NaN or Inf loss: {total}. Skipping update.")
            else:
                self.apply_grads(grads)
                grad_norm = nn_utils.clip_grad_norm_(bm.parameters(), gradient_clip_norm)
                optimizer_born.step()
                if scheduler is not None:
                    scheduler.step()

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
