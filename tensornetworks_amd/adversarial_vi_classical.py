"""Adversarial (KL) variational inference with the classical Born machine on MI355X.

Drop-in for the reference trainer adversarial_vi.py, which is wired to exactly this family (adversarial_vi.py:28): same
constructor and `train` signatures, history keys, printed lines, error messages, best-parameter restore and the forced
`init_method='small_random'` (:27).  The epoch loop, the prior / log p(x|z) tables from the score kernel, the classifier
step, the device-side skip of a NaN / Inf update, the history and the HIP-graph replay are the quantum trainer's
(adversarial_vi.AdversarialVariationalInference, the base class); this module supplies what depends on the family:

  reference Born step (adversarial_vi.py:187-231)               here
  ------------------------------------------------------       ------------------------------------------------------
  born_machine.sample: probs + 1e-10, renormalised,             the same torch calls on the kernel's q
     torch.multinomial, 2^n-tuple lookups per sample              (indices; bits by shifts)
  classifier forward on the samples                              the same, under no_grad
  raw reward, Python-float running baseline, get_log_q_z_x,      bornvi_reinforce_step: one call -> d loss_q / d q,
     loss_q with the entropy bonus, loss_q.backward() down        loss_q, the baseline (float64, on the device) and
     to q (a scatter-add over the samples' indices)               the NaN / Inf flag
  ... and from q to the table or the network's logits            bornvi_born_table_vjp (y = dL/dq, no KSD scaling)
  clip_grad_norm_, optimizer.step()                              the same torch objects (fused Adam reads the flag)

Table mode (conditioning_dim = 0): nothing is read back inside the epoch, and after two eager epochs the epoch is
captured into a HIP graph and replayed (`graph_epochs`, as in the quantum trainer).  MLP mode (conditioning_dim > 0, the
reference run script's configuration): the network stays stock torch.nn in train mode and makes the reference's forwards
in the reference's order -- one for `sample` (no grad), one for `get_log_q_z_x` (with grad) -- so the q the samples come
from and the q whose log enters the loss are different Dropout realisations, as in the reference; the VJP's output goes
into the network through torch.autograd.backward on the logits.  Graph capture is off by default in MLP mode
(`graph_epochs=True` tries it; a failed capture falls back to eager epochs and is recorded in `graph_error`).

Deviations from the reference, shared with the quantum trainer: `history['loss_born_machine']` is NaN for a skipped
epoch and `history['grad_norm_born']` keeps the last applied norm, both as in the reference, but the "NaN or Inf" warning
is printed at the next log point (every num_epochs // 20 epochs) instead of inside the step, because the loss is not
read back before that.
"""
import torch
import torch.nn.utils as nn_utils

from . import backend
from .adversarial_vi import AdversarialVariationalInference as _AdversarialBase
from .born_machine_classical_sim import ClassicalBornMachine
from .stein_utils import tvd_table
from .utils import calculate_tvd

ENTROPY_COEF = 0.01      # reference :219: entropy_bonus = -0.01 log q, subtracted from the loss
Q_FLOOR = 1e-10          # get_log_q_z_x: log(probs.clamp(min=1e-10)), born_machine_classical_sim.py:140-175


class AdversarialVariationalInference(_AdversarialBase):
    def __init__(self, bayesian_network, latent_vars_names, observed_vars_names,
                 born_machine_config, classifier_config, device='cpu'):
        """born_machine_config: keyword arguments of ClassicalBornMachine (use_logits, conditioning_dim, hidden_dims,
        use_layer_norm; init_method is overridden, reference :27).  classifier_config: those of BinaryClassifierMLP."""
        super().__init__(bayesian_network, latent_vars_names, observed_vars_names, born_machine_config,
                         classifier_config, device=device)
        self._log_p_c = self._log_p_c_src = None
        self._grad_buf = None

    def _make_born_machine(self, born_machine_config):
        return ClassicalBornMachine(num_latent_vars=self.num_latent_vars, **born_machine_config)

    def _x_condition(self, x_obs_tensor):
        return x_obs_tensor if self.born_machine.conditioning_dim > 0 else None

    def _sample_idx(self, batch_size, x_obs_tensor):
        """ClassicalBornMachine.sample up to the bit unpacking: one forward (a Dropout draw in MLP mode), probs + 1e-10
        renormalised, torch.multinomial -> int64 [batch]."""
        probs = self.born_machine.get_probabilities(self._x_condition(x_obs_tensor)).detach()
        probs = probs + 1e-10
        probs = probs / probs.sum(dim=-1, keepdim=True)
        return torch.multinomial(probs, batch_size, replacement=True)[0]

    def _sample_from_born(self, batch_size, x_obs_tensor):
        return self._bits(self._sample_idx(batch_size, x_obs_tensor).to(self.device))

    def _current_tvd(self, true_posterior_for_tvd, x_obs_tensor):
        x_condition = self._x_condition(x_obs_tensor)
        if torch.is_tensor(true_posterior_for_tvd):
            with torch.no_grad():
                q_now = self.born_machine.get_probabilities(x_condition).detach().reshape(-1)
            return float(tvd_table(true_posterior_for_tvd.to(q_now.device), q_now))
        return calculate_tvd(true_posterior_for_tvd, self.born_machine.get_prob_dict(x_condition=x_condition))

    def _graph_by_default(self):
        return self.born_machine.conditioning_dim == 0

    def _begin_training(self):
        super()._begin_training()
        # the kernel's in/out scalars live on the compute device (the parameters may be on the CPU)
        self._baseline = torch.zeros(1, dtype=torch.float64, device=self._cdev)
        self._found = torch.zeros(1, dtype=torch.float32, device=self._cdev)
        if self._found.device == self._found_inf.device:
            self._found_inf = self._found.reshape(())        # the tensor the fused optimiser reads: written by the kernel
        self._grad_buf = None

    def _born_step(self, batch_size, x_obs_tensor, with_x, optimizer_born, clip, baseline_decay, first):
        """reference :187-231.  Returns (loss [0-dim], grad norm [0-dim] or None, finite flag [0-dim bool])."""
        bm = self.born_machine
        mode = bm.born_mode
        cdev = self._cdev
        if self._log_p_c_src is not self._log_p_active:
            self._log_p_c = self._log_p_active.to(device=cdev, dtype=torch.float32).contiguous()
            self._log_p_c_src = self._log_p_active
        table = bm.conditioning_dim == 0
        with self._spans("born_forward"):
            with torch.no_grad():
                if table:           # the forwards draw nothing: one launch serves the samples and log q
                    home = bm.params.device
                    w = bm.params.detach().to(cdev).reshape(1, -1)
                    q32, q64, _ = backend.born_table_probs(w, mode, want_entropy=False)
                    probs = q32.to(home) + 1e-10
                    idx = torch.multinomial(probs / probs.sum(dim=-1, keepdim=True), batch_size, replacement=True)[0]
                else:
                    idx = self._sample_idx(batch_size, x_obs_tensor)
                logit_d = self.classifier(self._clf_inputs(self._bits(idx.to(self.device)), x_obs_tensor, with_x)).squeeze(-1)
            if not table:           # the forward of get_log_q_z_x: its own Dropout draw, differentiable
                optimizer_born.zero_grad()
                w_graph, home = bm.kernel_input(bm.raw_params(x_obs_tensor))
                w = w_graph.detach()
                q32, q64, _ = backend.born_table_probs(w, mode, want_entropy=False)
        with self._spans("born_backward"):
            dLdq, loss, found = backend.reinforce_step(
                idx.to(cdev).contiguous(), logit_d.to(device=cdev, dtype=torch.float32).contiguous(), self._log_p_c,
                q32.reshape(-1), self._baseline, first, baseline_decay, ENTROPY_COEF, Q_FLOOR, found_out=self._found)
            if table:
                if self._grad_buf is None:
                    self._grad_buf = torch.empty(1, w.shape[1], dtype=torch.float32, device=cdev)
                g = backend.born_table_vjp(w, q64, mode, y=dLdq.reshape(1, -1), out=self._grad_buf)
                # (the same buffer every step -- a captured epoch writes where the optimiser reads)
                bm.params.grad = g.reshape(bm.params.shape) if home == cdev else g.reshape(bm.params.shape).to(home)
            else:
                g = backend.born_table_vjp(w, q64, mode, y=dLdq.reshape(1, -1))
                torch.autograd.backward([w_graph], [g])
            loss_q = loss.reshape(()).to(self.device)
            finite = (found.reshape(()) == 0).to(self.device)
            params = list(bm.parameters())
            if params[0].is_cuda and optimizer_born.defaults.get("fused"):
                grad_norm_q = nn_utils.clip_grad_norm_(params, clip)
                optimizer_born.found_inf = self._found_inf              # skip the update on the device
                try:
                    optimizer_born.step()
                finally:
                    del optimizer_born.found_inf
            elif bool(finite):
                grad_norm_q = nn_utils.clip_grad_norm_(params, clip)
                optimizer_born.step()
            else:
                grad_norm_q = None
        return loss_q, grad_norm_q, finite
