"""Exact-ELBO (reverse-KL) variational inference with the quantum Born machine on MI355X.

  L(theta) = sum_z q_theta(z) [log q_theta(z) - log p(x, z)] = KL(q_theta || p(.|x)) - log p(x)

evaluated and differentiated exactly in O(2^n) per epoch: the circuit engine already holds q_theta for all 2^n states and
the score kernel p(x, z) for all of them (elbo_objective.ElboObjective).  No reference counterpart: the reference reaches
the same quantity through a classifier and REINFORCE (adversarial_vi.py).  An epoch is the KSD trainer's epoch with the
K_p contraction replaced by one pass over 2^n doubles (bornvi_elbo_weights: loss, entropy, w = dL/dq):

  fused dot      paramshift_dot_begin -> weights(q) -> paramshift_dot_finish(token, w)        (no Gram matrix, no scores)
  stored rows    paramshift_probs -> weights(q) -> 1/2 w . (q+ - q-) over the stored rows
  adjoint        adjoint_state -> weights(q) -> adjoint_vjp

The epoch loop -- optimiser, clip, NaN/Inf guard, deferred read-backs, HIP-graph replay, sharding of the shifted circuits
over a process group -- is the KSD quantum trainer's own code (this class derives from it and overrides the objective
hooks); its Stein side is never prepared.  Finite shots are not offered: a plug-in log of a histogram is biased and
unbounded at empty bins (the sample-based route to KL is the adversarial trainer).
"""
import torch

from . import backend
from . import paramshift_shard as shard
from .elbo_objective import ElboObjective
from .ksd_vi_quantum import KSDVariationalInference


class ELBOVariationalInference(KSDVariationalInference):
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
        super().__init__(bayesian_network, latent_vars_names, observed_vars_names, qbm_num_latent_vars, qbm_ansatz_layers,
                         qbm_conditioning_dim, qbm_pennylane_device_name, qbm_ansatz_type, qbm_init_method,
                         pytorch_device=pytorch_device, gram_mode="kron", process_group=process_group,
                         natural_gradient=natural_gradient)
        self.objective = ElboObjective(bayesian_network, latent_vars_names, pytorch_device, p_floor=p_floor)
        self._entropy = None         # entropy [1] of the last elbo_and_grad (device)

    # ---- the objective hooks of the inherited epoch loop ---------------------------------------------------
    def _prepare_observation(self, x_dict):
        print("Precomputing log p(x,z)...")
        self.objective.prepare(x_dict)
        print("log p(x,z) precomputed.")

    def _objective_and_grad(self, **kw):
        return self.elbo_and_grad(**kw)

    def _step_extras(self):
        return (self._entropy,) + self._natgrad_extras()

    def ksd_and_grad(self, theta64=None):
        raise backend.BornviError("the ELBO trainer has no Stein side: use elbo_and_grad")

    # ---- one ELBO-gradient step on the device ---------------------------------------------------------------
    def elbo_and_grad(self, theta64=None):
        """The device part of one epoch for the current theta: (loss [1] float64 = L(theta), grad [P] float64, q [2^n]),
        all on the GPU.  Requires objective.prepare(x) (train() calls it)."""
        bm = self.born_machine
        if theta64 is None:
            theta64 = bm.theta.detach().to(device=self.objective.log_p.device, dtype=torch.float64).contiguous()
        P = theta64.numel()
        rank, ws = shard.world(self.process_group)
        lo, hi, step = shard.shard_params(P, rank, ws)
        loss, grad_local, q = self.elbo_and_grad_local(theta64, lo, hi, step)
        if self.grad_engine == "adjoint":       # every rank computes the whole gradient (nothing to shard)
            return loss, grad_local, q
        with self._timed("allgather"):
            grad = shard.all_gather_grad(grad_local, P, self.process_group)
        return loss, grad, q

    def elbo_and_grad_local(self, theta64, lo, hi, step):
        """One rank's part: (loss [1], the gradient entries of the parameters range(lo, hi, step), q).  With the adjoint
        engine the whole gradient, whatever the range."""
        if self.objective.log_p is None:
            raise ValueError("elbo_and_grad before objective.prepare(x_dict) (train() calls it)")
        bm = self.born_machine
        n, L, at = self.num_latent_vars, bm.ansatz_layers, bm.ansatz_type
        dev = theta64.device
        n_local = len(range(lo, hi, step))
        if self.grad_engine == "adjoint":
            with self._timed("circuits"):
                state, q = backend.adjoint_state(at, n, L, theta64)
            with self._timed("elbo"):
                loss, self._entropy, w = self.objective.weights(q)
            with self._timed("finish"):
                grad = backend.adjoint_vjp(at, n, L, theta64, state, w)
            return loss, self._quantum_precondition(theta64, grad), q
        if self.grad_engine != "paramshift":
            raise ValueError("grad_engine must be 'paramshift' or 'adjoint'")
        if not self._rows_needed() and self.fused_dot and backend.paramshift_dot_supported(at, n, L, dev, n_local):
            # base circuit and all but the last pass of the shifted ones -> q -> w -> the shifted circuits' last pass
            # dotted with w: their probabilities are never written or re-read
            with self._timed("circuits"):
                q, token = backend.paramshift_dot_begin(at, n, L, theta64, lo, hi, p_stride=step)
            with self._timed("elbo"):
                loss, self._entropy, w = self.objective.weights(q)
            with self._timed("finish"):
                _, grad = backend.paramshift_dot_finish(token, w)
            return loss, self._quantum_precondition(theta64, grad), q      # (one rank with a preconditioner: local = whole)
        with self._timed("circuits"):
            probs = backend.paramshift_probs(at, n, L, theta64, lo, hi, include_base=True, p_stride=step)
        q = probs[0]
        with self._timed("elbo"):
            loss, self._entropy, w = self.objective.weights(q)
        with self._timed("finish"):
            grad = backend.shifted_dot(n, probs[1:], n_local, w)
        if self._rows_needed():       # (one rank: probs[1:] holds every parameter's rows)
            with self._timed("natgrad"):
                grad, self._natgrad_info = self.natural_gradient.precondition(probs[1:], q, grad)
        return loss, self._quantum_precondition(theta64, grad), q

    def train(self, x_observation_dict, num_epochs, lr_born_machine,
              verbose=True, true_posterior_for_tvd=None,
              use_lr_scheduler=True, gradient_clip_norm=10.0,
              optimizer_type="adam", adam_betas=(0.9, 0.999), *, host_sync=True):
        """The KSD quantum trainer's train(): same arguments, messages (the loss is labelled ELBO) and read-back modes.
        History: loss_elbo (= L), kl (= L + log p(x) = KL(q || p(.|x)) before the epoch's update), entropy (of that q),
        tvd, grad_norm; with natural_gradient also natgrad_info."""
        history = super().train(x_observation_dict, num_epochs, lr_born_machine, verbose, true_posterior_for_tvd,
                                use_lr_scheduler, gradient_clip_norm, optimizer_type, adam_betas, host_sync=host_sync)
        history['kl'] = [v + self.objective.log_evidence for v in history['loss_elbo']]
        return history
