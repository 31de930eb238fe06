"""What the two quantum trainers share: everything of a training run that does not know the objective.

`QuantumTrainer` owns the machine (a QuantumBornMachine and the preconditioner of its gradient), the gradient routes of a
step and the epoch loop around them: optimiser, clip, NaN/Inf guard, deferred read-backs, HIP-graph replay, sharding of
the shifted circuits over a process group.  The routes differ in how the circuits run,

  adjoint        forward walk -> q -> weights -> backward walk (adjoint_vjp)
  fused dot      circuits up to their last pass -> q -> weights -> last pass dotted with them (paramshift_dot_finish)
  stored rows    every row written -> q -> weights -> 1/2 w . (q+ - q-) over the rows  (finite shots: over histograms)

and the objectives only between "q is known" and "the weights are known".  A trainer derives from this class and supplies that piece
(ksd_vi_quantum.py: the Stein contraction; elbo_vi_quantum.py: one pass over 2^n doubles):

  _contract(q) -> (w [2^n], ksd2 [1] or None, loss [1] or None) under an event span of its own.  With ksd2 the finishing
      kernel makes loss = sqrt(max(ksd2, 1e-12)) and scales the gradient by 1 / (2 loss); without, the gradient is
      1/2 w . (q+ - q-) and the loss the one returned
  _objective_device(), _prepare_observation(x), _step_extras(), _loss_name, _loss_key, _extra_keys, and
  _objective_and_grad(**kw), the epoch loop's way to loss_and_grad through the trainer's own name for it
"""
import numpy as np
import torch
import torch.nn.utils as nn_utils
import torch.optim as optim

from . import backend
from . import paramshift_shard as shard
from .natural_gradient import MAX_PARAMS as NATGRAD_MAX_PARAMS, FisherPreconditioner
from .quantum_born_machine import QuantumBornMachine
from .stein_utils import tvd_table
from .utils import calculate_tvd


def cosine_annealing_lr(epoch, base_lr, T_max, eta_min):
    """optim.lr_scheduler.CosineAnnealingLR(T_max, eta_min) after `epoch` scheduler steps (scalar or array): its closed
    form, which its recursive form follows to rounding, beyond T_max as well (both are periodic in 2 T_max)."""
    e = np.asarray(epoch, dtype=np.float64)
    v = np.where(e == 0, base_lr, eta_min + (base_lr - eta_min) * (1.0 + np.cos(np.pi * e / T_max)) / 2.0)
    return v if e.shape else float(v)


class DeviceAdam:
    """optim.Adam(lr, betas) + CosineAnnealingLR(T_max, eta_min) + clip_grad_norm_ + the NaN/Inf guard as ONE launch per
    epoch (backend.clip_adam_step): moments, step count and epoch count live on the device, the schedule is a table the
    kernel indexes with its own epoch count.  For the HIP-graph replay of the latency-bound sizes, where torch's fused
    optimiser, its tensor-valued schedule and the float64 cast of theta were 9 of the step's 15 launches."""

    def __init__(self, theta, lr, betas=(0.9, 0.999), eps=1e-8, T_max=None, eta_min=0.0, capacity=1 << 16):
        if not (theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous()):
            raise backend.BornviError("DeviceAdam needs a contiguous float32 theta on the GPU")
        dev = theta.device
        self.theta, self.base_lr, self.betas, self.eps = theta, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.T_max, self.eta_min, self.capacity = (None if T_max is None else int(T_max)), float(eta_min), int(capacity)
        if theta.grad is None:
            theta.grad = torch.zeros_like(theta)
        self.exp_avg = torch.zeros(theta.numel(), dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)        # [good steps, epochs since the table's start]
        self.theta64 = theta.detach().to(torch.float64).clone()              # the circuits' input, kept current by the kernel
        self.norm = torch.zeros((), dtype=torch.float32, device=dev)
        self.lr_table = torch.empty(self.capacity, dtype=torch.float64, device=dev)
        self.loss_hist = torch.zeros(self.capacity, dtype=torch.float64, device=dev)    # written by the kernel, one entry
        self.norm_hist = torch.zeros(self.capacity, dtype=torch.float32, device=dev)    # per epoch of the window
        self._hist_done = []                 # (losses, norms) of the windows before the current one
        self.epochs = 0                      # epochs run so far (host count)
        self._window = 0                     # epoch of lr_table[0]
        self._fill()

    def lr_at(self, epoch):
        """Learning rate of epoch `epoch` (0-based): CosineAnnealingLR's closed form (periodic beyond T_max, like its
        recursive form), or the constant rate without a schedule."""
        if self.T_max is None:
            shape = np.shape(epoch)
            return np.full(shape, self.base_lr) if shape else self.base_lr
        return cosine_annealing_lr(epoch, self.base_lr, self.T_max, self.eta_min)

    def _fill(self):
        vals = self.lr_at(self._window + np.arange(self.capacity))
        self.lr_table.copy_(torch.from_numpy(np.ascontiguousarray(vals)))

    def step(self, grad64, loss, max_norm):
        """One epoch's hand-off (enqueued on the current stream; capturable).  -> the gradient norm, a device scalar
        owned by this object.  Follow it with advance() on the host."""
        return backend.clip_adam_step(grad64.reshape(-1), max_norm, loss, self.theta.view(-1), self.theta.grad.view(-1),
                                      self.theta64.view(-1), self.exp_avg, self.exp_avg_sq, self.counters, self.lr_table,
                                      self.betas[0], self.betas[1], self.eps, norm_out=self.norm,
                                      loss_history=self.loss_hist, norm_history=self.norm_hist)

    def advance(self):
        """Host side of an epoch (after step() or a replay of it): counts it, and moves the schedule table on when the
        device's epoch count is about to run off its end."""
        self.epochs += 1
        if self.epochs - self._window >= self.capacity:
            self._hist_done.append((self.loss_hist.clone(), self.norm_hist.clone()))
            self._window = self.epochs
            self._fill()
            self.counters[1:].zero_()

    def history(self, begin=0, end=None):
        """(losses float64, gradient norms float32) of epochs [begin, end) as device tensors: what the kernel recorded
        (the reference's per-epoch loss.item() and clip_grad_norm_ values, ksd_vi_quantum.py:163-166)."""
        end = self.epochs if end is None else int(end)
        k = self.epochs - self._window
        losses = torch.cat([c[0] for c in self._hist_done] + [self.loss_hist[:k]])
        norms = torch.cat([c[1] for c in self._hist_done] + [self.norm_hist[:k]])
        return losses[begin:end], norms[begin:end]

    def last_lr(self):
        """What scheduler.get_last_lr()[0] reads after this many epochs: the rate of the next one."""
        return self.lr_at(self.epochs)


class QuantumTrainer:
    """Machine, gradient routes and epoch loop of a quantum trainer; the objective is the deriving class's (module
    docstring: `_contract` and the other hooks)."""

    def __init__(self, latent_vars_names, observed_vars_names, qbm_num_latent_vars, qbm_ansatz_layers,
                 qbm_conditioning_dim, qbm_pennylane_device_name, qbm_ansatz_type, qbm_init_method, pytorch_device,
                 process_group=None, qbm_shots=None, shot_seed=None, natural_gradient=None):
        """The machine side of the quantum trainers' constructors (they document the arguments).  Touches neither the
        GPU nor the library."""
        self.natural_gradient = FisherPreconditioner.coerce(natural_gradient)
        self._natgrad_info = None    # int32 [1] of the last step (device)
        if self.natural_gradient is not None and qbm_shots is not None:
            raise ValueError("natural_gradient with qbm_shots: the Fisher matrix of histograms is biased and unbounded "
                             "at empty bins")
        if int(qbm_num_latent_vars) != len(latent_vars_names):
            # the scores are [2^len(latent_vars_names), len(latent_vars_names)] while the circuit has
            # qbm_num_latent_vars qubits: the device kernels would index one with the other's sizes
            raise ValueError(f"qbm_num_latent_vars ({qbm_num_latent_vars}) must equal len(latent_vars_names) "
                             f"({len(latent_vars_names)})")
        self.latent_vars_names = latent_vars_names
        self.num_latent_vars = len(latent_vars_names)
        self.process_group = process_group
        self.observed_vars_names = observed_vars_names
        self.num_observed_vars = len(observed_vars_names)
        self.pytorch_device = pytorch_device

        self.born_machine = QuantumBornMachine(
            num_latent_vars=self.num_latent_vars,
            ansatz_layers=qbm_ansatz_layers,
            conditioning_dim=qbm_conditioning_dim,
            device_name=qbm_pennylane_device_name,
            ansatz_type=qbm_ansatz_type,
            init_method=qbm_init_method,
            shots=qbm_shots,
            shot_seed=shot_seed
        ).to(pytorch_device)
        self.born_machine.process_group = process_group

        self.num_possible_latent_states = 2 ** self.num_latent_vars
        # Gradient engine.  "paramshift" (default) = the reference's rule: 2P shifted circuit evaluations
        # (diff_method="parameter-shift", quantum_born_machine.py:58).  "adjoint" = OPT-IN extra:
        # one forward and one backward walk over the gates (bornvi_adjoint_state / _vjp) -- the same gradient to
        # rounding from about three circuit evaluations; every rank computes it whole (nothing to shard).
        self.grad_engine = "paramshift"
        if self.natural_gradient is not None:
            P = self.born_machine.num_ansatz_params
            if P > NATGRAD_MAX_PARAMS:
                raise ValueError(f"natural_gradient: {P} parameters; the device solve holds at most {NATGRAD_MAX_PARAMS}")
            if shard.world(process_group)[1] > 1:
                raise ValueError("natural_gradient with a process group of more than one rank: the Fisher matrix needs "
                                 "the cross terms between the ranks' rows")
            if self.natural_gradient.quantum:
                self.natural_gradient.bind(self.born_machine.ansatz_type, self.num_latent_vars, self.born_machine.ansatz_layers, P)
            self._extra_keys = tuple(type(self)._extra_keys) + ('natgrad_info',)
        # The parameter-shift dot product  sum_z dL/dq_z (q+ - q-)(z)  inside the shifted circuits' last pass instead of a
        # pass over their stored probabilities (bornvi_paramshift_dot_begin / _finish): still all 2P circuit evaluations,
        # same gradient to rounding; taken where the library offers it (multi-pass plans of the 8-amplitude kernel),
        # else the probabilities are written and dotted as before.  False: always the un-fused path (A/B).
        self.fused_dot = True
        self.timers = None      # optional {name: [(start_event, end_event), ...]} filled by the step

    def _timed(self, name):
        return backend.EventSpan(self.timers, name)

    @property
    def grad_engine(self):
        return self._grad_engine

    @grad_engine.setter
    def grad_engine(self, engine):
        ng = getattr(self, "natural_gradient", None)
        if engine == "adjoint" and ng is not None and not ng.quantum:
            raise ValueError("natural_gradient with grad_engine = 'adjoint': the adjoint engine has no parameter-shift "
                             "rows to build the Fisher matrix from")
        self._grad_engine = engine

    def _rows_needed(self):
        """True when the step must store the parameter-shift rows: the classical Fisher matrix is built from them."""
        return self.natural_gradient is not None and not self.natural_gradient.quantum

    def _quantum_precondition(self, theta64, grad):
        """grad -> delta under the quantum metric (any gradient route); grad itself without that preconditioner."""
        if self.natural_gradient is None or not self.natural_gradient.quantum:
            return grad
        with self._timed("natgrad"):
            grad, self._natgrad_info = self.natural_gradient.precondition(theta64, grad)
        return grad

    def _natgrad_extras(self):
        """The natural-gradient solve's status of the step just enqueued, as the history's float64 device scalar."""
        return () if self.natural_gradient is None else (self._natgrad_info.to(torch.float64),)

    # Both exist only because the benchmark record reads them: the overlap stream modes were retired.
    overlap_choice = None

    @property
    def overlap_streams(self):
        return False

    @overlap_streams.setter
    def overlap_streams(self, mode):
        if mode is not None and mode is not False:
            raise ValueError(f"overlap_streams = {mode!r}: the overlap stream modes were retired (they measured no gain, "
                             "DESIGN.md section 4.1); commit 47ae535 is the last that has them")

    # ---- one gradient step on the device --------------------------------------------------------------------
    def loss_and_grad(self, theta64=None):
        """Runs the device part of one epoch for the current theta: returns (loss [1] float64 on the GPU,
        grad [P] float64 on the GPU, q [2^n]).  Requires the objective's tables (train() prepares them)."""
        if theta64 is None:
            theta64 = self.born_machine.theta.detach().to(device=self._objective_device(), dtype=torch.float64).contiguous()
        rank, ws = shard.world(self.process_group)
        lo, hi, step = shard.shard_params(theta64.numel(), rank, ws)
        loss, grad, q = self.loss_and_grad_local(theta64, lo, hi, step, True)
        return loss, self._quantum_precondition(theta64, grad), q

    # (`gather` is not part of the one-rank surface: it exists so that the exchange between the ranks happens inside the
    # "finish" span, as the benchmark's phase record expects; only loss_and_grad sets it, and then gets the whole gradient)
    def loss_and_grad_local(self, theta64, lo, hi, step, gather=False):
        """One rank's part: (loss [1], the gradient entries of the parameters range(lo, hi, step), q).  With the adjoint
        engine the whole gradient, whatever the range (nothing to shard).  gather: the ranks' entries are exchanged before
        the "finish" span closes and the whole gradient is returned (loss_and_grad).  Finite shots: the stored rows are
        replaced in place by histograms of S draws keyed by their global circuit ids at the machine's epoch, the epoch is
        advanced on the device (a graph replay draws afresh): (loss estimate, gradient estimate, the exact q)."""
        bm = self.born_machine
        n, L, at = self.num_latent_vars, bm.ansatz_layers, bm.ansatz_type
        dev = self._objective_device()
        n_local = len(range(lo, hi, step))
        shots = bm.shots
        if shots is not None and self.grad_engine != "paramshift":
            raise ValueError("finite shots need grad_engine='paramshift': adjoint gradients are exact")
        if self.grad_engine == "adjoint":
            with self._timed("circuits"):
                state, q = backend.adjoint_state(at, n, L, theta64)
            w, ksd2, loss = self._contract(q)
            with self._timed("finish"):
                if ksd2 is not None:
                    loss, _, w = backend.ksd_grad_finish(n, None, 0, w, ksd2, want_dldq=True)
                grad = backend.adjoint_vjp(at, n, L, theta64, state, w)
            return loss, grad, q
        if self.grad_engine != "paramshift":
            raise ValueError("grad_engine must be 'paramshift' or 'adjoint'")
        token, rows = None, self._rows_needed()
        if shots is None and not rows and self.fused_dot and backend.paramshift_dot_supported(at, n, L, dev, n_local):
            # The dot product with dL/dq fused into the shifted circuits' last pass (kernels_circuit8.hip): base circuit
            # and all but the last pass of the shifted ones -> q -> weights -> last pass of the shifted circuits dotted
            # with them.  Their probabilities are never written or re-read (8 GB each way at n = 20).
            with self._timed("circuits"):
                q, token = backend.paramshift_dot_begin(at, n, L, theta64, lo, hi, p_stride=step)
            w, ksd2, loss = self._contract(q)
        else:
            with self._timed("circuits"):
                probs = backend.paramshift_probs(at, n, L, theta64, lo, hi, include_base=True, p_stride=step)
            q, shifted = probs[0], probs[1:]
            base = q                  # the row the objective sees: a view, so with shots the histogram drawn below
            if shots is not None:
                q = q.clone()
                epoch = bm.shot_epoch(theta64.device)
                with self._timed("shots"):
                    backend.shots_histogram(probs, n, shots, bm.shot_seed, epoch, include_base=True, p_begin=lo,
                                            p_stride=step, out=probs)
                    epoch.add_(1)
            w, ksd2, loss = self._contract(base)
        with self._timed("finish"):
            if token is not None:
                finish_loss, grad = backend.paramshift_dot_finish(token, w, ksd2)
                loss = loss if ksd2 is None else finish_loss
            elif ksd2 is None:
                grad = backend.shifted_dot(n, shifted, n_local, w)
            else:
                loss, grad, _ = backend.ksd_grad_finish(n, shifted, n_local, w, ksd2)
            if gather:
                with self._timed("allgather"):
                    grad = shard.all_gather_grad(grad, theta64.numel(), self.process_group)
        if rows:                      # (one rank: `shifted` holds every parameter's rows)
            with self._timed("natgrad"):
                grad, self._natgrad_info = self.natural_gradient.precondition(shifted, q, grad)
        return loss, grad, q

    def _tvd_probabilities(self, x_condition=None):
        """The distribution train() measures the TVD of: the reference's get_probabilities(), or with shots the exact
        q_theta (an evaluation metric, not a training signal: DESIGN.md section 8)."""
        if self.born_machine.shots is not None:
            return self.born_machine.exact_probabilities()
        return self.born_machine.get_probabilities(x_condition=x_condition)

    def make_optimizer(self, lr_born_machine, num_epochs, use_lr_scheduler=True, optimizer_type="adam",
                       adam_betas=(0.9, 0.999), capturable=False):
        """Optimiser and scheduler exactly as the reference builds them (ksd_vi_quantum.py:92-103).
        capturable=True (Adam on the GPU only): the learning rate lives in a device tensor and the step counter on the
        device, so that the whole step can be replayed from a HIP graph (`make_graphed_step`); same update rule."""
        params = list(self.born_machine.parameters())
        # same optimisers and hyper-parameters as the reference; when theta lives on the GPU the single-kernel
        # ("fused") implementation of the same torch.optim class is selected: identical update rule, ~0.1 ms
        # less host time per step
        fused = {"fused": True} if all(p.is_cuda for p in params) else {}
        if capturable:
            if optimizer_type != "adam" or not fused:
                raise backend.BornviError("a graph-capturable step needs Adam with theta on the GPU")
            fused["capturable"] = True
            lr_born_machine_arg = torch.tensor(float(lr_born_machine), dtype=torch.float32, device=params[0].device)
        else:
            lr_born_machine_arg = lr_born_machine
        if optimizer_type == "adam":
            optimizer_born = optim.Adam(params, lr=lr_born_machine_arg, betas=adam_betas, **fused)
        elif optimizer_type == "sgd":
            optimizer_born = optim.SGD(params, lr=lr_born_machine, momentum=0.9, **fused)
        else:
            optimizer_born = optim.Adam(params, lr=lr_born_machine, **fused)
        scheduler = None
        if use_lr_scheduler:
            scheduler = optim.lr_scheduler.CosineAnnealingLR(optimizer_born, T_max=num_epochs,
                                                             eta_min=lr_born_machine / 10)
        return params, optimizer_born, scheduler

    def training_step_async(self, params, optimizer_born, scheduler, gradient_clip_norm):
        """The same epoch body with NO host synchronisation: returns (loss [1] float64 on the GPU, grad norm 0-dim
        float32 on the GPU, q); the caller reads the values when it needs them (e.g. after K steps), so the GPU runs
        the steps back to back instead of idling while the host handles `loss.item()`.  The NaN/Inf guard of the
        reference (:147-148, "Skipping update") runs on the device: the fused optimiser kernel skips the update
        when `found_inf` is set (the torch.amp.GradScaler mechanism of torch.optim).  One deviation: the LR
        scheduler also advances on such a step (the host cannot know).  Needs theta and a fused optimiser on the GPU."""
        theta = self.born_machine.theta
        if not (theta.is_cuda and theta.dtype == torch.float32 and len(params) == 1 and optimizer_born.defaults.get("fused")):
            raise backend.BornviError("training_step_async needs a float32 theta on the GPU and a fused torch optimiser")
        optimizer_born.zero_grad()
        loss_t, grad64, q = self._objective_and_grad()
        g32, grad_norm, found_inf = backend.clip_cast_grad_guard(grad64, gradient_clip_norm, loss_t)
        theta.grad = g32
        optimizer_born.found_inf = found_inf
        try:
            optimizer_born.step()
        finally:
            del optimizer_born.found_inf
        if scheduler is not None:
            scheduler.step()
        return (loss_t, grad_norm, q) + tuple(self._step_extras())

    @staticmethod
    def _device_adam_for(theta, optimizer_born, scheduler):
        """A DeviceAdam equal to (optimizer_born, scheduler) if they are what make_optimizer builds for "adam" and nothing
        has stepped yet; None otherwise (the torch objects run the update then)."""
        if type(optimizer_born) is not optim.Adam or len(optimizer_born.param_groups) != 1 or len(optimizer_born.state) != 0:
            return None
        g = optimizer_born.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad") or g.get("maximize") or g.get("differentiable"):
            return None
        T_max, eta_min, lr = None, 0.0, float(g["lr"])
        if scheduler is not None:
            if type(scheduler) is not optim.lr_scheduler.CosineAnnealingLR or scheduler.last_epoch != 0:
                return None
            T_max, eta_min, lr = scheduler.T_max, scheduler.eta_min, float(scheduler.base_lrs[0])
        return DeviceAdam(theta, lr, g["betas"], g["eps"], T_max, eta_min)

    def make_graphed_step(self, params, optimizer_born, scheduler, gradient_clip_norm, warmup=3, record=None,
                          device_adam=True):
        """The epoch body of `training_step_async` captured ONCE into a HIP graph (torch.cuda.CUDAGraph: our kernels
        are launched on torch's current stream, so the capture records them together with the cast, the fused Adam
        kernel and the guard) and replayed per step: one graph launch instead of ~15 kernel launches and their host
        work.  For the latency-bound sizes (n <= 13: BASELINE config 2 spends its step in launch overhead, SURVEY
        section 7.4).  Returns step() -> (loss [1], grad_norm, q): tensors OWNED BY THE GRAPH, overwritten by the next
        step (clone what must be kept).  Needs `make_optimizer(..., capturable=True)`; `warmup` eager steps run first
        (they are real optimiser steps).  device_adam (default): clip, guard, Adam, schedule and the float64 cast of
        theta are one launch of ours (`DeviceAdam`; 6 graph nodes at n = 8 instead of 10 plus 6 eager launches per
        step) -- equal to torch's update to rounding; the torch optimiser and scheduler objects are then left untouched,
        `step.adam` is the state and `step.last_lr()` the schedule's rate.  Otherwise (or when the optimiser is not the
        plain Adam + cosine pair of make_optimizer) torch's capturable fused Adam is captured and the scheduler advances
        on the host after each replay (it fills the learning-rate tensor the captured Adam kernel reads)."""
        theta = self.born_machine.theta
        if not (theta.is_cuda and theta.dtype == torch.float32 and len(params) == 1 and optimizer_born.defaults.get("capturable")):
            raise backend.BornviError("make_graphed_step needs a float32 theta on the GPU and make_optimizer(capturable=True)")
        if self.timers is not None:
            raise backend.BornviError("event timers cannot be recorded inside a graph capture: set timers = None")
        dev = theta.device
        if theta.grad is None:
            theta.grad = torch.zeros_like(theta)
        found = torch.zeros((), dtype=torch.float32, device=dev)
        adam = self._device_adam_for(theta, optimizer_born, scheduler) if device_adam else None

        def own_body():
            loss_t, grad64, q = self._objective_and_grad(theta64=adam.theta64)
            return (loss_t, adam.step(grad64, loss_t, gradient_clip_norm), q) + tuple(self._step_extras())

        def torch_body():
            loss_t, grad64, q = self._objective_and_grad()
            # (the clipped gradient and the guard flag are written straight into theta.grad and the flag tensor the fused
            # Adam kernel reads: no copy nodes in the graph)
            _, grad_norm, _ = backend.clip_cast_grad_guard(grad64, gradient_clip_norm, loss_t,
                                                           out=theta.grad.view(grad64.shape), found_out=found)
            optimizer_born.found_inf = found
            try:
                optimizer_born.step()
            finally:
                del optimizer_born.found_inf
            return (loss_t, grad_norm, q) + tuple(self._step_extras())

        body = own_body if adam is not None else torch_body

        def host_advance():
            if adam is not None:
                adam.advance()
            elif scheduler is not None:
                scheduler.step()

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, int(warmup))):      # plans, workspaces and optimiser state exist before the capture
                w = body()                            # (real optimiser steps: `record`, a list, receives their outputs)
                if record is not None:
                    record.append(tuple(t.clone() for t in w))
                host_advance()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = body()

        def step():
            graph.replay()
            host_advance()
            return out

        step.graph = graph
        step.adam = adam
        step.last_lr = (adam.last_lr if adam is not None else
                        (lambda: float(scheduler.get_last_lr()[0])) if scheduler is not None else None)
        step.found_inf = found        # the captured kernels write and read this tensor on every replay: it lives as long
        return step                   # as step() does (freed, its block is handed to the caller's next small tensor)

    def training_step(self, params, optimizer_born, scheduler, gradient_clip_norm):
        """One epoch body (reference :111-161) without the logging: device step, NaN/Inf guard, clip,
        optimiser and scheduler step.  Returns (loss_value, grad_norm or None if skipped, q)."""
        optimizer_born.zero_grad()
        loss_t, grad64, q = self._objective_and_grad()
        loss_value = float(loss_t.item())        # the epoch's one host sync (reference: loss.item(), :163)
        if np.isnan(loss_value) or np.isinf(loss_value):
            return loss_value, None, q
        theta = self.born_machine.theta
        if theta.dtype == torch.float32 and len(params) == 1:
            # cast + clip_grad_norm_ (reference :153) in one device launch; same formula as torch's
            g32, grad_norm = backend.clip_cast_grad(grad64, gradient_clip_norm)
            theta.grad = g32.to(theta.device)
        else:
            theta.grad = grad64.to(device=theta.device, dtype=theta.dtype)
            grad_norm = nn_utils.clip_grad_norm_(params, gradient_clip_norm)
        optimizer_born.step()
        if scheduler is not None:
            scheduler.step()
        return loss_value, grad_norm, q

    def train(self, x_observation_dict, num_epochs, lr_born_machine,
              verbose=True, true_posterior_for_tvd=None,
              use_lr_scheduler=True, gradient_clip_norm=10.0,
              optimizer_type="adam", adam_betas=(0.9, 0.999), *, host_sync=True):
        """Same signature, history keys and messages as the reference (ksd_vi_quantum.py:76-190).
        host_sync (keyword-only extra): True = the reference's epoch, which reads `loss.item()` every epoch.  False =
        the same epochs without host synchronisation (theta on the GPU): `training_step_async` per epoch -- for
        n <= 13 with Adam replayed from ONE HIP graph (`make_graphed_step`) -- with the NaN/Inf guard on the device; losses,
        norms and TVDs stay on the device and are read where the reference prints and once at the end, so a "Skipping
        update" warning appears at the next such point.  Same history."""
        if not host_sync:
            return self._train_deferred(x_observation_dict, num_epochs, lr_born_machine, verbose, true_posterior_for_tvd,
                                        use_lr_scheduler, gradient_clip_norm, optimizer_type, adam_betas)

        if self.num_observed_vars > 0 and set(x_observation_dict.keys()) != set(self.observed_vars_names):
            raise ValueError("Keys in x_observation_dict must match self.observed_vars_names.")

        qbm_x_condition_input = None
        if self.num_observed_vars > 0 and self.born_machine.conditioning_dim > 0:
            x_obs_list_for_qbm = [x_observation_dict[name] for name in self.observed_vars_names]
            qbm_x_condition_input = torch.tensor(x_obs_list_for_qbm, dtype=torch.float32, device=self.pytorch_device)

        self._prepare_observation(x_observation_dict)

        params, optimizer_born, scheduler = self.make_optimizer(lr_born_machine, num_epochs, use_lr_scheduler,
                                                                optimizer_type, adam_betas)

        history = {self._loss_key: [], 'tvd': [], 'grad_norm': [], **{k: [] for k in self._extra_keys}}
        best_tvd = float('inf')
        best_params = None
        grad_norm = None
        log_every = (num_epochs // 10 if num_epochs >= 10 else 1)

        for epoch in range(num_epochs):
            if self.born_machine.conditioning_dim > 0 and qbm_x_condition_input is not None:
                print("Warning: Conditioning with x_condition not fully implemented in PQC ansatz yet.")
            loss_value, step_norm, q = self.training_step(params, optimizer_born, scheduler, gradient_clip_norm)

            if verbose and epoch % log_every == 0:
                print(f"  Epoch {epoch+1} Q Probs (first 4): {q[:4].detach().cpu().numpy()}")

            if q.shape[0] != self.num_possible_latent_states:
                raise ValueError(f"Probabilities from Born machine have unexpected shape")

            if step_norm is None:
                print(f"Warning: NaN or Inf {self._loss_name} loss: {loss_value}. Skipping update.")
            else:
                grad_norm = step_norm
                if verbose and epoch % log_every == 0:
                    print(f"  Epoch {epoch+1} Grad Norm (after clipping): {grad_norm:.4f}")

            history[self._loss_key].append(loss_value)
            history['grad_norm'].append(grad_norm if grad_norm is not None else 0.0)
            for k, v in zip(self._extra_keys, self._step_extras()):
                history[k].append(float(v))

            if true_posterior_for_tvd is not None:
                if torch.is_tensor(true_posterior_for_tvd):
                    # array form (stein_utils.true_posterior_table): no dict of 2^n tuples; like the reference the
                    # distribution AFTER this epoch's update is compared (one more circuit, :168)
                    q_now = self._tvd_probabilities(x_condition=qbm_x_condition_input).detach().squeeze()
                    tvd = float(tvd_table(true_posterior_for_tvd.to(q_now.device), q_now))
                elif self.born_machine.shots is not None:
                    current_q_dist_dict = dict(zip(self.born_machine.all_outcomes_tuples,
                                                   self._tvd_probabilities().cpu().tolist()))
                    tvd = calculate_tvd(true_posterior_for_tvd, current_q_dist_dict)
                else:
                    current_q_dist_dict = self.born_machine.get_prob_dict(x_condition=qbm_x_condition_input)
                    tvd = calculate_tvd(true_posterior_for_tvd, current_q_dist_dict)
                history['tvd'].append(tvd)
                if tvd < best_tvd:
                    best_tvd = tvd
                    best_params = self.born_machine.state_dict()     # aliases the live tensors (quirk Q3)
            else:
                history['tvd'].append(np.nan)

            if verbose and (epoch % max(1, num_epochs // 20) == 0 or epoch == num_epochs - 1):
                log_msg = f"Epoch {epoch+1}/{num_epochs} | {self._loss_name}: {loss_value:.6f}"
                if scheduler is not None:
                    log_msg += f" | LR: {scheduler.get_last_lr()[0]:.6f}"
                if true_posterior_for_tvd is not None and len(true_posterior_for_tvd) and not np.isnan(history['tvd'][-1]):
                    log_msg += f" | TVD: {history['tvd'][-1]:.6f}"
                print(log_msg)

        if best_params is not None and verbose:
            print(f"\nRestoring best parameters (TVD: {best_tvd:.6f})")
            self.born_machine.load_state_dict(best_params)

        return history

    def _train_deferred(self, x_observation_dict, num_epochs, lr_born_machine, verbose, true_posterior_for_tvd,
                        use_lr_scheduler, gradient_clip_norm, optimizer_type, adam_betas):
        """train(host_sync=False): see there.  The epochs are `training_step_async` (or its HIP-graph replay)."""
        if self.num_observed_vars > 0 and set(x_observation_dict.keys()) != set(self.observed_vars_names):
            raise ValueError("Keys in x_observation_dict must match self.observed_vars_names.")
        theta = self.born_machine.theta
        if not (theta.is_cuda and theta.dtype == torch.float32):
            raise backend.BornviError("train(host_sync=False) needs a float32 theta on the GPU (pytorch_device='cuda:N')")
        self._prepare_observation(x_observation_dict)
        n = self.num_latent_vars
        rank, ws = shard.world(self.process_group)
        use_graph = (optimizer_type == "adam" and n <= 13 and ws == 1 and self.timers is None and num_epochs > 4
                     and true_posterior_for_tvd is None)   # (a TVD per epoch needs theta after exactly that epoch)
        params, optimizer_born, scheduler = self.make_optimizer(lr_born_machine, num_epochs, use_lr_scheduler,
                                                                optimizer_type, adam_betas, capturable=use_graph)
        dev = theta.device
        losses, norms, tvds, extras = [], [], [], []
        log_every = (num_epochs // 10 if num_epochs >= 10 else 1)
        tvd_table_dev = None
        if true_posterior_for_tvd is not None:
            tvd_table_dev = (true_posterior_for_tvd if torch.is_tensor(true_posterior_for_tvd)
                             else torch.tensor([true_posterior_for_tvd.get(o, 0.0) for o in self.born_machine.all_outcomes_tuples],
                                               dtype=torch.float64)).to(dev)
        step = None
        seen = 0                              # epochs whose warnings / values have been reported

        adam = None                           # the graphed step's DeviceAdam: the kernel keeps the history, no clones

        def report(upto):
            nonlocal seen
            if upto <= seen:
                return None
            if adam is not None:
                vals = adam.history(seen, upto)[0].cpu().tolist()
            else:
                vals = torch.stack([l.reshape(()) for l in losses[seen:upto]]).cpu().tolist()
            for v in vals:
                if np.isnan(v) or np.isinf(v):
                    print(f"Warning: NaN or Inf {self._loss_name} loss: {v}. Skipping update.")
            seen = upto
            return vals[-1]

        for epoch in range(num_epochs):
            if use_graph and epoch == 0:
                rec = []
                step = self.make_graphed_step(params, optimizer_born, scheduler, gradient_clip_norm, warmup=2, record=rec)
                pending = rec                 # epochs 0 and 1 are the graph's two eager warm-up steps
                adam = step.adam
            if use_graph and epoch < 2:
                loss_t, gn, q, *ex = pending[epoch]
            elif use_graph and adam is not None:
                loss_t, gn, q, *ex = step()   # graph-owned: read below, before the next replay, or not at all
            elif use_graph:
                loss_t, gn, q, *ex = (t.clone() for t in step())
            else:
                loss_t, gn, q, *ex = self.training_step_async(params, optimizer_born, scheduler, gradient_clip_norm)
            if ex:
                extras.append(torch.stack([e.reshape(()) for e in ex]))      # (a copy: the next step overwrites them)
            if q.shape[0] != self.num_possible_latent_states:
                raise ValueError(f"Probabilities from Born machine have unexpected shape")
            if adam is None:
                losses.append(loss_t)
                norms.append(gn)
            if tvd_table_dev is not None:     # like the reference: the distribution AFTER this epoch's update (:168)
                q_now = self._tvd_probabilities().detach().squeeze()
                tvds.append(tvd_table(tvd_table_dev.to(q_now.device), q_now))
            if verbose and epoch % log_every == 0:
                print(f"  Epoch {epoch+1} Q Probs (first 4): {q[:4].detach().cpu().numpy()}")
                report(epoch + 1)
                print(f"  Epoch {epoch+1} Grad Norm (after clipping): {float(gn):.4f}")
            if verbose and (epoch % max(1, num_epochs // 20) == 0 or epoch == num_epochs - 1):
                last = report(epoch + 1)
                last = float(loss_t) if last is None else last
                log_msg = f"Epoch {epoch+1}/{num_epochs} | {self._loss_name}: {last:.6f}"
                if scheduler is not None:
                    lr_now = (step.adam.lr_at(epoch + 1) if step is not None and step.adam is not None
                              else float(scheduler.get_last_lr()[0]))
                    log_msg += f" | LR: {lr_now:.6f}"
                if tvds:
                    log_msg += f" | TVD: {float(tvds[-1]):.6f}"
                print(log_msg)
        report(num_epochs)
        if adam is not None:
            hl, hn = adam.history(0, num_epochs)
            loss_h, norm_h = hl.cpu().tolist(), hn.to(torch.float64).cpu().tolist()
        else:
            loss_h = torch.stack([l.reshape(()) for l in losses]).cpu().tolist() if losses else []
            norm_h = torch.stack([g.reshape(()).to(torch.float64) for g in norms]).cpu().tolist() if norms else []
        # the reference keeps the last good norm on a skipped epoch (0.0 before the first good one)
        grad_h, last_good = [], None
        for lv, gv in zip(loss_h, norm_h):
            if not (np.isnan(lv) or np.isinf(lv)):
                last_good = gv
            grad_h.append(last_good if last_good is not None else 0.0)
        tvd_h = (torch.stack([t.reshape(()) for t in tvds]).cpu().tolist() if tvds else [np.nan] * num_epochs)
        history = {self._loss_key: loss_h, 'tvd': tvd_h, 'grad_norm': grad_h}
        if extras:
            for k, col in zip(self._extra_keys, torch.stack(extras).t().cpu().tolist()):
                history[k] = col
        if tvds and verbose:
            print(f"\nRestoring best parameters (TVD: {min(tvd_h):.6f})")     # (a no-op in the reference too: quirk Q3)
        return history
