"""The epoch of the sampled MPS trainers, owned once: no 2^n object at any n <= 63.

An epoch: the machine's environments, its draw with (seed, epoch) -> (idx, log q); the objective's weights w_b from the
samples (the subclass: `sample_weights`); its score_gradient -> sum_b w_b grad log q(z_b) (for real cores mps_environments,
mps_sample and mps_score_vjp, for born_machine_config['cores'] = 'complex' the cmps_* three, for 'purified' (with
'purification_dim') the lps_* three, for 'tree' the ttn_* three: the epoch names no family -- the tables FAMILIES and TREE_FAMILIES pick the machine's class, and
everything else is asked of the machine, born_machine_sampled.SampledSurface); then the NaN/Inf guard, clip and Adam or SGD
with cosine annealing through torch.optim on the float64 cores: the enumerated trainers' own make_optimizer and
guarded_update (ksd_vi.py).  Epoch e draws with (seed, e): fresh samples every epoch, the same ones on a rerun.
With `natural_gradient` (natural_gradient.SampledFisherPreconditioner.coerce says what it accepts) the gradient is replaced,
before the guard and the clip, by delta = (F^ + damping I)^-1 grad, F^ the Fisher estimate from the epoch's own samples;
history['natgrad_info'] counts the blocks per epoch whose factorisation failed (they keep the plain gradient).
natural_gradient='sample' (SampleSpaceFisherPreconditioner) is the full-matrix step solved in sample space: it takes the
weights w and returns delta = sum_b u_b grad log q(z_b) with (T + damping I) u = w, for num_samples <= 1024.
natural_gradient='cg' (CGFisherPreconditioner) solves the same full-matrix system by conjugate gradients without a matrix, at
any bond dimension and any num_samples; history['natgrad_iters'] then holds the iterations each epoch took.

A subclass supplies
  LOSS_KEYS                     the history keys it fills per epoch, MIN_SAMPLES / MAX_SAMPLES and their wording,
  sample_weights(idx, logq)     -> (loss [] float64, w [B] float64) on the device, nothing read back,
  record_loss(history, loss)    the epoch's entries of LOSS_KEYS from the loss as a float,
  describe(loss)                the loss part of the progress line.
SampledELBOVariationalInference (elbo_vi_sampled.py) and SampledKSDVariationalInference (ksd_vi_sampled.py) are the two.
Networks with summed-out nodes are refused (the enumerated trainers handle them).
"""
import numpy as np
import torch

from . import backend
from .bayesian_network import pack_network
from .born_machine_cmps_sampled import ComplexSampledMPSBornMachine
from .born_machine_lps_sampled import PurifiedSampledMPSBornMachine
from .born_machine_mps_sampled import SampledMPSBornMachine
from .born_machine_ttn_sampled import TreeSampledBornMachine
from .ksd_vi import guarded_update, make_optimizer
from .natural_gradient import CGFisherPreconditioner, SampledFisherPreconditioner, SampleSpaceFisherPreconditioner

# born_machine_config['cores'] -> (the machine's class, the config keys that go with this family alone).  What else the
# epoch needs of a family it asks the machine: environments / draw / score_gradient, bond_dim, ENUMERATED_MAX_N,
# NATURAL_GRADIENT and CORES (born_machine_sampled.SampledSurface).
FAMILIES = {'real': (SampledMPSBornMachine, ()), 'complex': (ComplexSampledMPSBornMachine, ()),
            'purified': (PurifiedSampledMPSBornMachine, ('purification_dim',))}
# The same for the families that are no chain: FAMILIES is the table of the matrix-product states (its three entries are what
# the chains' host definition is checked against), the tree tensor network has this one, and the trainer reads both.
TREE_FAMILIES = {'tree': (TreeSampledBornMachine, ())}
ALL_FAMILIES = {**FAMILIES, **TREE_FAMILIES}


def checked_config(born_machine_config, allowed_keys, min_samples, max_samples, samples_range):
    """(born_machine_config as a dict, its num_samples, default 1024), with the caller's own allowed keys and sample range."""
    cfg = dict(born_machine_config or {})
    unknown = set(cfg) - set(allowed_keys)
    if unknown:
        raise ValueError(f"born_machine_config: unknown keys {sorted(unknown)}")
    B = cfg.get('num_samples', 1024)
    if isinstance(B, bool) or not isinstance(B, int) or not min_samples <= B <= max_samples:
        raise ValueError(f"num_samples must be an integer in {samples_range}, got {B!r}")
    return cfg, B


def make_sampled_optimizer(born_machine, lr_born_machine, num_epochs, use_lr_scheduler, optimizer_type, adam_betas, sgd_momentum):
    """make_optimizer's (optimiser, scheduler) for the machine's parameters; optimizer_type="sgd" takes the checked momentum."""
    opt, sched = make_optimizer(born_machine.parameters(), lr_born_machine, num_epochs, use_lr_scheduler, optimizer_type, adam_betas)
    if optimizer_type != "adam":
        if isinstance(sgd_momentum, bool) or not isinstance(sgd_momentum, (int, float)) or not 0 <= sgd_momentum < 1:
            raise ValueError(f"sgd_momentum must be a number in [0, 1), got {sgd_momentum!r}")
        for group in opt.param_groups:
            group['momentum'] = float(sgd_momentum)
    return opt, sched


def host_update(loss_t, grad, born_machine, opt, sched, gradient_clip_norm, grad_norm):
    """The epoch's host part: the loss read back, then guarded_update on the cores -> (loss as a float, grad_norm)."""
    loss = float(loss_t.item())                       # the epoch's host synchronisation
    cores = born_machine.cores
    grad_norm = guarded_update(born_machine, opt, sched, loss, [(cores, grad.to(device=cores.device, dtype=cores.dtype))],
                               gradient_clip_norm, grad_norm)
    return loss, grad_norm


class SampledTrainer:
    LOSS_KEYS = ()
    MIN_SAMPLES = 1
    MAX_SAMPLES = backend.MPS_SAMPLED_MAX_BATCH
    SAMPLES_RANGE = "1 ... 2^24"

    def __init__(self, bayesian_network, latent_vars_names, observed_vars_names, born_machine_config, device='cpu',
                 p_floor=1e-30, natural_gradient=None):
        family_keys = tuple(key for _, keys in ALL_FAMILIES.values() for key in keys)
        cfg, B = checked_config(born_machine_config, ('bond_dim', 'num_samples', 'seed', 'init_method', 'cores') + family_keys,
                                self.MIN_SAMPLES, self.MAX_SAMPLES, self.SAMPLES_RANGE)
        kind = cfg.get('cores', 'real')
        if kind not in ALL_FAMILIES:
            raise ValueError(f"born_machine_config['cores'] must be 'real', 'complex', 'purified' or 'tree', got {kind!r}")
        family, own_keys = ALL_FAMILIES[kind]
        for owner, (_, keys) in ALL_FAMILIES.items():
            for key in set(keys).intersection(cfg).difference(own_keys):
                raise ValueError(f"born_machine_config[{key!r}] goes with 'cores': {owner!r} only")
        if natural_gradient is not None and not family.NATURAL_GRADIENT:
            raise ValueError(f"natural_gradient is not offered with {family.CORES}: the Fisher estimates exist for the real "
                             "family (born_machine_config['cores'] = 'real') only")
        if isinstance(p_floor, bool) or not isinstance(p_floor, (int, float)) or not np.isfinite(p_floor) or not p_floor > 0:
            raise ValueError(f"p_floor must be a positive finite number, got {p_floor!r}")
        self.bn = bayesian_network
        self.latent_vars_names = list(latent_vars_names)
        self.observed_vars_names = list(observed_vars_names)
        self.num_latent_vars = len(self.latent_vars_names)
        self.num_observed_vars = len(self.observed_vars_names)
        self.num_samples = B
        self.seed = cfg.get('seed', 0)
        self.p_floor = float(p_floor)
        self.device = torch.device(device)
        self.born_machine = family(self.num_latent_vars, bond_dim=cfg.get('bond_dim', 4),
                                   init_method=cfg.get('init_method', 'small_random'), seed=self.seed,
                                   **{key: cfg[key] for key in own_keys if key in cfg}).to(self.device)
        self.natural_gradient = SampledFisherPreconditioner.coerce(natural_gradient)
        if self.natural_gradient is not None:
            self.natural_gradient.plan(self.num_latent_vars, self.born_machine.bond_dim, B)
        self._desc = None
        self.last_idx = None

    def _prepare_observation(self, x_dict):
        packed = pack_network(self.bn, self.latent_vars_names, x_dict)
        if (packed["role"] == -3).any():
            raise ValueError("a network node is neither latent nor observed: the sampled trainer has no log joint per "
                             "sample for summed-out nodes (use the enumerated trainers)")
        dev = backend.compute_device(self.device)
        self._desc = backend.bn_descriptor(packed, dev)          # (device arrays kept alive, descriptor)
        self._epoch_dev = torch.zeros(1, dtype=torch.int64, device=dev)

    def draw(self, epoch):
        """The epoch's exact samples -> (cores, idx int64 [B], logq float64 [B], status int32 [1]), all on the device."""
        cores, _ = self.born_machine.kernel_input()
        B = self.num_samples
        self._epoch_dev.fill_(int(epoch))
        self.born_machine.environments(cores, B)
        idx, logq, st_s = self.born_machine.draw(cores, B, self.seed, self._epoch_dev)
        return cores, idx, logq, st_s

    def sample_weights(self, idx, logq):
        raise NotImplementedError

    def loss_and_grad(self, epoch):
        """Device part of one epoch -> (loss [] float64, grad float64 [n, 2, D, D], logq mean [], status [1] int32: the
        sampler's and the gradient's status words or-ed).  Nothing is read back to the host."""
        cores, idx, logq, st_s = self.draw(epoch)
        loss, w = self.sample_weights(idx, logq)
        self.last_idx = idx
        if isinstance(self.natural_gradient, SampleSpaceFisherPreconditioner):      # delta = O^T u: the plain O^T w need not run
            grad, _ = self.natural_gradient.precondition_weights(cores, idx, w.contiguous())
            return loss, grad, logq.mean(), st_s | self.natural_gradient.status
        grad, _, st_g = self.born_machine.score_gradient(cores, idx, w.contiguous())
        if self.natural_gradient is not None:
            grad, _ = self.natural_gradient.precondition(cores, idx, grad)
            return loss, grad, logq.mean(), st_s | st_g | self.natural_gradient.status
        return loss, grad, logq.mean(), st_s | st_g

    def record_loss(self, history, loss):
        raise NotImplementedError

    def describe(self, loss):
        raise NotImplementedError

    def train(self, x_observation_dict, num_epochs, lr_born_machine, verbose=True, true_posterior_for_tvd=None,
              use_lr_scheduler=True, gradient_clip_norm=10.0, optimizer_type="adam", adam_betas=(0.9, 0.999), sgd_momentum=0.9):
        """The arguments of elbo_vi's train() that make sense here (no entropy_weight, no early stopping), and sgd_momentum:
        the momentum of optimizer_type="sgd" (0.9: make_optimizer's; 0 gives the plain step lr * delta); Adam has none and
        ignores it.
        true_posterior_for_tvd: a float tensor [2^n] (stein_utils.true_posterior_table), honoured for n <= 26 only, where
        q is enumerated by mps_probs for the report (complex cores: for n <= 20, by log_prob over all 2^n indices).  History:
        the trainer's LOSS_KEYS, grad_norm, logq_mean, status, and for n <= 26 (complex cores: n <= 20) with a posterior: tvd
        and kl (= exact KL(q || posterior))."""
        if self.num_observed_vars > 0 and set(x_observation_dict.keys()) != set(self.observed_vars_names):
            raise ValueError("Keys in x_observation_dict must match self.observed_vars_names.")
        bm = self.born_machine
        self._prepare_observation(x_observation_dict)
        opt, sched = make_sampled_optimizer(bm, lr_born_machine, num_epochs, use_lr_scheduler, optimizer_type, adam_betas, sgd_momentum)
        exact = true_posterior_for_tvd is not None and self.num_latent_vars <= bm.ENUMERATED_MAX_N
        history = {k: [] for k in self.LOSS_KEYS + ('grad_norm', 'logq_mean', 'status')}
        if exact:
            history['tvd'], history['kl'] = [], []
        if self.natural_gradient is not None:
            history['natgrad_info'] = []
        cg = isinstance(self.natural_gradient, CGFisherPreconditioner)
        if cg:
            history['natgrad_iters'] = []
        grad_norm = None
        for epoch in range(num_epochs):
            opt.zero_grad()
            loss_t, grad, lq_t, st_t = self.loss_and_grad(epoch)
            loss, grad_norm = host_update(loss_t, grad, bm, opt, sched, gradient_clip_norm, grad_norm)
            self.record_loss(history, loss)
            history['grad_norm'].append(grad_norm.item() if grad_norm is not None else 0.0)
            history['logq_mean'].append(float(lq_t.item()))
            history['status'].append(int(st_t.item()))
            if self.natural_gradient is not None:
                history['natgrad_info'].append(int((self.natural_gradient.info != 0).sum().item()))
            if cg:
                history['natgrad_iters'].append(int(self.natural_gradient.iters.item()))
            if exact:
                tvd, kl = self.exact_report(true_posterior_for_tvd)
                history['tvd'].append(tvd)
                history['kl'].append(kl)
            if verbose and (epoch % max(1, num_epochs // 20) == 0 or epoch == num_epochs - 1):
                msg = f"Epoch {epoch+1}/{num_epochs} | {self.describe(loss)} | mean log q: {history['logq_mean'][-1]:.4f}"
                if sched is not None:
                    msg += f" | LR: {sched.get_last_lr()[0]:.6f}"
                if exact:
                    msg += f" | TVD: {history['tvd'][-1]:.6f} | KL: {history['kl'][-1]:.6f}"
                print(msg)
        return history

    # ---- the fitted posterior, read out exactly (SampledMPSBornMachine's queries by variable name) ------------------
    def _evidence_by_name(self, evidence):
        """{name: value} (or a sequence of such dicts) -> the same with tuple positions, through latent_vars_names."""
        if isinstance(evidence, dict):
            out = {}
            for name, val in evidence.items():
                if name in self.observed_vars_names:
                    raise ValueError(f"{name!r} is an observed variable: the posterior is already conditioned on it")
                if name not in self.latent_vars_names:
                    raise ValueError(f"{name!r} is not a latent variable of this trainer")
                out[self.latent_vars_names.index(name)] = val
            return out
        if isinstance(evidence, (list, tuple)):
            return [self._evidence_by_name(e) if isinstance(e, dict) else e for e in evidence]
        return evidence

    def posterior_marginals(self):
        """{name: q(z = 1)} of the current cores, exact."""
        m1 = self.born_machine.marginals().cpu().tolist()
        return dict(zip(self.latent_vars_names, m1))

    def posterior_log_marginal(self, evidence):
        """float64 [Q] on the compute device: log q of {name: value, ...}, or of each dict of a list."""
        return self.born_machine.log_marginal(self._evidence_by_name(evidence))

    def posterior_sample_given(self, evidence, num_samples, seed=None, epoch=0):
        """(idx, logq_cond, log_marginal) of SampledMPSBornMachine.sample_given, the evidence by variable name."""
        if not isinstance(evidence, dict):
            raise ValueError(f"evidence: a dict {{name: 0 or 1}}, got {evidence!r}")
        return self.born_machine.sample_given(self._evidence_by_name(evidence), num_samples, seed=seed, epoch=epoch)

    def exact_report(self, posterior):
        """(TVD, KL(q || posterior)) of the current cores against a posterior table [2^n], by enumeration: the machine's
        probabilities64() (n <= 26 by mps_probs; complex cores n <= 20 by log_prob over all indices)."""
        with torch.no_grad():
            q = self.born_machine.probabilities64().detach()
            p = posterior.to(device=q.device, dtype=torch.float64).reshape(-1)
            tvd = 0.5 * (q - p).abs().sum()
            m = q > 0
            kl = (q[m] * (torch.log(q[m]) - torch.log(p[m].clamp(min=1e-300)))).sum()
        return float(tvd), float(kl)
