"""Amortised inference with the sampled MPS Born machine: one fit, any evidence.

The MPS runs over the latent AND the observed variables of the network.  It is fitted to the network itself, which is a
generative model: epoch e draws (x_b, z_b) ~ p exactly (backend.bn_sample with (seed, e); other network nodes are drawn and
dropped) and takes a maximum-likelihood step on the draws, the forward KL(p || q) up to the constant entropy of p:
  'joint'        loss = -mean log q(x_b, z_b)                       mps_environments + mps_score_vjp(idx, -1 / B)
  'conditional'  loss = -mean [log q(x_b, z_b) - log q(x_b)]        and mps_log_marginals_vjp over the observed sites, + 1 / B
No observation enters the training.  The fitted q then answers q(z | x) exactly for any x, through the queries of
SampledMPSBornMachine (log_marginal, sample_given): posterior_sample, posterior_log_prob, posterior_marginals, log_evidence.
With at most 16 observed sites the 'conditional' query list is all 2^c evidences of those sites with the weights
count_j / B (the counts are integers, added on the device); with more there is one query per sample and num_samples <= 2^16.
The optimiser, the NaN/Inf guard and the clip are SampledTrainer's (make_sampled_optimizer, host_update: sampled_trainer.py).
"""
import math

import torch

from . import backend
from .bayesian_network import pack_network_for_sampling
from .born_machine_mps_sampled import SampledMPSBornMachine, append_sweep
from .sampled_trainer import checked_config, host_update, make_sampled_optimizer
from .utils import generate_all_binary_outcomes


class AmortisedMPSInference:
    MAX_SITES = backend.MPS_SAMPLED_MAX_N
    MAX_ENUMERATED_OBSERVED = backend.MPS_QUERY_MAX_QUERIES.bit_length() - 1    # 2^16 evidences: one mps_log_marginals_vjp call
    OBJECTIVES = ('joint', 'conditional')

    def __init__(self, bayesian_network, latent_vars_names, observed_vars_names, born_machine_config, device='cpu'):
        cfg, B = checked_config(born_machine_config, ('bond_dim', 'num_samples', 'seed', 'init_method', 'site_order'), 1,
                                backend.MPS_SAMPLED_MAX_BATCH, "1 ... 2^24")
        self.bn = bayesian_network
        self.latent_vars_names = list(latent_vars_names)
        self.observed_vars_names = list(observed_vars_names)
        names = self.latent_vars_names + self.observed_vars_names
        if len(set(names)) != len(names):
            raise ValueError("latent and observed variable names must be disjoint and not repeated")
        for nm in names:
            if nm not in bayesian_network.node_to_index:
                raise ValueError(f"{nm!r} is not a node of the network")
        order = cfg.get('site_order')
        if order is None:
            order = [nm for nm in bayesian_network.nodes if nm in set(names)]
        order = list(order)
        if len(set(order)) != len(order):
            raise ValueError(f"site_order: a name is repeated in {order}")
        if set(order) != set(names):
            raise ValueError(f"site_order must list every latent and observed variable once: missing "
                             f"{sorted(set(names) - set(order))}, unknown {sorted(set(order) - set(names))}")
        if not 1 <= len(order) <= self.MAX_SITES:
            raise ValueError(f"the MPS takes 1 ... {self.MAX_SITES} sites (latent plus observed), got {len(order)}")
        self.site_names = order
        self.num_sites = len(order)
        self.num_samples = B
        self.seed = cfg.get('seed', 0)
        self.device = torch.device(device)
        self._packed = pack_network_for_sampling(bayesian_network, order)        # topological order is checked here
        self.born_machine = SampledMPSBornMachine(self.num_sites, bond_dim=cfg.get('bond_dim', 4),
                                                  init_method=cfg.get('init_method', 'small_random'),
                                                  seed=self.seed).to(self.device)
        n = self.num_sites
        self._observed_positions = [order.index(nm) for nm in self.observed_vars_names]
        self._observed_mask = sum(1 << (n - 1 - p) for p in self._observed_positions)
        self._desc = None
        self._p_table = None
        self.last_idx = None

    # ---- the epoch ------------------------------------------------------------------------------------------------
    def _check_objective(self, objective):
        if objective not in self.OBJECTIVES:
            raise ValueError(f"objective must be one of {self.OBJECTIVES}, got {objective!r}")
        if objective == 'conditional':
            if not self._observed_positions:
                raise ValueError("objective 'conditional' needs at least one observed variable")
            if len(self._observed_positions) > self.MAX_ENUMERATED_OBSERVED and self.num_samples > backend.MPS_QUERY_MAX_QUERIES:
                raise ValueError(f"objective 'conditional' with more than {self.MAX_ENUMERATED_OBSERVED} observed variables takes "
                                 f"one query per sample: num_samples <= 2^16, got {self.num_samples}")

    def _prepare(self):
        if self._desc is not None:
            return
        dev = backend.compute_device(self.device)
        self._desc = backend.bn_descriptor(self._packed, dev)            # (device arrays kept alive, descriptor)
        self._epoch_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        B, n, c = self.num_samples, self.num_sites, len(self._observed_positions)
        self._w = torch.full((B,), -1.0 / B, dtype=torch.float64, device=dev)
        if 0 < c <= self.MAX_ENUMERATED_OBSERVED:
            shifts = [n - 1 - p for p in self._observed_positions]
            self._shifts = torch.tensor(shifts, dtype=torch.int64, device=dev)
            self._code_weights = torch.tensor([1 << (c - 1 - i) for i in range(c)], dtype=torch.int64, device=dev)
            values = [sum(((j >> (c - 1 - i)) & 1) << shifts[i] for i in range(c)) for j in range(1 << c)]
            self._query_value = torch.tensor(values, dtype=torch.int64, device=dev)
            self._query_mask = torch.full((1 << c,), self._observed_mask, dtype=torch.int64, device=dev)

    def evidence_queries(self, idx, per_sample=False):
        """The 'conditional' term's query list for the epoch's samples -> (mask [Q], value [Q] int64, c [Q] float64), all on
        the device, nothing read back: all 2^c evidences of the observed sites with c_j = count_j / B, or (more than 16
        observed sites, or per_sample) one query per sample with c = 1 / B."""
        c = len(self._observed_positions)
        if c <= self.MAX_ENUMERATED_OBSERVED and not per_sample:
            code = (((idx[:, None] >> self._shifts[None, :]) & 1) * self._code_weights[None, :]).sum(dim=1)
            counts = torch.zeros(1 << c, dtype=torch.int64, device=idx.device).scatter_add_(0, code, torch.ones_like(code))
            return self._query_mask, self._query_value, counts.to(torch.float64) / self.num_samples
        B = self.num_samples
        mask = torch.full((B,), self._observed_mask, dtype=torch.int64, device=idx.device)
        return mask, idx & mask, torch.full((B,), 1.0 / B, dtype=torch.float64, device=idx.device)

    def loss_and_grad(self, epoch, objective='joint', per_sample_queries=False):
        """Device part of one epoch -> (loss [] float64, grad float64 [n, 2, D, D], status [1] int32: the status words of the
        calls or-ed).  Nothing is read back to the host."""
        self._check_objective(objective)
        self._prepare()
        cores, _ = self.born_machine.kernel_input()
        B, n = self.num_samples, self.num_sites
        self._epoch_dev.fill_(int(epoch))
        idx, _, st_s = backend.bn_sample(self._desc[1], n, B, self.seed, self._epoch_dev)
        self.last_idx = idx
        backend.mps_environments(cores, B)
        grad, logq, st_g = backend.mps_score_vjp(cores, idx, self._w)
        loss = -logq.mean()
        status = st_s | st_g
        if objective == 'conditional':
            mask, value, c = self.evidence_queries(idx, per_sample_queries)
            grad_m, logm, st_m = backend.mps_log_marginals_vjp(cores, mask, value, c)
            grad = grad + grad_m
            loss = loss + torch.where(c > 0, c * logm, torch.zeros_like(logm)).sum()
            status = status | st_m
        return loss, grad, status

    def train(self, num_epochs, lr_born_machine, objective='joint', verbose=True, use_lr_scheduler=True, gradient_clip_norm=10.0,
              optimizer_type="adam", adam_betas=(0.9, 0.999), sgd_momentum=0.9, epoch_callback=None):
        """The optimiser arguments of SampledTrainer.train; no observation.  epoch_callback(epoch, self), where given, runs
        after every update (read-outs there leave the run unchanged).  History: loss, grad_norm, status."""
        self._check_objective(objective)
        bm = self.born_machine
        opt, sched = make_sampled_optimizer(bm, lr_born_machine, num_epochs, use_lr_scheduler, optimizer_type, adam_betas, sgd_momentum)
        history = {'loss': [], 'grad_norm': [], 'status': []}
        grad_norm = None
        for epoch in range(num_epochs):
            opt.zero_grad()
            loss_t, grad, st_t = self.loss_and_grad(epoch, objective)
            loss, grad_norm = host_update(loss_t, grad, bm, opt, sched, gradient_clip_norm, grad_norm)
            history['loss'].append(loss)
            history['grad_norm'].append(grad_norm.item() if grad_norm is not None else 0.0)
            history['status'].append(int(st_t.item()))
            if epoch_callback is not None:
                epoch_callback(epoch, self)
            if verbose and (epoch % max(1, num_epochs // 20) == 0 or epoch == num_epochs - 1):
                msg = f"Epoch {epoch+1}/{num_epochs} | loss ({objective}): {loss:.6f} | grad norm: {history['grad_norm'][-1]:.4f}"
                if sched is not None:
                    msg += f" | LR: {sched.get_last_lr()[0]:.6f}"
                print(msg)
        return history

    def train_two_site(self, num_sweeps, lr, descent_steps=5, cutoff=1e-4, max_rank=None, verbose=True, sweep_callback=None):
        """Training by two-site sweeps, objective 'joint' only: sweep e draws fresh (x, z) ~ p with
        (seed, e) exactly as loss_and_grad does and runs one round trip of SampledMPSBornMachine.two_site_sweep_ on the draws
        with weights 1 / B: descent_steps plain steps of size lr per bond, every bond then cut to the rank its spectrum shows
        (at most max_rank, default the machine's bond_dim: expand_ raises that cap; values go from the small end while their
        squares sum to <= cutoff).  No optimiser.  sweep_callback(sweep, self), where given, runs after every sweep.  History:
        loss (the last bond's), bond_loss, rank, discarded, status (the sweep's status word; 16 is added when the network
        sampler reported a dead draw)."""
        if isinstance(num_sweeps, bool) or not isinstance(num_sweeps, int) or num_sweeps < 1:
            raise ValueError(f"num_sweeps must be a positive integer, got {num_sweeps!r}")
        bm = self.born_machine
        B, n = self.num_samples, self.num_sites
        bm._check_two_site(B, None, lr, descent_steps, cutoff, max_rank)
        self._prepare()
        history = {'loss': [], 'bond_loss': [], 'rank': [], 'discarded': [], 'status': []}
        for sweep in range(num_sweeps):
            self._epoch_dev.fill_(sweep)
            idx, _, st_s = backend.bn_sample(self._desc[1], n, B, self.seed, self._epoch_dev)
            self.last_idx = idx
            report = bm.two_site_sweep_(idx, None, lr, descent_steps, cutoff, max_rank)
            append_sweep(history, report)
            if int(st_s.item()) != 0:
                history['status'][-1] |= 16
            if sweep_callback is not None:
                sweep_callback(sweep, self)
            if verbose:
                print(f"Sweep {sweep+1}/{num_sweeps} | loss (joint, last bond): {history['loss'][-1]:.6f} | ranks: {history['rank'][-1]}")
        return history

    # ---- the fitted q read out per evidence: SampledMPSBornMachine's queries by variable name ----------------------------
    def _evidence_by_name(self, x_observation_dict):
        """{name: 0 or 1} over any subset of the observed or latent names -> {tuple position: value}; raises on the host."""
        if not isinstance(x_observation_dict, dict):
            raise ValueError(f"x_observation_dict: a dict {{name: 0 or 1}}, got {x_observation_dict!r}")
        out = {}
        for name, val in x_observation_dict.items():
            if name not in self.site_names:
                raise ValueError(f"{name!r} is neither a latent nor an observed variable of this trainer")
            if isinstance(val, bool) or not isinstance(val, int) or val not in (0, 1):
                raise ValueError(f"the value of {name!r} must be 0 or 1, got {val!r}")
            out[self.site_names.index(name)] = val
        return out

    def free_names(self, x_observation_dict):
        """The sites that x leaves free, in site order."""
        return [nm for nm in self.site_names if nm not in x_observation_dict]

    def posterior_sample(self, x_observation_dict, num_samples, seed=None, epoch=0):
        """(idx int64 [num]: whole states over the sites, carrying x; logq float64 [num] = log q(state | x); log q(x) [1])."""
        ev = self._evidence_by_name(x_observation_dict)
        return self.born_machine.sample_given(ev, num_samples, seed=seed, epoch=epoch)

    def posterior_log_prob(self, x_observation_dict, z_bits):
        """float64 [B] on the compute device: log q(z | x) = log q(x, z) - log q(x) for rows z_bits [B, free sites] of 0 / 1 over
        free_names(x) in site order; B < 2^16."""
        ev = self._evidence_by_name(x_observation_dict)
        free = [p for p in range(self.num_sites) if p not in ev]
        z = torch.as_tensor(z_bits)
        if z.dim() != 2 or z.shape[1] != len(free) or not 1 <= z.shape[0] < backend.MPS_QUERY_MAX_QUERIES:
            raise ValueError(f"z_bits: rows of {len(free)} bits (the free sites in site order), at most 2^16 - 1 of them")
        if not bool(((z == 0) | (z == 1)).all()):
            raise ValueError("z_bits: every entry must be 0 or 1")
        n = self.num_sites
        base = sum(v << (n - 1 - p) for p, v in ev.items())
        shifts = torch.tensor([n - 1 - p for p in free], dtype=torch.int64)
        value = (z.to(device='cpu', dtype=torch.int64) << shifts[None, :]).sum(dim=1) + base
        value = torch.cat([value, torch.tensor([base], dtype=torch.int64)])
        mask = torch.full_like(value, (1 << n) - 1)
        mask[-1] = sum(1 << (n - 1 - p) for p in ev)
        logm = self.born_machine.log_marginal((mask, value))
        return logm[:-1] - logm[-1]

    def posterior_marginals(self, x_observation_dict):
        """{name: q(name = 1 | x)} for every free site, exact: exp(logm(x and name = 1) - logm(x)), one log_marginal call."""
        ev = self._evidence_by_name(x_observation_dict)
        free = [p for p in range(self.num_sites) if p not in ev]
        logm = self.born_machine.log_marginal([{**ev, p: 1} for p in free] + [ev])
        m = torch.exp(logm[:-1] - logm[-1]).cpu().tolist()
        return {self.site_names[p]: v for p, v in zip(free, m)}

    def log_evidence(self, x_observation_dict):
        """log q(x): the fitted estimate of log p(x)."""
        return float(self.born_machine.log_marginal(self._evidence_by_name(x_observation_dict)).item())

    def site_joint_table(self):
        """p over the sites, float64 [2^n] on the host (n <= 26), other network nodes summed out, by enumeration."""
        if self.num_sites > backend.MPS_MAX_N:
            raise ValueError(f"the enumerated joint exists for at most {backend.MPS_MAX_N} sites, got {self.num_sites}")
        if self._p_table is None:
            n = self.num_sites
            pos = {nm: self.site_names.index(nm) for nm in self.site_names}
            table = [0.0] * (1 << n)
            for assignment in generate_all_binary_outcomes(len(self.bn.nodes)):
                state = 0
                for nm, v in zip(self.bn.nodes, assignment):
                    if nm in pos:
                        state |= v << (n - 1 - pos[nm])
                table[state] += self.bn.get_joint_probability(assignment)
            self._p_table = torch.tensor(table, dtype=torch.float64)
        return self._p_table

    def exact_forward_kl(self):
        """KL(p || q) over the sites by enumeration (n <= 26): probabilities64 against get_joint_probability."""
        p = self.site_joint_table()
        with torch.no_grad():
            q = self.born_machine.probabilities64().detach().cpu()
        m = p > 0
        if bool((q[m] <= 0).any()):
            return math.inf
        return float((p[m] * (torch.log(p[m]) - torch.log(q[m]))).sum())
