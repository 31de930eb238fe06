"""Restatements of the classical adversarial trainer's Born step (not a test module).

reinforce_numpy / table_vjp_numpy: float64 NumPy evaluation of the formulas bornvi_reinforce_step and
bornvi_born_table_vjp(ksd2 = NULL) document (reference adversarial_vi.py:200-222 and the autograd chain below it).

train: a torch-only restatement of the trainer's eager epochs for a trainer object built with the same seed: the same
torch.multinomial / Dropout / classifier calls in the same order, so the same random numbers; the Born step is the
reference's chain of torch ops (gather, log, mean, the running baseline as a Python float) differentiated by plain
autograd, whose index-gather backward is torch's scatter-add.  It uses the trainer's modules, prior and log p(x|z) table
and none of the reinforce / born-table kernels.  The Born probabilities are the softmax (or |w| / sum |w|) evaluated in
float64 and rounded to float32 once, as the kernel rounds them, so that both sides hand torch.multinomial the same
bits; the Born loss is evaluated in float64."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.utils as nn_utils
import torch.optim as optim

FLOOR32 = np.float32(1e-10)      # torch's clamp(min=1e-10) on a float32 tensor


def reinforce_numpy(idx, logit, log_p, q32, baseline, first, decay, coef=0.01):
    """-> (dLdq float64 [2^n], loss float, new baseline float); all arithmetic in float64 on the float32 inputs."""
    idx = np.asarray(idx, dtype=np.int64)
    B, N = idx.shape[0], q32.shape[0]
    with np.errstate(all="ignore"):
        raw = logit.astype(np.float64) - log_p.astype(np.float64)[idx]
        mean = raw.sum() / B
        base = mean if first else decay * baseline + (1 - decay) * mean
        w = raw - base + coef
        q = q32.astype(np.float64)
        logq = np.log(np.maximum(q32, FLOOR32).astype(np.float64))
        loss = (logq[idx] * w).sum() / B
        S = np.zeros(N)
        np.add.at(S, idx, w)
        hit = np.zeros(N, dtype=bool)
        hit[idx] = True
        d = np.where(hit & (q32 >= FLOOR32), S / (B * np.where(q > 0, q, 1.0)), 0.0)
    return d, loss, base


def table_vjp_numpy(w, q32, dLdq, mode):
    """d/dw of a loss with gradient dLdq at q = softmax(w) (mode 0) or |w| / sum |w| (mode 1), float64."""
    q = q32.astype(np.float64)
    c = (q * dLdq).sum()
    if mode == 0:
        return q * (dLdq - c)
    return np.sign(w.astype(np.float64)) * (dLdq - c) / np.abs(w.astype(np.float64)).sum()


def _probs(bm, x_condition):
    """float32 [2^n] Born probabilities of the trainer's machine, by torch: differentiable."""
    raw = bm.param_generator_net(x_condition.reshape(1, -1))[0] if bm.conditioning_dim > 0 else bm.params
    raw = raw.to(torch.float64)
    if bm.use_logits:
        return torch.softmax(raw - raw.max(), dim=0).to(torch.float32)
    return (raw.abs() / raw.abs().sum()).to(torch.float32)


def _sample(bm, x_condition, batch):
    with torch.no_grad():
        probs = _probs(bm, x_condition).reshape(1, -1) + 1e-10
        probs = probs / probs.sum(dim=-1, keepdim=True)
        return torch.multinomial(probs, batch, replacement=True)[0]


def train(vi, x_observation_dict, num_epochs, batch_size, lr_born_machine, lr_classifier, k_classifier_steps=1,
          k_born_steps=1, gradient_clip_norm=10.0, baseline_decay=0.99, adam_betas=(0.9, 0.999)):
    """Eager epochs of AdversarialVariationalInference.train (Adam, cosine schedule, no TVD) on vi's own modules.
    -> history dict (without 'tvd')."""
    dev = torch.device(vi.device)
    bm, clf = vi.born_machine, vi.classifier
    x_obs = torch.tensor([x_observation_dict[nm] for nm in vi.observed_vars_names], dtype=torch.float32, device=dev)
    x_condition = x_obs if bm.conditioning_dim > 0 else None
    fused = {"fused": True} if dev.type == "cuda" else {}
    opt_b = optim.Adam(bm.parameters(), lr=lr_born_machine, betas=adam_betas, **fused)
    opt_c = optim.Adam(clf.parameters(), lr=lr_classifier, betas=adam_betas, **fused)
    sch_b = optim.lr_scheduler.CosineAnnealingLR(opt_b, T_max=num_epochs, eta_min=lr_born_machine / 10)
    sch_c = optim.lr_scheduler.CosineAnnealingLR(opt_c, T_max=num_epochs, eta_min=lr_classifier / 10)
    crit = nn.BCEWithLogitsLoss()
    log_p_table = vi._log_p_table(x_obs)
    with_x = clf.network[0].in_features == vi.num_latent_vars + vi.num_observed_vars and vi.num_observed_vars > 0
    labels = torch.cat((torch.ones(batch_size, 1, device=dev), torch.zeros(batch_size, 1, device=dev)), dim=0)
    hist = {'loss_classifier': [], 'loss_born_machine': [], 'grad_norm_born': [], 'grad_norm_classifier': []}
    baseline, gn_q = 0.0, None
    for epoch in range(num_epochs):
        for _ in range(k_classifier_steps):
            opt_c.zero_grad()
            z_born = vi._bits(_sample(bm, x_condition, batch_size))
            z_prior = vi._sample_from_prior_z(batch_size)
            inputs = torch.cat((vi._clf_inputs(z_born, x_obs, with_x), vi._clf_inputs(z_prior, x_obs, with_x)), dim=0)
            loss_d = crit(clf(inputs), labels)
            loss_d.backward()
            gn_d = nn_utils.clip_grad_norm_(clf.parameters(), gradient_clip_norm)
            opt_c.step()
        hist['loss_classifier'].append(loss_d.item())
        hist['grad_norm_classifier'].append(gn_d.item())
        for _ in range(k_born_steps):
            opt_b.zero_grad()
            idx = _sample(bm, x_condition, batch_size)
            with torch.no_grad():
                logit = clf(vi._clf_inputs(vi._bits(idx), x_obs, with_x)).squeeze(-1)
            raw = logit.to(torch.float64) - log_p_table[idx].to(torch.float64)
            mean = raw.mean().item()
            baseline = mean if epoch == 0 else baseline_decay * baseline + (1 - baseline_decay) * mean
            log_q = torch.log(_probs(bm, x_condition).clamp(min=1e-10))[idx].to(torch.float64)
            loss_q = (log_q * (raw - baseline) - (-0.01 * log_q)).mean()
            if not (torch.isnan(loss_q) or torch.isinf(loss_q)):
                loss_q.backward()
                gn_q = nn_utils.clip_grad_norm_(bm.parameters(), gradient_clip_norm)
                opt_b.step()
        finite = not (torch.isnan(loss_q) or torch.isinf(loss_q))
        hist['loss_born_machine'].append(loss_q.item() if finite else np.nan)
        hist['grad_norm_born'].append(gn_q.item() if gn_q is not None else 0.0)
        sch_b.step()
        sch_c.step()
    return hist
