#!/usr/bin/env python3
"""Capture the Born-machine (REINFORCE) steps of the reference's adversarial trainer WITH their gradients (run in the
build container only; numbers only are stored).

Imports the reference's adversarial_vi / bayesian_network / utils from /root/reference and runs its own train() on the
Sprinkler network (W = 1, classical probability table, seed 11, batch 64, 4 epochs, baseline_decay 0.9) once with
use_logits=True and once with use_logits=False.  Spies record, per Born step: the sample indices, the classifier's
logits, log p(x|z) of the samples, q and the table w of the log-q forward, and `params.grad` BEFORE clipping (a spy on
nn_utils.clip_grad_norm_ in the reference module's namespace keeps the call whose only parameter is born_machine.params).
The running baseline is a local of train(): it is recomputed from the recorded rewards as make_golden.py: reinforce_trace
does and checked against the recorded loss_q before anything is written.

    python tests/golden/make_golden_adversarial_classical.py    ->  tests/golden/adversarial_classical_trace.npz
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

import adversarial_vi as ref_adv                  # noqa: E402  (reference)
import bayesian_network as ref_bn                 # noqa: E402  (reference)
import utils as ref_utils                         # noqa: E402  (reference)

SEED, EPOCHS, BATCH, DECAY = 11, 4, 64, 0.9


def run_case(use_logits):
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    bn, lat, obs = ref_bn.get_sprinkler_network(False), ['C', 'S', 'R'], ['W']
    adv = ref_adv.AdversarialVariationalInference(bn, lat, obs,
                                                  born_machine_config={'use_logits': use_logits, 'conditioning_dim': 0},
                                                  classifier_config={}, device='cpu')
    outs = ref_utils.generate_all_binary_outcomes(len(lat))
    rec = {k: [] for k in ("idx", "logits", "log_p", "q", "w", "grad")}
    state = {}
    bm, clf = adv.born_machine, adv.classifier
    orig_logq, orig_logp, orig_fwd, orig_clip = bm.get_log_q_z_x, adv._get_log_p_x_given_z, clf.forward, ref_adv.nn_utils.clip_grad_norm_

    def spy_logq(z, xc=None):                      # called once per Born step, after the classifier and log p
        out = orig_logq(z, xc)
        rec["idx"].append(np.array([outs.index(tuple(int(v) for v in row)) for row in z.tolist()]))
        rec["q"].append(bm.get_probabilities(xc).detach().squeeze().numpy().copy())
        rec["w"].append(bm.params.detach().numpy().copy())
        rec["logits"].append(state.pop("last_logits"))
        rec["log_p"].append(state.pop("last_logp"))
        return out

    def spy_logp(x, z):
        out = orig_logp(x, z)
        state["last_logp"] = out.detach().numpy().copy()
        return out

    def spy_fwd(x):
        out = orig_fwd(x)
        state["last_logits"] = out.detach().squeeze().numpy().copy()      # (the Born step's call is the last one before log q)
        return out

    def spy_clip(parameters, max_norm, *a, **kw):
        params = list(parameters)
        if len(params) == 1 and params[0] is bm.params:
            rec["grad"].append(bm.params.grad.detach().numpy().copy())    # before the clip scales it
        return orig_clip(params, max_norm, *a, **kw)

    bm.get_log_q_z_x, adv._get_log_p_x_given_z, clf.forward = spy_logq, spy_logp, spy_fwd
    ref_adv.nn_utils.clip_grad_norm_ = spy_clip
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            hist = adv.train({'W': 1}, num_epochs=EPOCHS, batch_size=BATCH, lr_born_machine=0.01, lr_classifier=0.01,
                             k_classifier_steps=1, k_born_steps=1, verbose=False, baseline_decay=DECAY)
    finally:
        ref_adv.nn_utils.clip_grad_norm_ = orig_clip
    assert all(len(v) == EPOCHS for v in rec.values()), {k: len(v) for k, v in rec.items()}
    # log p(x|z) of every outcome, through the reference's own function (the kernel gathers from this table)
    z_all = torch.tensor(outs, dtype=torch.float32)
    table = orig_logp(torch.tensor([1.0]), z_all).detach().numpy().astype(np.float32)
    base, bases, losses = 0.0, [], []
    for e in range(EPOCHS):
        assert np.array_equal(table[rec["idx"][e]], rec["log_p"][e])
        raw = torch.tensor(rec["logits"][e]) - torch.tensor(rec["log_p"][e])
        base = raw.mean().item() if e == 0 else DECAY * base + (1 - DECAY) * raw.mean().item()
        bases.append(base)
        lq = torch.log(torch.tensor(rec["q"][e]).clamp(min=1e-10))[torch.tensor(rec["idx"][e])]
        losses.append(float((lq * (raw - base) - (-0.01 * lq)).mean()))
    assert np.allclose(losses, hist['loss_born_machine'], rtol=1e-6, atol=1e-7), (losses, hist['loss_born_machine'])
    print(f"use_logits={use_logits}: loss_q {hist['loss_born_machine']} baseline {bases}")
    return dict(idx=np.array(rec["idx"], dtype=np.int64), logits=np.array(rec["logits"], dtype=np.float32),
                log_p=np.array(rec["log_p"], dtype=np.float32), log_p_table=table, q=np.array(rec["q"], dtype=np.float32),
                w=np.array(rec["w"], dtype=np.float32), grad=np.array(rec["grad"], dtype=np.float32),
                baseline=np.array(bases, dtype=np.float64), loss_q=np.array(hist['loss_born_machine'], dtype=np.float64))


if __name__ == "__main__":
    out = {"baseline_decay": np.float64(DECAY), "seed": np.int64(SEED)}
    for use_logits, tag in ((True, "logits"), (False, "abs")):
        out.update({f"{tag}_{k}": v for k, v in run_case(use_logits).items()})
    np.savez_compressed(os.path.join(HERE, "adversarial_classical_trace.npz"), **out)
