#!/usr/bin/env python3
"""Capture golden traces of the reference's classical KSD trainer (run in the build container only).

Imports the reference's ksd_vi / born_machine_classical_sim / bayesian_network from /root/reference, trains seeded
classical Born machines for a few epochs and stores numbers only (per-epoch q of the loss forward, parameters, every
history list, the final fixed probabilities) as small .npz files next to this script:

    classical_sprinkler_logits.npz   table, use_logits=True, Sprinkler W=1, Adam, entropy 0.01, posterior given
    classical_sprinkler_abs.npz      the same with use_logits=False
    classical_sprinkler_sgd.npz      the same as the first with SGD (momentum 0.9)
    classical_synthetic_n6.npz       table on synthetic_network(6, 0)
    classical_sprinkler_mlp.npz      MLP, conditioning_dim 1, param_generator_net.eval() before train()

    python tests/golden/make_golden_classical.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
sys.path.insert(1, REPO)

import bayesian_network as ref_bn                 # noqa: E402  (reference)
import ksd_vi as ref_ksd                          # noqa: E402  (reference)
import utils as ref_utils                         # noqa: E402  (reference)

from tensornetworks_amd.bayesian_network import synthetic_network  # noqa: E402

EPOCHS = 40
MLP_PARAM_EPOCHS = (0, 1, 2, 10, 20, 40)           # parameter snapshots kept for the MLP (2472 numbers each)


def to_ref_bn(our_bn):
    bn = ref_bn.BayesianNetwork()
    for nm in our_bn.nodes:
        pa = list(our_bn.parents[nm]) if nm in our_bn.parents else None
        bn.add_node(nm, cpt=our_bn.cpts[nm], parent_names=pa or None)
    return bn


def run_case(name, bn, lat, obs, x, cfg, seed, optimizer_type="adam", lam=0.01, lr=0.01, clip=10.0, eval_net=False):
    torch.manual_seed(seed)
    vi = ref_ksd.KSDVariationalInference(bn, lat, obs, born_machine_config=cfg)
    bm = vi.born_machine
    if eval_net:
        bm.param_generator_net.eval()
    post, _ = bn.get_true_posterior(lat, x)
    outs = ref_utils.generate_all_binary_outcomes(len(lat))

    def flat():
        return torch.cat([p.detach().reshape(-1) for p in bm.parameters()]).numpy().copy()

    rec = {"q": [], "params": [flat()]}
    state = {"loss_forward_next": True}
    orig_gp, orig_pd = bm.get_probabilities, bm.get_prob_dict

    def gp(x_condition=None):
        out = orig_gp(x_condition=x_condition)
        # the epoch's first forward with autograd on is the loss forward (the best snapshot runs under no_grad)
        if state["loss_forward_next"] and torch.is_grad_enabled() and not bm._use_fixed_probs:
            rec["q"].append(out.detach().squeeze().numpy().copy())
            state["loss_forward_next"] = False
        return out

    def pd(x_condition=None):
        out = orig_pd(x_condition=x_condition)     # the TVD forward, once per epoch after the update
        if not bm._use_fixed_probs:
            rec["params"].append(flat())
            state["loss_forward_next"] = True
        return out

    bm.get_probabilities, bm.get_prob_dict = gp, pd
    with contextlib.redirect_stdout(io.StringIO()):
        hist = vi.train(x, num_epochs=EPOCHS, lr_born_machine=lr, verbose=False, true_posterior_for_tvd=post,
                        gradient_clip_norm=clip, optimizer_type=optimizer_type, entropy_weight=lam, patience=200)
    params = np.array(rec["params"], dtype=np.float32)
    param_epochs = np.arange(len(params))
    if cfg.get("conditioning_dim", 0) > 0:
        param_epochs = np.array(MLP_PARAM_EPOCHS)
        params = params[param_epochs]
    out = dict(q=np.array(rec["q"], dtype=np.float32), params=params, param_epochs=param_epochs,
               loss_ksd=np.array(hist["loss_ksd"]), tvd=np.array(hist["tvd"]), grad_norm=np.array(hist["grad_norm"]),
               entropy=np.array(hist["entropy"]), fixed_probs=bm._fixed_probs.numpy().astype(np.float32),
               posterior=np.array([post[z] for z in outs]), seed=np.int64(seed), lr=np.float64(lr),
               entropy_weight=np.float64(lam), clip=np.float64(clip), use_logits=np.bool_(cfg.get("use_logits", True)),
               conditioning_dim=np.int64(cfg.get("conditioning_dim", 0)), sgd=np.bool_(optimizer_type == "sgd"),
               x_value=np.array([x[o] for o in obs], dtype=np.int64), n=np.int64(len(lat)))
    assert len(out["q"]) == EPOCHS and len(rec["params"]) == EPOCHS + 1
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"{name}: loss {out['loss_ksd'][0]:.6f} -> {out['loss_ksd'][-1]:.6f}, tvd -> {out['tvd'][-1]:.6f}")


if __name__ == "__main__":
    spr = ref_bn.get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    run_case("classical_sprinkler_logits", spr, lat, obs, x, {'use_logits': True, 'conditioning_dim': 0}, seed=3)
    run_case("classical_sprinkler_abs", spr, lat, obs, x, {'use_logits': False, 'conditioning_dim': 0}, seed=3)
    run_case("classical_sprinkler_sgd", spr, lat, obs, x, {'use_logits': True, 'conditioning_dim': 0}, seed=3,
             optimizer_type="sgd")
    ours6, lat6, obs6, x6 = synthetic_network(6, 0)
    run_case("classical_synthetic_n6", to_ref_bn(ours6), lat6, obs6, x6, {'use_logits': True, 'conditioning_dim': 0},
             seed=5)
    run_case("classical_sprinkler_mlp", spr, lat, obs, x, {'use_logits': True, 'conditioning_dim': 1}, seed=4,
             lr=0.003, clip=5.0, lam=0.001, eval_net=True)
