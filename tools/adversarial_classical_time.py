#!/usr/bin/env python3
"""Born step of the classical adversarial trainer on the MI355X, table mode (GPU only: fails without one).

For each size n (synthetic_network(n, 0, 0.4, 0.6), softmax table, REINFORCE batch B) prints one JSON line with, from
device events in one process on the same inputs:
  fused_step_ms      the Born step as the trainer enqueues it up to the gradient: born_table_probs -> torch.multinomial
                     -> classifier forward -> reinforce_step -> born_table_vjp into the gradient buffer
  mirror_step_ms     the same step as a chain of torch ops (softmax, multinomial, classifier forward, gather, log, mean,
                     in-place baseline, autograd backward with its duplicate-index scatter-add): the formulation of the
                     quantum trainer's _born_step for this part.  THE BASELINE of the comparison.
  reinforce_ms       reinforce_step alone
The two steps are timed alternately, `rounds` blocks of `block` iterations each after a warm-up of both; each figure is
the median of the per-block means, with the smallest and largest block mean as the spread.
  eager_epochs_per_s / graph_epochs_per_s   whole train() epochs (one classifier step and one Born step per epoch, no
                     TVD), host clock around a call that ends in the history read-back, first call discarded.

    python tools/adversarial_classical_time.py [--sizes 12 16 20] [--batch 65536] [--rounds 10] [--block 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                                      # noqa: E402
from tensornetworks_amd.adversarial_vi_classical import AdversarialVariationalInference    # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network                           # noqa: E402

DEV = "cuda:0"


def block_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(samples):
    return {"median": round(statistics.median(samples), 4), "min": round(min(samples), 4), "max": round(max(samples), 4)}


def measure(n, B, rounds, block, epochs):
    torch.manual_seed(0)
    bn, lat, obs, x = synthetic_network(n, 0, p_low=0.4, p_high=0.6)
    vi = AdversarialVariationalInference(bn, lat, obs, {'use_logits': True, 'conditioning_dim': 0}, {}, device=DEV)
    bm, clf = vi.born_machine, vi.classifier
    x_obs = torch.tensor([float(x[nm]) for nm in obs], device=DEV)
    log_p = vi._log_p_table(x_obs)
    grad = torch.empty(1, 1 << n, dtype=torch.float32, device=DEV)
    base64 = torch.zeros(1, dtype=torch.float64, device=DEV)
    base32 = torch.zeros((), device=DEV)

    def fused():
        with torch.no_grad():
            w = bm.params.detach().reshape(1, -1)
            q32, q64, _ = backend.born_table_probs(w, 0, want_entropy=False)
            probs = q32 + 1e-10
            idx = torch.multinomial(probs / probs.sum(dim=-1, keepdim=True), B, replacement=True)[0]
            logit = clf(vi._bits(idx)).squeeze(-1)
            d, _, _ = backend.reinforce_step(idx, logit, log_p, q32[0], base64, False, 0.99)
            backend.born_table_vjp(w, q64, 0, y=d.reshape(1, -1), out=grad)

    def torch_mirror():
        bm.params.grad = None
        q = torch.softmax(bm.params, dim=0)
        with torch.no_grad():
            probs = q.detach().reshape(1, -1) + 1e-10
            idx = torch.multinomial(probs / probs.sum(dim=-1, keepdim=True), B, replacement=True)[0]
            logit = clf(vi._bits(idx)).squeeze(-1)
            reward = vi._reinforce_reward(logit, log_p[idx], base32, False, 0.99)
        log_q = torch.log(q.clamp(min=1e-10))[idx]
        vi._reinforce_loss(log_q, reward).backward()

    with torch.no_grad():
        w = bm.params.detach().reshape(1, -1)
        q32, _, _ = backend.born_table_probs(w, 0, want_entropy=False)
        idx = torch.multinomial(q32, B, replacement=True)[0]
        logit = clf(vi._bits(idx)).squeeze(-1)
    dbuf = torch.empty(1 << n, dtype=torch.float64, device=DEV)

    def reinforce_only():
        backend.reinforce_step(idx, logit, log_p, q32[0], base64, False, 0.99, out=dbuf)

    for fn in (fused, torch_mirror, reinforce_only):
        block_ms(fn, block)
    t = {"fused": [], "mirror": [], "reinforce": []}
    for _ in range(rounds):
        t["fused"].append(block_ms(fused, block))
        t["mirror"].append(block_ms(torch_mirror, block))
        t["reinforce"].append(block_ms(reinforce_only, block))
    out = {"n": n, "B": B, "iterations": rounds * block, "fused_step_ms": summary(t["fused"]),
           "mirror_step_ms": summary(t["mirror"]), "reinforce_ms": summary(t["reinforce"]),
           "mirror_over_fused": round(statistics.median(t["mirror"]) / statistics.median(t["fused"]), 3)}
    bm.params.grad = None
    for graph in (False, True):
        rates = []
        for _ in range(3):
            t0 = time.perf_counter()
            vi.train(x, num_epochs=epochs, batch_size=B, lr_born_machine=0.003, lr_classifier=0.03, verbose=False,
                     graph_epochs=graph)
            rates.append(epochs / (time.perf_counter() - t0))
        key = "graph_epochs_per_s" if graph else "eager_epochs_per_s"
        out[key] = {"median": round(statistics.median(rates[1:]), 1), "runs": [round(r, 1) for r in rates[1:]]}
        if graph:
            out["graphed_epochs"], out["graph_error"] = vi.graphed_epochs, vi.graph_error
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adversarial_classical_time.py needs an MI355X (torch.cuda.is_available() is False)")
    if args.rounds * args.block < 200:
        raise SystemExit("rounds * block must be >= 200 iterations")
    for n in args.sizes:
        print(json.dumps(measure(n, args.batch, args.rounds, args.block, args.epochs)), flush=True)
        backend.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
