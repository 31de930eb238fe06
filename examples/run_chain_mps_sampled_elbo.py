#!/usr/bin/env python3
"""Reverse-KL inference on a 40-variable chain, far past anything 2^n can hold: synthetic_network(40, 0) (an order-2 chain
whose posterior's square root is exactly an MPS of bond 4) with the sampled MPS trainer, D = 4, B = 4096 samples per epoch.
The loss is an estimate of KL(q || p(.|x)) - log p(x), so it is printed beside -log p(x), computed exactly on the host by
variable elimination along the chain (tree-width 2): the gap that is left is the KL.  No plotting.

    python examples/run_chain_mps_sampled_elbo.py [--n 40] [--bond 4] [--samples 4096] [--epochs 300] [--lr 0.02]"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference    # noqa: E402


def exact_log_evidence(bn, latents, x):
    """log p(x) of a network in which every node's parents lie among the two latents before it (synthetic_network):
    a forward message over (z_{k-1}, z_k), renormalised at every step."""
    def factor(name, value, assign):
        pa = tuple(assign[p] for p in (bn.parents[name] if name in bn.parents else ()))
        return bn.cpts[name][pa][value]
    n = len(latents)
    msg = np.zeros((2, 2))            # msg[a, b]: mass of (z_{k-1} = a, z_k = b); before the second node a is a dummy 0
    for b in (0, 1):
        msg[0, b] = factor(latents[0], b, {})
    log_scale = 0.0
    for k in range(1, n):
        new = np.zeros((2, 2))
        for a in (0, 1):
            for b in (0, 1):
                if msg[a, b] == 0.0:
                    continue
                assign = {latents[k - 1]: b}
                if k >= 2:
                    assign[latents[k - 2]] = a
                for c in (0, 1):
                    new[b, c] += msg[a, b] * factor(latents[k], c, assign)
        s = new.sum()
        msg, log_scale = new / s, log_scale + math.log(s)
    total = 0.0
    for a in (0, 1):
        for b in (0, 1):
            assign = {latents[n - 1]: b}
            if n >= 2:
                assign[latents[n - 2]] = a
            f = 1.0
            for name, value in x.items():
                f *= factor(name, value, assign)
            total += msg[a, b] * f
    return math.log(total) + log_scale


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--bond", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    torch.manual_seed(args.seed)
    bn, latents, observed, x = synthetic_network(args.n, 0)
    target = -exact_log_evidence(bn, latents, x)
    vi = SampledELBOVariationalInference(bn, latents, observed, {'bond_dim': args.bond, 'num_samples': args.samples, 'seed': args.seed},
                                         device=args.device)
    history = vi.train(x, args.epochs, args.lr, verbose=True)
    tail = float(np.mean(history['loss_elbo'][-10:]))
    print(f"n = {args.n}, D = {args.bond}, B = {args.samples}: loss (mean of the last 10 epochs) {tail:.6f}  against  -log p(x) = {target:.6f}"
          f"  (KL estimate {tail - target:.6f}; first epoch {history['loss_elbo'][0]:.6f})")


if __name__ == "__main__":
    main()
