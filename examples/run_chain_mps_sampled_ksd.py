#!/usr/bin/env python3
"""KSD inference on a 40-variable chain, far past anything 2^n can hold: synthetic_network(40, 0) (an order-2 chain whose
posterior's square root is exactly an MPS of bond 4) with the sampled KSD trainer, D = 4, B = 4096 samples per epoch: the
Stein objective from the samples' own B^2 kernel values, no enumeration anywhere.  Prints the trace of U (the unbiased
estimate of q^T K_p q) and, at the end, the largest error of q's single-site marginals, estimated from the last epoch's
samples, against the exact posterior marginals by forward-backward along the chain (tree-width 2).  No plotting.

    python examples/run_chain_mps_sampled_ksd.py [--n 40] [--bond 4] [--samples 4096] [--epochs 300] [--lr 0.02]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.ksd_vi_sampled import SampledKSDVariationalInference  # noqa: E402


def exact_marginals(bn, latents, x):
    """p(z_k = 1 | x) for every k, of a network in which every node's parents lie among the two latents before it
    (synthetic_network): forward and backward messages over (z_{k-1}, z_k), renormalised at every step."""
    def factor(name, value, assign):
        pa = tuple(assign[p] for p in (bn.parents[name] if name in bn.parents else ()))
        return bn.cpts[name][pa][value]
    n = len(latents)
    F = [None] * n                      # F[k][a, b, c]: factor of z_k = c given z_{k-1} = b, z_{k-2} = a
    for k in range(1, n):
        F[k] = np.zeros((2, 2, 2))
        for a in (0, 1):
            for b in (0, 1):
                assign = {latents[k - 1]: b}
                if k >= 2:
                    assign[latents[k - 2]] = a
                for c in (0, 1):
                    F[k][a, b, c] = factor(latents[k], c, assign)
    alpha = [None] * n                  # alpha[k][a, b]: mass of (z_{k-1} = a, z_k = b) and the past; a is a dummy 0 at k = 0
    alpha[0] = np.zeros((2, 2))
    for b in (0, 1):
        alpha[0][0, b] = factor(latents[0], b, {})
    for k in range(1, n):
        new = np.einsum('ab,abc->bc', alpha[k - 1], F[k])
        alpha[k] = new / new.sum()
    beta = [None] * n                   # beta[k][a, b]: mass of the future and the evidence given (z_{k-1} = a, z_k = b)
    beta[n - 1] = np.ones((2, 2))
    for a in (0, 1):
        for b in (0, 1):
            assign = {latents[n - 1]: b}
            if n >= 2:
                assign[latents[n - 2]] = a
            for name, value in x.items():
                beta[n - 1][a, b] *= factor(name, value, assign)
    for k in range(n - 1, 0, -1):
        new = np.einsum('abc,bc->ab', F[k], beta[k])
        beta[k - 1] = new / new.sum()
    out = np.zeros(n)
    for k in range(n):
        m = (alpha[k] * beta[k]).sum(axis=0)
        out[k] = m[1] / m.sum()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--bond", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--length-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    torch.manual_seed(args.seed)
    bn, latents, observed, x = synthetic_network(args.n, 0)
    vi = SampledKSDVariationalInference(bn, latents, observed, {'bond_dim': args.bond, 'num_samples': args.samples, 'seed': args.seed},
                                        base_kernel_length_scale=args.length_scale, device=args.device)
    history = vi.train(x, args.epochs, args.lr, verbose=True)
    trace = history['loss_ksd2']
    step = max(1, args.epochs // 10)
    print("U trace: " + "  ".join(f"[{e}] {trace[e]:.4e}" for e in list(range(0, args.epochs, step)) + [args.epochs - 1]))
    idx = vi.last_idx.cpu().numpy()
    bits = (idx[:, None] >> (args.n - 1 - np.arange(args.n))[None, :]) & 1
    q1 = bits.mean(axis=0)
    p1 = exact_marginals(bn, latents, x)
    k = int(np.argmax(np.abs(q1 - p1)))
    print(f"n = {args.n}, D = {args.bond}, B = {args.samples}: U (mean of the last 10 epochs) {float(np.mean(trace[-10:])):.4e} "
          f"(first epoch {trace[0]:.4e}); largest single-site marginal error |q(z_k = 1) - p(z_k = 1 | x)| = "
          f"{abs(q1[k] - p1[k]):.4f} at k = {k}, mean over the sites {float(np.mean(np.abs(q1 - p1))):.4f} "
          f"(sampling error of the estimate about {0.5 / np.sqrt(args.samples):.4f})")


if __name__ == "__main__":
    main()
