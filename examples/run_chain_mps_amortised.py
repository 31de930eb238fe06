#!/usr/bin/env python3
"""Amortised inference on the 40-variable chain of the sampled examples (synthetic_network(40, 0)): one MPS over all 41
sites (Z0 .. Z39 and the observed leaf X) fitted to draws from the network, no observation given; then, from that one fit,
the largest |q(z_k = 1 | X = x) - p(z_k = 1 | X = x)| against forward-backward for X = 0 and for X = 1, and log q(X = x).
No plotting.

    python examples/run_chain_mps_amortised.py [--n 40] [--bond 4] [--samples 4096] [--epochs 300] [--lr 0.02] [--objective joint]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from run_chain_mps_sampled_ksd import exact_marginals                         # noqa: E402
from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference     # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--bond", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--objective", default="joint", choices=AmortisedMPSInference.OBJECTIVES)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    torch.manual_seed(args.seed)
    bn, latents, observed, _ = synthetic_network(args.n, 0)
    vi = AmortisedMPSInference(bn, latents, observed, {'bond_dim': args.bond, 'num_samples': args.samples, 'seed': args.seed},
                               device=args.device)
    vi.train(args.epochs, args.lr, objective=args.objective, verbose=True)
    for xv in (0, 1):
        x = {observed[0]: xv}
        p1 = exact_marginals(bn, latents, x)
        post = vi.posterior_marginals(x)
        q1 = np.array([post[name] for name in latents])
        k = int(np.argmax(np.abs(q1 - p1)))
        print(f"X = {xv}: largest |q(z_k = 1 | x) - p(z_k = 1 | x)| = {abs(q1[k] - p1[k]):.6f} at k = {k} of {args.n};  "
              f"log q(x) = {vi.log_evidence(x):.5f}")


if __name__ == "__main__":
    main()
