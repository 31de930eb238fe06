#!/usr/bin/env python3
"""Amortised inference on Sprinkler: ONE fit of an MPS over (C, S, R, W) to draws from the network itself, no observation
given, then the posterior of every evidence read out of it: for every value of W and of (S, W) the table q(free | x) beside
get_true_posterior's, and log q(x) beside log p(x).  No plotting.

    python examples/run_sprinkler_amortised_mps.py [--bond 4] [--samples 8192] [--epochs 200] [--lr 0.05] [--objective joint]"""
import argparse
import itertools
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference     # noqa: E402
from tensornetworks_amd.bayesian_network import get_sprinkler_network         # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bond", type=int, default=4)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--objective", default="joint", choices=AmortisedMPSInference.OBJECTIVES)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    torch.manual_seed(args.seed)
    bn = get_sprinkler_network(False)
    vi = AmortisedMPSInference(bn, ['C', 'S', 'R'], ['W'], {'bond_dim': args.bond, 'num_samples': args.samples, 'seed': args.seed},
                               device=args.device)
    print(f"KL(p || q) before: {vi.exact_forward_kl():.6f}")
    vi.train(args.epochs, args.lr, objective=args.objective, verbose=True)
    print(f"KL(p || q) after {args.epochs} epochs of {args.samples} draws: {vi.exact_forward_kl():.6f}")
    evidences = [{'W': w} for w in (0, 1)] + [{'S': s, 'W': w} for s in (0, 1) for w in (0, 1)]
    for x in evidences:
        free = vi.free_names(x)
        post, px = bn.get_true_posterior(free, x)
        states = list(itertools.product((0, 1), repeat=len(free)))
        logq = vi.posterior_log_prob(x, states).cpu().tolist()
        print(f"evidence {x}:  log q(x) = {vi.log_evidence(x):.5f}   log p(x) = {math.log(px):.5f}")
        print(f"  {''.join(free):>6}  q(. | x)   p(. | x)")
        for z, lq in zip(states, logq):
            print(f"  {''.join(map(str, z)):>6}  {math.exp(lq):.6f}   {post[z]:.6f}")
        tvd = 0.5 * sum(abs(math.exp(lq) - post[z]) for z, lq in zip(states, logq))
        print(f"  TVD = {tvd:.6f}")


if __name__ == "__main__":
    main()
