#!/usr/bin/env python3
"""Adaptive bond dimension: reverse-KL training on the 40-variable chain of the sampled examples (synthetic_network(40, 0),
B = 4096) where bond_dim is measured and changed between train() calls instead of being chosen blind:
  - fit at D = 2 and print bond_entropies(): how much of D every bond uses;
  - expand_(4, noise=1e-2) and train on from the fitted cores (nothing starts again);
  - compress_(cutoff=1e-8): back to the bond dimension the fit needs, with the discarded weight of every bond known;
after each stage the ranks, the discarded weights and the largest marginal error against forward-backward.  No plotting.

    python examples/run_chain_mps_adaptive_bond.py [--n 40] [--bond 2] [--grow 4] [--samples 4096] [--epochs 200] [--lr 0.02]
                                                   [--noise 1e-2] [--cutoff 1e-8]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from run_chain_mps_sampled_ksd import exact_marginals                         # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference    # noqa: E402


def report_stage(name, vi, latents, p1, report=None):
    bm = vi.born_machine
    post = vi.posterior_marginals()
    q1 = np.array([post[v] for v in latents])
    k = int(np.argmax(np.abs(q1 - p1)))
    spectrum = bm.bond_spectrum().cpu().numpy()
    ranks = (spectrum > 0).sum(axis=1)
    print(f"[{name}] D = {bm.bond_dim}: largest |q(z_k = 1) - p(z_k = 1 | x)| = {abs(q1[k] - p1[k]):.6f} at k = {k}")
    print(f"  ranks            {ranks.tolist()}")
    print(f"  bond entropies   {np.round(bm.bond_entropies().cpu().numpy(), 4).tolist()}")
    if report is not None:
        print(f"  kept             {report['rank'].cpu().tolist()}")
        print(f"  discarded weight {['%.1e' % d for d in report['discarded'].cpu().tolist()]}  (status {int(report['status'].item())})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--bond", type=int, default=2)
    ap.add_argument("--grow", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--noise", type=float, default=1e-2)
    ap.add_argument("--cutoff", type=float, default=1e-8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    torch.manual_seed(args.seed)
    bn, latents, observed, x = synthetic_network(args.n, 0)
    vi = SampledELBOVariationalInference(bn, latents, observed, {'bond_dim': args.bond, 'num_samples': args.samples, 'seed': args.seed},
                                         device=args.device)
    p1 = exact_marginals(bn, latents, x)
    vi.train(x, args.epochs, args.lr, verbose=False)
    report_stage(f"fit at D = {args.bond}", vi, latents, p1)
    vi.born_machine.expand_(args.grow, noise=args.noise, seed=args.seed)
    vi.train(x, args.epochs, args.lr, verbose=False)
    report_stage(f"expand_({args.grow}) and train on", vi, latents, p1)
    report = vi.born_machine.compress_(cutoff=args.cutoff)
    report_stage(f"compress_(cutoff={args.cutoff:g})", vi, latents, p1, report)


if __name__ == "__main__":
    main()
