#!/usr/bin/env python3
"""Two-site (DMRG-style) sweeps on the 40-variable chain of the sampled examples (synthetic_network(40, 0)): one MPS over all 41
sites (Z0 .. Z39 and the observed leaf X), started from the PRODUCT STATE at cap 8 and fitted to draws from the network by
train_two_site: every bond grows to the rank its spectrum shows.  Printed: the ranks and the bond entropies after the sweeps,
and the largest |q(z_k = 1 | X = x) - p(z_k = 1 | X = x)| against forward-backward for X = 0 and X = 1.  Beside it the same
budget of draws spent by train() (Adam on all cores at once) at the fixed bond dimension 8.  No plotting.

    python examples/run_chain_mps_two_site.py [--n 40] [--cap 8] [--samples 8192] [--sweeps 6] [--steps 5] [--lr 0.03] [--cutoff 1e-4]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from run_chain_mps_sampled_ksd import exact_marginals                         # noqa: E402
from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference     # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402


def marginal_errors(name, vi, bn, latents, observed):
    for xv in (0, 1):
        x = {observed[0]: xv}
        p1 = exact_marginals(bn, latents, x)
        post = vi.posterior_marginals(x)
        q1 = np.array([post[v] for v in latents])
        k = int(np.argmax(np.abs(q1 - p1)))
        print(f"[{name}] X = {xv}: largest |q(z_k = 1 | x) - p(z_k = 1 | x)| = {abs(q1[k] - p1[k]):.6f} at k = {k};  "
              f"log q(x) = {vi.log_evidence(x):.5f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--cap", type=int, default=8)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--sweeps", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.03)
    ap.add_argument("--cutoff", type=float, default=1e-4)
    ap.add_argument("--adam-lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    torch.manual_seed(args.seed)
    bn, latents, observed, _ = synthetic_network(args.n, 0)
    cfg = {'bond_dim': args.cap, 'num_samples': args.samples, 'seed': args.seed}
    vi = AmortisedMPSInference(bn, latents, observed, {**cfg, 'init_method': 'zero'}, device=args.device)      # 'zero': the uniform product state
    hist = vi.train_two_site(args.sweeps, args.lr, descent_steps=args.steps, cutoff=args.cutoff, verbose=True)
    bm = vi.born_machine
    print(f"[two-site] ranks          {hist['rank'][-1]}  (cap {args.cap}, status {hist['status'][-1]})")
    print(f"[two-site] bond entropies {np.round(bm.bond_entropies().cpu().numpy(), 4).tolist()}")
    print(f"[two-site] largest discarded weight of the last sweep {max(hist['discarded'][-1]):.2e}")
    marginal_errors("two-site", vi, bn, latents, observed)
    # the same budget: a sweep evaluates every sample 2 (n - 1) (steps + 1) times at one bond, an epoch once at all n sites
    epochs = args.sweeps * 2 * (args.steps + 1)
    torch.manual_seed(args.seed)
    ref = AmortisedMPSInference(bn, latents, observed, cfg, device=args.device)
    ref.train(epochs, args.adam_lr, verbose=False)
    print(f"[train(), D = {args.cap}, {epochs} epochs] bond entropies {np.round(ref.born_machine.bond_entropies().cpu().numpy(), 4).tolist()}")
    marginal_errors(f"train(), D = {args.cap}", ref, bn, latents, observed)


if __name__ == "__main__":
    main()
