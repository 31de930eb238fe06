#!/usr/bin/env python3
"""A chain and a tree on the 40-variable chain network: synthetic_network(40, 0) with the sampled ELBO trainer, two runs of the same
budget at bond D = 4: real MPS cores and tree-tensor-network cores (variables on the leaves in tuple order).  Each loss is an
estimate of KL(q || p(.|x)) - log p(x) and is printed beside -log p(x), computed exactly on the host
(run_chain_mps_sampled_elbo.exact_log_evidence).  Nothing is asserted about which wins.  No plotting.

    python examples/run_chain_ttn_elbo.py [--n 40] [--samples 4096] [--epochs 300] [--lr 0.02]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from run_chain_mps_sampled_elbo import exact_log_evidence                      # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference    # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    bn, latents, observed, x = synthetic_network(args.n, 0)
    target = -exact_log_evidence(bn, latents, x)
    print(f"n = {args.n}, B = {args.samples}, {args.epochs} epochs, lr {args.lr}: -log p(x) = {target:.6f}")
    for kind in ("real", "tree"):
        torch.manual_seed(args.seed)
        vi = SampledELBOVariationalInference(bn, latents, observed, {'bond_dim': 4, 'num_samples': args.samples, 'seed': args.seed,
                                                                      'cores': kind}, device=args.device)
        history = vi.train(x, args.epochs, args.lr, verbose=False)
        tail = float(np.mean(history['loss_elbo'][-10:]))
        print(f"{kind:>5} D = 4 ({vi.born_machine.num_parameters:5d} parameters): loss (mean of the last 10 epochs) "
              f"{tail:.6f}  KL estimate {tail - target:.6f}  (first epoch {history['loss_elbo'][0]:.6f}, worst status {max(history['status'])})")


if __name__ == "__main__":
    main()
