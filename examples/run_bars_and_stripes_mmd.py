#!/usr/bin/env python3
"""MMD training from data on the 3 x 3 Bars-and-Stripes set (n = 9, 14 patterns, generated here): the quantum Born machine
(exact MMD^2 through two Walsh-Hadamard transforms per epoch) and the sampled MPS at bond 4 (the unbiased estimate from
integer pair counts).  Prints each machine's loss trace and its final TVD against the uniform distribution over the patterns.
No plotting.

    python examples/run_bars_and_stripes_mmd.py [--epochs 300] [--layers 6] [--samples 2048] [--lr 0.05]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def bars_and_stripes(side=3):
    """The patterns as bit rows [P, side^2]: every choice of filled rows and of filled columns (all-0 and all-1 counted once)."""
    rows = set()
    for mask in range(1 << side):
        line = [(mask >> i) & 1 for i in range(side)]
        rows.add(tuple(np.repeat(line, side)))          # bars: whole rows
        rows.add(tuple(np.tile(line, side)))            # stripes: whole columns
    return np.array(sorted(rows), dtype=np.int64)


def trace(name, losses, every):
    print(f"{name}: loss_mmd2 " + " ".join(f"{v:.3e}" for v in losses[::every]) + f" ... {losses[-1]:.3e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    from tensornetworks_amd import QuantumMMDTrainer, SampledMMDTrainer
    data = torch.from_numpy(bars_and_stripes(3))
    n = data.shape[1]
    idx = (data * (1 << torch.arange(n - 1, -1, -1))).sum(dim=1)
    target = torch.bincount(idx, minlength=1 << n).double() / len(idx)
    every = max(1, args.epochs // 10)
    print(f"3 x 3 Bars-and-Stripes: n = {n}, {len(idx)} patterns, {args.epochs} epochs, lr {args.lr}")

    torch.manual_seed(args.seed)
    qvi = QuantumMMDTrainer(n, args.layers, "hardware_efficient", pytorch_device=args.device)
    hist = qvi.train(data, args.epochs, args.lr, verbose=False, target_for_tvd=target.to(args.device))
    trace(f"quantum (hardware_efficient, {args.layers} layers)", hist['loss_mmd2'], every)
    print(f"  final TVD to the uniform distribution over the patterns: {hist['tvd'][-1]:.4f} (first epoch {hist['tvd'][0]:.4f})")

    torch.manual_seed(args.seed)
    svi = SampledMMDTrainer(n, {'bond_dim': 4, 'num_samples': args.samples, 'seed': args.seed}, device=args.device)
    hist = svi.train(data, args.epochs, args.lr, verbose=False, target_for_tvd=target)
    trace(f"sampled MPS (D = 4, B = {args.samples}; the estimate U)", hist['loss_mmd2'], every)
    trace("sampled MPS, exact MMD^2 of the enumerated q", hist['mmd2_exact'], every)
    print(f"  final TVD to the uniform distribution over the patterns: {hist['tvd'][-1]:.4f} (first epoch {hist['tvd'][0]:.4f})")


if __name__ == "__main__":
    main()
