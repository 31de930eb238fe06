#!/usr/bin/env python3
"""The matrix-free full-matrix natural gradient of the sampled MPS Born machine on the 40-variable chain
(synthetic_network(40, 0), D = 4, B = 4096): P = 2 n D^2 = 1280 parameters and 4096 samples, more than blocks='full' can
factor in parameter space and more than 'sample' can factor in sample space, so the step is solved by conjugate gradients
(natural_gradient='cg', natural_gradient.CGFisherPreconditioner: one tangent sweep and one score gradient per iteration, no
matrix).  Each trainer runs with the plain gradient, with the site blocks ('site') and with 'cg'; same seeds, same optimiser.
The columns are those of run_chain_mps_sampled_natgrad_full.py, and for 'cg' the iterations per epoch.  Prints what comes
out; no plotting.

    python examples/run_chain_mps_sampled_natgrad_cg.py [--n 40] [--bond 4] [--samples 4096] [--epochs 300] [--lr 0.02]
                                                        [--damping 1e-3] [--max-iters 32] [--rel-tol 1e-6]"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]
from run_chain_mps_sampled_elbo import exact_log_evidence                     # noqa: E402
from run_chain_mps_sampled_ksd import exact_marginals                         # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference  # noqa: E402
from tensornetworks_amd.ksd_vi_sampled import SampledKSDVariationalInference  # noqa: E402
from tensornetworks_amd.natural_gradient import CGFisherPreconditioner, SampledFisherPreconditioner  # noqa: E402


def runs(values):
    """[32, 32, 32, 17] -> '3 x 32, 1 x 17': the per-epoch counts, equal neighbours folded."""
    out = []
    for v in values:
        if out and out[-1][1] == v:
            out[-1][0] += 1
        else:
            out.append([1, v])
    return ", ".join(f"{c} x {v}" for c, v in out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--bond", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--damping", type=float, default=1e-3)
    ap.add_argument("--max-iters", type=int, default=CGFisherPreconditioner.MAX_ITERS)
    ap.add_argument("--rel-tol", type=float, default=CGFisherPreconditioner.REL_TOL)
    ap.add_argument("--optimizer", default="adam", choices=("adam", "sgd"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    import torch
    bn, latents, observed, x = synthetic_network(args.n, 0)
    target = -exact_log_evidence(bn, latents, x)
    p1 = exact_marginals(bn, latents, x)
    cfg = {'bond_dim': args.bond, 'num_samples': args.samples, 'seed': args.seed}
    for name, cls, key in (("ELBO", SampledELBOVariationalInference, 'loss_elbo'), ("KSD", SampledKSDVariationalInference, 'loss_ksd2')):
        for label in ("plain", "site", "cg"):
            ng = {"plain": None, "site": SampledFisherPreconditioner(damping=args.damping),
                  "cg": CGFisherPreconditioner(damping=args.damping, max_iters=args.max_iters, rel_tol=args.rel_tol)}[label]
            torch.manual_seed(args.seed)
            vi = cls(bn, latents, observed, cfg, device=args.device, natural_gradient=ng)
            history = vi.train(x, args.epochs, args.lr, verbose=False, optimizer_type=args.optimizer)
            tail = float(np.mean(history[key][-10:]))
            idx = vi.last_idx.cpu().numpy()
            bits = (idx[:, None] >> (args.n - 1 - np.arange(args.n))[None, :]) & 1
            err = np.abs(bits.mean(axis=0) - p1)
            how = "plain gradient" if ng is None else (f"natural gradient '{label}' (damping {args.damping:g}, fallbacks to the plain "
                                                       f"gradient {sum(history['natgrad_info'])})")
            what = (f"loss {tail:.6f} against -log p(x) = {target:.6f} (KL estimate {tail - target:.6f})" if name == "ELBO"
                    else f"U {tail:.4e} (-log p(x) = {target:.6f})")
            print(f"{name}, {how}: first epoch {history[key][0]:.6g}, mean of the last 10 of {args.epochs} epochs: {what}; largest "
                  f"single-site marginal error {err.max():.4f} at k = {int(err.argmax())}, mean {err.mean():.4f} "
                  f"(sampling error about {0.5 / np.sqrt(args.samples):.4f}); status {max(history['status'])}", flush=True)
            if label == "cg":
                it = history['natgrad_iters']
                capped = sum(1 for k in it if k >= args.max_iters)
                print(f"  CG iterations per epoch (max_iters {args.max_iters}, rel_tol {args.rel_tol:g}): min {min(it)}, median "
                      f"{int(np.median(it))}, max {max(it)}, epochs that used all of them {capped} of {len(it)}; last relres "
                      f"{float(ng.relres.item()):.3e}\n  per epoch: {runs(it)}", flush=True)


if __name__ == "__main__":
    main()
