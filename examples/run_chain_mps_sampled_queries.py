#!/usr/bin/env python3
"""Reading the fitted posterior out exactly: reverse-KL training on the 40-variable chain of the sampled examples
(synthetic_network(40, 0), D = 4, B = 4096), then the trained machine's exact queries, none of which touches 2^n or a sample:
  - the largest |q(z_k = 1) - p(z_k = 1 | x)| from marginals(), beside the same error estimated from B samples;
  - one conditional, q(z_j = 1 | z_i = 1) = m2[i, j] / m1[i] from pair_marginals(), against forward-backward along the chain
    with z_i = 1 added to the evidence;
  - 8 draws from sample_given({z_i: 1}) with their conditional log-probabilities and the evidence's log marginal.
No plotting.

    python examples/run_chain_mps_sampled_queries.py [--n 40] [--bond 4] [--samples 4096] [--epochs 300] [--lr 0.02] [--i 10] [--j 12]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from run_chain_mps_sampled_ksd import exact_marginals                         # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference    # noqa: E402


def exact_conditional(bn, latents, x, i, j):
    """p(z_j = 1 | z_i = 1, x) for i < j on the chain of exact_marginals: the same forward and backward messages over
    (z_{k-1}, z_k), with the forward message at k = i kept on z_i = 1 only."""
    def factor(name, value, assign):
        pa = tuple(assign[p] for p in (bn.parents[name] if name in bn.parents else ()))
        return bn.cpts[name][pa][value]
    n = len(latents)

    def transition(k):
        F = np.zeros((2, 2, 2))           # F[a, b, c]: factor of z_k = c given z_{k-1} = b, z_{k-2} = a
        for a in (0, 1):
            for b in (0, 1):
                assign = {latents[k - 1]: b}
                if k >= 2:
                    assign[latents[k - 2]] = a
                for c in (0, 1):
                    F[a, b, c] = factor(latents[k], c, assign)
        return F
    alpha = np.zeros((2, 2))
    for b in (0, 1):
        alpha[0, b] = factor(latents[0], b, {})
    if i == 0:
        alpha[:, 0] = 0.0
    for k in range(1, j + 1):
        alpha = np.einsum('ab,abc->bc', alpha, transition(k))
        if k == i:
            alpha[:, 0] = 0.0
        alpha /= alpha.sum()
    beta = np.ones((2, 2))
    for a in (0, 1):
        for b in (0, 1):
            assign = {latents[n - 1]: b}
            if n >= 2:
                assign[latents[n - 2]] = a
            for name, value in x.items():
                beta[a, b] *= factor(name, value, assign)
    for k in range(n - 1, j, -1):
        beta = np.einsum('abc,bc->ab', transition(k), beta)
        beta /= beta.sum()
    m = (alpha * beta).sum(axis=0)
    return m[1] / m.sum()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--bond", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--i", type=int, default=10)
    ap.add_argument("--j", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if not 0 <= args.i < args.j < args.n:
        raise SystemExit("--i and --j: 0 <= i < j < n")
    import torch
    torch.manual_seed(args.seed)
    bn, latents, observed, x = synthetic_network(args.n, 0)
    vi = SampledELBOVariationalInference(bn, latents, observed, {'bond_dim': args.bond, 'num_samples': args.samples, 'seed': args.seed},
                                         device=args.device)
    vi.train(x, args.epochs, args.lr, verbose=True)
    p1 = exact_marginals(bn, latents, x)
    post = vi.posterior_marginals()
    q1 = np.array([post[name] for name in latents])
    idx = vi.last_idx.cpu().numpy()
    s1 = ((idx[:, None] >> (args.n - 1 - np.arange(args.n))[None, :]) & 1).mean(axis=0)
    k = int(np.argmax(np.abs(q1 - p1)))
    print(f"n = {args.n}, D = {args.bond}: largest |q(z_k = 1) - p(z_k = 1 | x)| = {abs(q1[k] - p1[k]):.6f} at k = {k} from marginals() "
          f"(exact in q);  the same from the last epoch's {args.samples} samples: {np.abs(s1 - p1).max():.6f} "
          f"(their own error against q: {np.abs(s1 - q1).max():.6f}, about {0.5 / np.sqrt(args.samples):.4f} expected)")
    m1, m2 = vi.born_machine.pair_marginals()
    cond_q = float(m2[args.i, args.j] / m1[args.i])
    cond_p = exact_conditional(bn, latents, x, args.i, args.j)
    print(f"q({latents[args.j]} = 1 | {latents[args.i]} = 1) = m2 / m1 = {cond_q:.6f}  against forward-backward with "
          f"{latents[args.i]} = 1 in the evidence: {cond_p:.6f}  (q({latents[args.j]} = 1) = {q1[args.j]:.6f})")
    draws, logq, logm = vi.posterior_sample_given({latents[args.i]: 1}, 8)
    print(f"8 draws from q(. | {latents[args.i]} = 1), log q({latents[args.i]} = 1) = {float(logm.item()):.6f}:")
    for z, lq in zip(draws.cpu().tolist(), logq.cpu().tolist()):
        print(f"  {z:0{args.n}b}  log q(z | evidence) = {lq:.4f}")


if __name__ == "__main__":
    main()
