#!/usr/bin/env python3
"""The reference's classical experiment on this engine: KSD variational inference of P(C, S, R | W = 1) in the Sprinkler
network with the classical Born machine (run_sprinkler_ksd.py of the reference: an MLP of x with conditioning_dim 1,
Adam lr = 0.003 with cosine annealing, clip 5, entropy weight 0.001, patience 200, 2000 epochs; the trainer forces the
small_random initialisation).  Prints the learned distribution beside the exact posterior and the TVD statistics the
reference prints; no plotting.

    python examples/run_sprinkler_ksd.py [--epochs 2000] [--device cuda:0] [--quiet]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd.bayesian_network import get_sprinkler_network          # noqa: E402
from tensornetworks_amd.ksd_vi import KSDVariationalInference                 # noqa: E402
from tensornetworks_amd.utils import calculate_tvd                            # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=0, help="torch seed of the initialisation and the Dropout draws")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()

    import torch
    torch.manual_seed(args.seed)
    latent, observed, evidence = ["C", "S", "R"], ["W"], {"W": 1}
    network = get_sprinkler_network(random_cpts=False)
    posterior, p_evidence = network.get_true_posterior(latent, evidence)
    print(f"Sprinkler network, evidence {evidence}: P(evidence) = {p_evidence:.4f}")
    if p_evidence < 1e-9:
        raise SystemExit("the evidence has probability zero under the network")

    config = {"use_logits": True, "conditioning_dim": len(observed), "init_method": "uniform", "hidden_dims": None,
              "use_layer_norm": False}
    vi = KSDVariationalInference(bayesian_network=network, latent_vars_names=latent, observed_vars_names=observed,
                                 born_machine_config=config, base_kernel_length_scale=1.0, device=args.device)
    n_params = sum(p.numel() for p in vi.born_machine.parameters() if p.requires_grad)
    print(f"Classical Born machine: MLP of x, {n_params} parameters; Adam lr 0.003 with cosine annealing, clip 5, "
          f"entropy weight 0.001, patience 200, {args.epochs} epochs on {args.device}")

    t0 = time.perf_counter()
    history = vi.train(x_observation_dict=evidence, num_epochs=args.epochs, lr_born_machine=0.003, verbose=not args.quiet,
                       true_posterior_for_tvd=posterior, use_lr_scheduler=True, gradient_clip_norm=5.0,
                       optimizer_type="adam", adam_betas=(0.9, 0.999), entropy_weight=0.001, patience=200)
    seconds = time.perf_counter() - t0

    x = torch.tensor([evidence[nm] for nm in observed], dtype=torch.float32, device=args.device)
    learned = vi.born_machine.get_prob_dict(x_condition=x)
    print(f"\n{'outcome ' + str(tuple(latent)):<22} | {'true P(z|x)':<13} | {'learned Q(z|x)':<15} | difference")
    print("-" * 70)
    worst = 0.0
    for z in sorted(posterior):
        p, q = posterior.get(z, 0.0), float(learned.get(z, 0.0))
        worst = max(worst, abs(p - q))
        print(f"{str(z):<22} | {p:<13.6f} | {q:<15.6f} | {abs(p - q):.6f}")
    tvd = np.asarray(history["tvd"], dtype=np.float64)
    epochs_run = len(history["loss_ksd"])
    print(f"\nFinal TVD: {calculate_tvd(posterior, learned):.6f}   max pointwise difference: {worst:.6f}")
    print(f"Best TVD during training: {tvd.min():.6f} (epoch {int(tvd.argmin()) + 1})   mean {tvd.mean():.6f}   "
          f"std {tvd.std():.6f}   mean of the last 100 epochs {tvd[-100:].mean():.6f}")
    print(f"KSD loss: first {history['loss_ksd'][0]:.6f}, last {history['loss_ksd'][-1]:.6f}; "
          f"{epochs_run} epochs in {seconds:.2f} s ({epochs_run / seconds:.0f} epochs/s)")


if __name__ == "__main__":
    main()
