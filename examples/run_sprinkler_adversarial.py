#!/usr/bin/env python3
"""The reference's adversarial experiment on this engine: adversarial (KL) variational inference of P(C, S, R | W = 1)
in the Sprinkler network with the classical Born machine (run_sprinkler_adversarial.py of the reference: an MLP of x
with conditioning_dim 1, classifier 32-16, batch 100, Adam lr 0.003 / 0.03 with cosine annealing and betas (0.5, 0.999),
5 classifier steps per Born step, clip 5, baseline decay 0.95, 1500 epochs; the trainer forces the small_random
initialisation).  Prints the learned distribution beside the exact posterior, the TVD statistics and the stability
lines the reference prints; no plotting.

    python examples/run_sprinkler_adversarial.py [--epochs 1500] [--device cuda:0] [--table] [--quiet]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd.adversarial_vi_classical import AdversarialVariationalInference   # noqa: E402
from tensornetworks_amd.bayesian_network import get_sprinkler_network                       # noqa: E402
from tensornetworks_amd.utils import calculate_tvd                                         # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--epochs", type=int, default=1500)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=0, help="torch seed of the initialisation, the samples and Dropout")
    ap.add_argument("--table", action="store_true", help="probability table (conditioning_dim 0) instead of the MLP of x")
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

    config = {"use_logits": True, "conditioning_dim": 0 if args.table else len(observed), "init_method": "uniform"}
    vi = AdversarialVariationalInference(bayesian_network=network, latent_vars_names=latent, observed_vars_names=observed,
                                         born_machine_config=config,
                                         classifier_config={"hidden_dims": [32, 16], "use_batch_norm": False},
                                         device=args.device)
    n_params = sum(p.numel() for p in vi.born_machine.parameters() if p.requires_grad)
    print(f"Classical Born machine: {'table' if args.table else 'MLP of x'}, {n_params} parameters; batch 100, Adam lr 0.003 / "
          f"0.03 with cosine annealing, betas (0.5, 0.999), clip 5, baseline decay 0.95, {args.epochs} epochs on {args.device}")

    t0 = time.perf_counter()
    history = vi.train(x_observation_dict=evidence, num_epochs=args.epochs, batch_size=100, lr_born_machine=0.003,
                       lr_classifier=0.03, k_classifier_steps=5, k_born_steps=1, verbose=not args.quiet,
                       true_posterior_for_tvd=posterior, use_lr_scheduler=True, gradient_clip_norm=5.0,
                       baseline_decay=0.95, optimizer_type="adam", adam_betas=(0.5, 0.999))
    seconds = time.perf_counter() - t0

    x = torch.tensor([evidence[nm] for nm in observed], dtype=torch.float32, device=args.device)
    learned = vi.born_machine.get_prob_dict(x_condition=None if args.table else x)
    print(f"\n{'outcome ' + str(tuple(latent)):<22} | {'true P(z|x)':<13} | {'learned Q(z|x)':<15} | difference")
    print("-" * 70)
    worst = 0.0
    for z in sorted(posterior):
        p, q = posterior.get(z, 0.0), float(learned.get(z, 0.0))
        worst = max(worst, abs(p - q))
        print(f"{str(z):<22} | {p:<13.6f} | {q:<15.6f} | {abs(p - q):.6f}")
    tvd = np.asarray(history["tvd"], dtype=np.float64)
    print(f"\nFinal TVD: {calculate_tvd(posterior, learned):.6f}   max pointwise difference: {worst:.6f}")
    print(f"Best TVD during training: {tvd.min():.6f} (epoch {int(tvd.argmin()) + 1})   mean {tvd.mean():.6f}   "
          f"std {tvd.std():.6f}   mean of the last 100 epochs {tvd[-100:].mean():.6f}")
    if len(tvd) > 200:
        early, late = tvd[:100].std(), tvd[-100:].std()
        print(f"Stability: TVD std of the first 100 epochs {early:.6f}, of the last 100 epochs {late:.6f}")
        if late > 2 * early:
            print("Warning: Training became less stable over time.")
    skipped = int(np.isnan(history["loss_born_machine"]).sum())
    print(f"{len(tvd)} epochs in {seconds:.2f} s ({len(tvd) / seconds:.0f} epochs/s), {vi.graphed_epochs} of them replayed "
          f"from a HIP graph, {skipped} Born updates skipped")


if __name__ == "__main__":
    main()
