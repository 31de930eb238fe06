#!/usr/bin/env python3
"""The ELBO Sprinkler experiment of run_sprinkler_quantum_natgrad.py with the quantum natural gradient beside the other
two: variational inference of P(C, S, R | W = 1) with a 3-qubit Born machine (hardware_efficient ansatz, 4 layers), trained
on the exact ELBO by plain gradient descent (no momentum, constant rate, clip 10) along the raw parameter-shift gradient,
along (F + damping I)^-1 g with F the classical Fisher matrix of q_theta, and along (Q + damping I)^-1 g with Q the quantum
Fisher information of the circuit (4 x the Fubini-Study metric; natural_gradient.QuantumFisherPreconditioner).  The runs
start from the same parameters; prints the final KL and TVD of each.

    python examples/run_sprinkler_quantum_qng.py [--epochs 40] [--lr 0.3] [--damping 1e-3] [--device cuda:0]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd.bayesian_network import get_sprinkler_network          # noqa: E402
from tensornetworks_amd.elbo_vi_quantum import ELBOVariationalInference       # noqa: E402
from tensornetworks_amd.utils import calculate_tvd                            # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.3)
    ap.add_argument("--damping", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0, help="torch seed of the small_random initialisation")
    args = ap.parse_args()

    import torch
    latent, observed, evidence = ["C", "S", "R"], ["W"], {"W": 1}
    network = get_sprinkler_network(random_cpts=False)
    posterior, p_evidence = network.get_true_posterior(latent, evidence)
    print(f"Sprinkler network, evidence {evidence}: P(evidence) = {p_evidence:.4f}; plain gradient descent, lr {args.lr}, "
          f"clip 10, {args.epochs} epochs on {args.device}")
    from tensornetworks_amd.natural_gradient import QuantumFisherPreconditioner
    for name, natgrad in (("plain gradient", None), (f"natural gradient (damping {args.damping})", args.damping),
                          (f"quantum natural gradient ({args.damping})", QuantumFisherPreconditioner(args.damping))):
        torch.manual_seed(args.seed)
        vi = ELBOVariationalInference(bayesian_network=network, latent_vars_names=latent, observed_vars_names=observed,
                                      qbm_num_latent_vars=len(latent), qbm_ansatz_layers=args.layers,
                                      qbm_ansatz_type="hardware_efficient", qbm_init_method="small_random",
                                      pytorch_device=args.device, natural_gradient=natgrad)
        vi.objective.prepare(evidence)
        params = list(vi.born_machine.parameters())
        optimizer = torch.optim.SGD(params, lr=args.lr, momentum=0.0)
        t0 = time.perf_counter()
        failed = 0
        for _ in range(args.epochs):
            vi.training_step(params, optimizer, None, 10.0)
            if natgrad is not None:
                failed += int(vi._natgrad_info) != 0
        kl = float(vi.elbo_and_grad()[0]) + vi.objective.log_evidence
        seconds = time.perf_counter() - t0
        tvd = calculate_tvd(posterior, vi.born_machine.get_prob_dict(x_condition=None))
        extra = f", {failed} epochs fell back to the plain gradient" if natgrad is not None else ""
        print(f"{name:<36}: final KL {kl:.3e}   final TVD {tvd:.3e}   ({seconds:.2f} s{extra})")


if __name__ == "__main__":
    main()
