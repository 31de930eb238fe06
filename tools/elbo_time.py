#!/usr/bin/env python3
"""One ELBO step against one KSD step of the quantum trainers on the MI355X (GPU only: fails without one).

For each (n, L) (synthetic_network(n, 0), hardware_efficient, theta0 = 0.1 N(0, 1) seeded) both trainers are built in the
same process on the same card and their device steps (elbo_and_grad / ksd_and_grad: circuits, the objective's piece, the
gradient) are timed ALTERNATELY: `blocks` blocks of `reps` steps each per trainer, device events around a block, after
warm-up.  Prints one JSON line per size: the median of the block means and [smallest, largest block] for each, their
difference, the ELBO piece alone (bornvi_elbo_weights) and the KSD contraction alone.

    python tools/elbo_time.py [--sizes 16:6 20:8] [--blocks 10] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_quantum import ELBOVariationalInference       # noqa: E402
from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference         # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def measure(n, L, blocks, reps, warmup):
    bn, lat, obs, x = synthetic_network(n, 0)
    torch.manual_seed(0)
    ksd = KSDVariationalInference(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, pytorch_device="cuda:0")
    torch.manual_seed(0)
    elbo = ELBOVariationalInference(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, pytorch_device="cuda:0")
    assert torch.equal(ksd.born_machine.theta, elbo.born_machine.theta)
    ksd._prepare_stein(x)
    elbo.objective.prepare(x)
    for _ in range(warmup):
        ksd.ksd_and_grad()
        elbo.elbo_and_grad()
    torch.cuda.synchronize()
    t = {"ksd": [], "elbo": []}
    for _ in range(blocks):
        t["ksd"].append(timed(ksd.ksd_and_grad, reps))
        t["elbo"].append(timed(elbo.elbo_and_grad, reps))
    q = elbo.elbo_and_grad()[2]
    piece = [timed(lambda: elbo.objective.weights(q), 10 * reps) for _ in range(3)]
    contraction = [timed(lambda: ksd._stein_contract(q), reps) for _ in range(3)]
    dev = q.device
    P = elbo.born_machine.num_ansatz_params
    return {"n": n, "L": L, "P": P, "gram": ksd._K_form, "blocks": blocks, "reps": reps,
            "fused_dot": bool(backend.paramshift_dot_supported("hardware_efficient", n, L, dev, P)),
            "ksd_step": summary(t["ksd"]), "elbo_step": summary(t["elbo"]),
            "ksd_minus_elbo_ms": round(statistics.median(t["ksd"]) - statistics.median(t["elbo"]), 4),
            "elbo_weights": summary(piece), "ksd_contraction": summary(contraction)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["16:6", "20:8"], help="n:L pairs")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("elbo_time.py needs an MI355X (torch.cuda.is_available() is False)")
    for s in args.sizes:
        n, L = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, L, args.blocks, args.reps, args.warmup)), flush=True)
        backend.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
