#!/usr/bin/env python3
"""The natural-gradient step against the plain KSD steps of the quantum trainer on the MI355X (GPU only: fails without one).

Per size (default n = 16, L = 6 and n = 20, L = 8; synthetic_network(n, 0), hardware_efficient) three trainers are built in
the same process on the same card and their device steps (ksd_and_grad: circuits, contraction, gradient, and for the third
the Fisher matrix and the solve) are timed in alternation with device events: the stored-rows step (fused_dot = False,
the route natural gradient builds on), the fused step, the natural-gradient step.  Reported per kind: the median of the
block means with the smallest and largest block.  Also: bornvi_fisher_gram alone (with its TFLOP/s, counting the computed
tiles: 2 x 64 x 64 x tiles x 2^n flop) and bornvi_spd_solve alone, on the step's own rows, q and gradient.

    python tools/natgrad_time.py [--sizes 16:6 20:8] [--blocks 10] [--reps 20] [--warmup 5]
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
    vis = {}
    for name, kw in (("stored", {}), ("fused", {}), ("natgrad", {"natural_gradient": True})):
        torch.manual_seed(0)
        vi = KSDVariationalInference(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, pytorch_device="cuda:0", **kw)
        vi.fused_dot = name == "fused"
        if vis:                                   # one Stein side for the three (K_p is the largest buffer)
            for attr in ("_S", "_K", "_K_rows", "_K_pairs", "_K_sig", "_K_form", "_stein_key"):
                setattr(vi, attr, getattr(vis["stored"], attr))
        else:
            vi._prepare_stein(x)
        vis[name] = vi
    for _ in range(warmup):
        for vi in vis.values():
            vi.ksd_and_grad()
    torch.cuda.synchronize()
    t = {k: [] for k in vis}
    for _ in range(blocks):
        for k, vi in vis.items():
            t[k].append(timed(vi.ksd_and_grad, reps))
    nat = vis["natgrad"]
    P = nat.born_machine.num_ansatz_params
    dev = torch.device("cuda", 0)
    theta64 = nat.born_machine.theta.detach().double().contiguous()
    probs = backend.paramshift_probs("hardware_efficient", n, L, theta64, 0, P, include_base=True)
    q, rows = probs[0], probs[1:]
    g = vis["stored"].ksd_and_grad()[1]
    F = backend.fisher_gram(rows, q, nat.natural_gradient.q_floor)
    gram = [timed(lambda: backend.fisher_gram(rows, q, nat.natural_gradient.q_floor, out=F), reps) for _ in range(blocks)]
    solve = [timed(lambda: backend.spd_solve(F, g, nat.natural_gradient.damping), reps) for _ in range(blocks)]
    _, info = backend.spd_solve(F, g, nat.natural_gradient.damping)
    tiles = -(-P // 64) * (-(-P // 64) + 1) // 2
    flop = 2.0 * 64 * 64 * tiles * (1 << n)
    gm = statistics.median(gram)
    return {"n": n, "L": L, "P": P, "gram_form": nat._K_form, "blocks": blocks, "reps": reps,
            "fused_dot": bool(backend.paramshift_dot_supported("hardware_efficient", n, L, dev, P)),
            "stored_step": summary(t["stored"]), "fused_step": summary(t["fused"]), "natgrad_step": summary(t["natgrad"]),
            "fisher_gram": summary(gram), "fisher_gram_tflops": round(flop / gm * 1e-9, 2),
            "fisher_rows_read_GBps": round(2.0 * P * 8 * (1 << n) / gm * 1e-6, 1),
            "spd_solve": summary(solve), "solve_info": int(info)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["16:6", "20:8"], help="n:L pairs")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("natgrad_time.py needs an MI355X (torch.cuda.is_available() is False)")
    for s in args.sizes:
        n, L = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, L, args.blocks, args.reps, args.warmup)), flush=True)
        backend.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
