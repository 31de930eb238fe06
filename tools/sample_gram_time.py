#!/usr/bin/env python3
"""The sample-space natural gradient's three calls and the whole epoch on the MI355X (GPU only: fails without one).

For each (n, D, B), in one process on one card, after warm-up: mps_score_sample_gram, spd_solve of the B x B system, the
second mps_score_vjp, and the device part of an ELBO epoch (SampledELBOVariationalInference.loss_and_grad) with the plain
gradient, with natural_gradient='site' (where 2 D^2 <= 1024: else "refused") and with natural_gradient='sample', timed
ALTERNATELY in `blocks` blocks of `reps` calls each (device events around a block); medians over the blocks with minima and
maxima -- the method of tools/sampled_natgrad_time.py.  Beside each time, FLOPs by construction: the Gram issues two
16 x 16 x 4 matrix-core products per D4 / 4 steps, site and fragment pair, over the 32 x 32 tiles on or above the diagonal
(`issued_flops`; the useful part is B^2 n 4 D4 / 2 for the upper triangle, `flops`), the Cholesky B^3 / 3.  Prints one JSON
line per size; the record kept in the repository:

    python tools/sample_gram_time.py > profiles/sample_gram_time.jsonl

    python tools/sample_gram_time.py [--sizes 16:4:1024 40:4:1024 63:8:1024 63:16:1024 63:32:1024] [--blocks 5] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sampled_natgrad_time import summary, timed                               # noqa: E402
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference  # noqa: E402


def measure(n, D, B, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    bn, lat, obs, x = synthetic_network(n, 0)
    trainers = {}
    for name, spec in (("plain", None), ("site", "site"), ("sample", "sample")):
        torch.manual_seed(0)
        try:
            vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 1}, device='cuda:0',
                                                 natural_gradient=spec)
        except ValueError as e:
            trainers[name] = str(e)
            continue
        vi._prepare_observation(x)
        trainers[name] = vi
    nat = trainers["sample"]
    pre = nat.natural_gradient
    cores, idx, logq, _ = nat.draw(0)
    _, w = nat.sample_weights(idx, logq)
    w = w.contiguous()
    nat.loss_and_grad(0)                                       # the preconditioner's buffers
    T, u, delta = pre._T, torch.empty_like(pre._u), torch.empty_like(pre._delta)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    lq = torch.empty(B, dtype=torch.float64, device=dev)
    backend.mps_environments(cores, B)
    calls = {"sample_gram": lambda: backend.mps_score_sample_gram(cores, idx, out=T, status=st),
             "solve": lambda: backend.spd_solve(T, w, pre.damping, out=u, info=info),
             "second_vjp": lambda: backend.mps_score_vjp(cores, idx, u, out=delta, out_logq=lq, status=st)}
    for name, vi in trainers.items():
        if not isinstance(vi, str):
            calls["epoch_" + name] = (lambda v: lambda: v.loss_and_grad(0))(vi)
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, reps))
    D4 = (D + 3) // 4 * 4
    tiles = -(-B // 32)
    out = {"n": n, "D": D, "B": B, "P": 2 * n * D * D, "D4": D4, "tiles": tiles * (tiles + 1) // 2, "blocks": blocks, "reps": reps,
           "failed_solves": int((pre.info != 0).sum().item()),
           "vectors_bytes": 2 * n * (-(-B // 64) * 64) * D4 * 8,
           "sample_gram": summary(t["sample_gram"], B * B * n * 4 * D4 // 2,
                                  issued_flops=tiles * (tiles + 1) // 2 * n * 4 * 2 * (D4 // 4) * 2 * 16 * 16 * 4),
           "solve": summary(t["solve"], B ** 3 // 3, B * B * 8 * 2),
           "second_vjp": summary(t["second_vjp"])}
    for name, vi in trainers.items():
        out["epoch_" + name] = {"refused": vi} if isinstance(vi, str) else summary(t["epoch_" + name])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["16:4:1024", "40:4:1024", "63:8:1024", "63:16:1024", "63:32:1024"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sample_gram_time.py needs an MI355X")
    for s in args.sizes:
        n, D, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, B, args.blocks, args.reps, args.warmup)), flush=True)
        backend.release_workspaces()


if __name__ == "__main__":
    main()
