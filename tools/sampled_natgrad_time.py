#!/usr/bin/env python3
"""The sampled natural gradient's three calls and the whole epoch on the MI355X (GPU only: fails without one).

For each (n, D, B), in one process on one card, after warm-up: mps_score_rows, score_fisher_gram, spd_solve_batched (the
site blocks, one chunk of as many sites as the preconditioner's rows budget holds) and the device part of an ELBO epoch
(SampledELBOVariationalInference.loss_and_grad) with and without the preconditioner, timed ALTERNATELY in `blocks` blocks
of `reps` calls each (device events around a block); medians over the blocks with minima and maxima.  Beside each time:
bytes and FLOPs by construction -- the rows written once (8 R ld per site), 2 R^2 ld issued per Gram block (the padded
tiles issue more: `issued_flops`), P^3 / 3 per Cholesky.  Prints one JSON line per size; the record kept in the repository:

    python tools/sampled_natgrad_time.py > profiles/sampled_natgrad_time.jsonl

    python tools/sampled_natgrad_time.py [--sizes 16:4:4096 40:4:4096 63:8:16384 63:16:16384] [--blocks 5] [--reps 5] [--warmup 2]
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
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference  # noqa: E402
from tensornetworks_amd.natural_gradient import SampledFisherPreconditioner   # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(v, flops=None, nbytes=None, **more):
    med = statistics.median(v)
    out = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    if flops is not None:
        out["flops"] = int(flops)
        out["gflops"] = round(flops / (med * 1e-3) / 1e9, 1)
    if nbytes is not None:
        out["bytes"] = int(nbytes)
        out["gbytes_per_s"] = round(nbytes / (med * 1e-3) / 1e9, 1)
    out.update(more)
    return out


def measure(n, D, B, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    bn, lat, obs, x = synthetic_network(n, 0)
    torch.manual_seed(0)
    plain = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 1}, device='cuda:0')
    torch.manual_seed(0)
    nat = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 1}, device='cuda:0',
                                          natural_gradient=SampledFisherPreconditioner())
    for vi in (plain, nat):
        vi._prepare_observation(x)
    pre = nat.natural_gradient
    R, _, chunk = pre.plan(n, D, B)
    ld = backend.score_rows_ld(B)
    cores, idx, logq, _ = nat.draw(0)
    nat.loss_and_grad(0)                                       # the preconditioner's buffers; its chunk is the one timed below
    chunk = pre._rows.shape[0]
    rows, F = pre._rows, pre._F
    g = torch.randn(chunk, R, dtype=torch.float64, device=dev)
    xs = torch.empty_like(g)
    info = torch.empty(chunk, dtype=torch.int32, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    backend.mps_environments(cores, B)
    calls = {"score_rows": lambda: backend.mps_score_rows(cores, idx, 0, chunk, out=rows, status=st),
             "fisher_gram": lambda: backend.score_fisher_gram(rows, B, out=F),
             "solve_batched": lambda: backend.spd_solve_batched(F, g, pre.damping, out=xs, info=info),
             "epoch_plain": lambda: plain.loss_and_grad(0),
             "epoch_natgrad": lambda: nat.loss_and_grad(0)}
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, reps))
    tiles = -(-R // 64)
    out = {"n": n, "D": D, "B": B, "ld": ld, "R": R, "sites_per_chunk": chunk, "chunks_per_epoch": -(-n // chunk),
           "blocks": blocks, "reps": reps, "failed_solves": int((pre.info != 0).sum().item()), "rows_bytes": chunk * R * ld * 8,
           "score_rows": summary(t["score_rows"], None, chunk * R * ld * 8),
           "fisher_gram": summary(t["fisher_gram"], 2 * R * R * ld * chunk, chunk * R * ld * 8,
                                  issued_flops=2 * 64 * 64 * ld * chunk * tiles * (tiles + 1) // 2),
           "solve_batched": summary(t["solve_batched"], chunk * R ** 3 // 3, chunk * R * R * 8 * 2),
           "epoch_plain": summary(t["epoch_plain"]), "epoch_natgrad": summary(t["epoch_natgrad"])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["16:4:4096", "40:4:4096", "63:8:16384", "63:16:16384"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sampled_natgrad_time.py needs an MI355X")
    for s in args.sizes:
        n, D, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, B, args.blocks, args.reps, args.warmup)), flush=True)
        backend.release_workspaces()


if __name__ == "__main__":
    main()
