#!/usr/bin/env python3
"""The sampled MPS path's three calls on the MI355X (GPU only: fails without one).

For each (n, D, B), in one process on one card, after warm-up: mps_environments, mps_sample and mps_score_vjp timed
ALTERNATELY in `blocks` blocks of `reps` calls each (device events around a block); medians over the blocks.  At n = 16 the
enumerated pair mps_probs + mps_vjp of the same cores is timed in the same alternation for comparison.  Beside each time:
the FLOPs and bytes of the call by construction (kernels_mps_sample.hip).  Prints one JSON line per size; the record kept
in the repository is

    python tools/mps_sampled_time.py > profiles/mps_sampled_time.jsonl

    python tools/mps_sampled_time.py [--sizes 16:4:4096 16:16:4096 40:4:4096 63:16:65536] [--blocks 10] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(v, flops=None, nbytes=None):
    out = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    if flops is not None:
        out["flops"] = int(flops)
        out["gflops"] = round(flops / (statistics.median(v) * 1e-3) / 1e9, 1)
    if nbytes is not None:
        out["bytes"] = int(nbytes)
    return out


def by_construction(n, D, B):
    """(FLOPs, bytes) of the three calls as the kernels are written, padded bond DP and row pitch DS included."""
    DP = 2 if D <= 2 else 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 32
    DS = (D + 1) & ~1
    tiles = -(-B // 64)
    G = min(tiles, 256)
    env = (2 * n * 2 * (2 * D ** 3 + 2 * D ** 3) * 1, 8 * (2 * n * 2 * D * D + 2 * (n + 1) * D * D))
    samp = (tiles * 64 * n * 2 * (4 * DP * DP + 4 * DP), tiles * n * 8 * (2 * D * D + D * D) + 16 * B)
    score_f = tiles * 64 * n * 2 * (2 * DP * DP) + tiles * n * 2 * 2 * 64 * (16 if DP <= 16 else 32) ** 2 + n * 2 * (4 * D ** 3)
    score_b = tiles * n * 2 * 8 * 2 * D * D + 2 * tiles * (n - 1) * 64 * (8 * DS + 4) + (2 * tiles - G) * n * 16 * D * D \
        + G * n * 16 * D * D + 24 * B
    return {"environments": env, "sample": samp, "score_vjp": (score_f, score_b)}


def measure(n, D, B, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    cores = ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    logq = torch.empty(B, dtype=torch.float64, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    grad = torch.empty_like(cores)
    w = torch.randn(B, dtype=torch.float64, device=dev) / B
    calls = {"environments": lambda: backend.mps_environments(cores, B),
             "sample": lambda: backend.mps_sample(cores, B, 1, ep, out_idx=idx, out_logq=logq, status=st),
             "score_vjp": lambda: backend.mps_score_vjp(cores, idx, w, out=grad, out_logq=logq, status=st)}
    if n <= 16:
        g = torch.randn(1 << n, dtype=torch.float64, device=dev)

        def pair():
            backend.mps_probs(cores)
            backend.mps_vjp(cores, g, out=grad)
        calls["enumerated_pair"] = pair
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, reps))
    con = by_construction(n, D, B)
    out = {"n": n, "D": D, "B": B, "parameters": cores.numel(), "blocks": blocks, "reps": reps, "status": int(st.item()),
           "workspace_bytes": int(backend._cached_size(backend._ext.handle_for(dev), "bornvi_mps_sample_workspace_bytes", n, D, B))}
    for k in calls:
        out[k] = summary(t[k], *con.get(k, (None, None)))
    out["sampled_epoch_ms"] = round(sum(statistics.median(t[k]) for k in ("environments", "sample", "score_vjp")), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["16:4:4096", "16:16:4096", "40:4:4096", "63:16:65536"])
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mps_sampled_time.py needs an MI355X")
    for s in args.sizes:
        n, D, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, B, args.blocks, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
