#!/usr/bin/env python3
"""The two-site sweep of the sampled MPS on the MI355X (GPU only: fails without one).

For (n, D, B) in {16, 63} x {4, 16} x {4096, 65536, 2^20}, in one process on one card, after warm-up, timed ALTERNATELY in
`blocks` blocks of `reps` calls each (device events around a block; medians over the blocks, with min and max):
  mps_twosite_sweep (bornvi_mps_twosite_sweep: one round trip, `steps` descent steps a bond; a chain of
    2 (n - 1) (2 steps + 3) small launches, the last advance of either pass left out, and 4 in front),
  one gradient epoch on the same cores and samples, mps_environments + mps_score_vjp: the yardstick, what train() pays per epoch,
and their ratio.  The sweep runs on canonical cores (mps_canonicalise once, outside the timing) with samples drawn from them,
lr = 0 so that every repetition does the same work on the same state.  No target ratio is set.
Prints one JSON line per shape; the record kept in the repository is

    python tools/mps_twosite_time.py > profiles/mps_twosite_time.jsonl

    python tools/mps_twosite_time.py [--sites 16 63] [--bonds 4 16] [--batches 4096 65536 1048576] [--steps 5] [--blocks 5] [--reps 3]
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


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def measure(n, D, B, steps, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    cores = ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()
    cores = backend.mps_canonicalise(cores)[0]
    backend.mps_environments(cores, B)
    idx = backend.mps_sample(cores, B, 1, torch.zeros(1, dtype=torch.int64, device=dev))[0]
    w = torch.full((B,), -1.0 / B, dtype=torch.float64, device=dev)
    grad = torch.empty_like(cores)
    work = cores.clone()

    def epoch():
        backend.mps_environments(cores, B)
        backend.mps_score_vjp(cores, idx, w, out=grad)

    calls = {"twosite_sweep": lambda: backend.mps_twosite_sweep(work, idx, None, 0.0, steps), "gradient_epoch": epoch}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    status = int(backend.mps_twosite_sweep(work, idx, None, 0.0, steps)[4].item())
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, reps))
    launches = 4 + 2 * (n - 1) * (2 * steps + 3) - 2
    out = {"n": n, "D": D, "B": B, "steps": steps, "blocks": blocks, "reps": reps, "status": status, "launches": launches}
    for k in calls:
        out[k] = summary(t[k])
    med = statistics.median(t["twosite_sweep"])
    out["us_per_launch"] = round(1e3 * med / launches, 3)
    out["sweep_over_epoch"] = round(med / statistics.median(t["gradient_epoch"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sites", type=int, nargs="*", default=[16, 63])
    ap.add_argument("--bonds", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--batches", type=int, nargs="*", default=[4096, 65536, 1 << 20])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mps_twosite_time.py needs an MI355X")
    for n in args.sites:
        for D in args.bonds:
            for B in args.batches:
                print(json.dumps(measure(n, D, B, args.steps, args.blocks, args.reps, args.warmup)), flush=True)
                backend.release_workspaces()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
