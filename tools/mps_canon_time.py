#!/usr/bin/env python3
"""The MPS canonicaliser on the MI355X (GPU only: fails without one).

For n in {16, 63} and each D, in one process on one card, after warm-up, timed ALTERNATELY in `blocks` blocks of `reps` calls
each (device events around a block; medians over the blocks, with min and max):
  mps_canonicalise (bornvi_mps_canonicalise: one workgroup, 2 (n - 1) Jacobi factorisations in sequence),
  mps_marginals without the pair marginals on the same cores: two sequential environment sweeps of the same depth, the
    yardstick for a latency-bound one-workgroup chain,
and their ratio; beside them the largest sweep count of the call's factorisations (the workspace's first word) and the
barriers the sweeps execute by construction: per factorisation sweeps x (rounds + 2), rounds = D - 1 (D for odd D).
Prints one JSON line per (n, D); the record kept in the repository is

    python tools/mps_canon_time.py > profiles/mps_canon_time.jsonl

    python tools/mps_canon_time.py [--sites 16 63] [--bonds 4 16 32] [--blocks 7] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
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


def measure(n, D, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    cores = ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()
    m1 = torch.empty(n, dtype=torch.float64, device=dev)
    calls = {"canonicalise": lambda: backend.mps_canonicalise(cores), "marginals": lambda: backend.mps_marginals(cores, out_m1=m1)}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    buf = backend._workspaces[backend._ws_key(dev, f"mps_canon_{n}_{D}")]
    sweeps = int(buf[(-buf.data_ptr()) % 256:][:4].cpu().numpy().view(np.int32)[0])
    status = int(backend.mps_canonicalise(cores)[5].item())
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, reps))
    rounds = D - 1 if D % 2 == 0 else D
    out = {"n": n, "D": D, "blocks": blocks, "reps": reps, "status": status, "max_sweeps": sweeps, "rounds_per_sweep": rounds,
           "factorisations": 2 * (n - 1), "sweep_barriers_upper": 2 * (n - 1) * sweeps * (rounds + 2)}
    for k in calls:
        out[k] = summary(t[k])
    out["canonicalise_over_marginals"] = round(statistics.median(t["canonicalise"]) / statistics.median(t["marginals"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sites", type=int, nargs="*", default=[16, 63])
    ap.add_argument("--bonds", type=int, nargs="*", default=[4, 16, 32])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mps_canon_time.py needs an MI355X")
    for n in args.sites:
        for D in args.bonds:
            print(json.dumps(measure(n, D, args.blocks, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
