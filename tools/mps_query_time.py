#!/usr/bin/env python3
"""The sampled MPS's exact queries on the MI355X (GPU only: fails without one).

For n = 63 and each D, in one process on one card, after warm-up, timed ALTERNATELY in `blocks` blocks of `reps` calls each
(device events around a block; medians over the blocks):
  mps_marginals without and with the pair marginals,
  mps_log_marginals at Q in {1, 1024, 65536} evidences with half the sites clamped (seeded random masks); beside each time
    the fp64 FLOPs of the call by construction (kernels_mps_query.hip: a free site's step is 4 D^3 fmas, a clamped one's
    2 D^3, and one workgroup more sweeps the empty mask),
  mps_sample_clamped at B = 65536 under one such evidence, beside mps_environments + mps_sample at the same shape, and
    their ratio.
Prints one JSON line per D; the record kept in the repository is

    python tools/mps_query_time.py > profiles/mps_query_time.jsonl

    python tools/mps_query_time.py [--n 63] [--bonds 4 16 32] [--queries 1 1024 65536] [--samples 65536] [--blocks 7] [--reps 10]
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


def summary(v, flops=None):
    out = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    if flops is not None:
        out["flops"] = int(flops)
        out["gflops"] = round(flops / (statistics.median(v) * 1e-3) / 1e9, 1)
    return out


def half_masks(n, Q, rng):
    """Q evidences with n // 2 clamped sites each: (mask, value) int64 arrays."""
    mask = np.zeros(Q, np.int64)
    value = np.zeros(Q, np.int64)
    for j in range(Q):
        sites = rng.choice(n, size=n // 2, replace=False)
        m = int(sum(1 << int(s) for s in sites))
        mask[j] = m
        value[j] = int(rng.integers(0, 1 << 62)) & m
    return mask, value


def measure(n, D, queries, B, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rng = np.random.default_rng([n, D])
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    cores = ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    logq = torch.empty(B, dtype=torch.float64, device=dev)
    logm = torch.empty(1, dtype=torch.float64, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    m1 = torch.empty(n, dtype=torch.float64, device=dev)
    m2 = torch.empty(n, n, dtype=torch.float64, device=dev)
    calls, flops, heavy = {}, {}, set()
    calls["marginals"] = lambda: backend.mps_marginals(cores, out_m1=m1)
    calls["marginals_pairs"] = lambda: backend.mps_marginals(cores, want_pairs=True, out_m1=m1, out_m2=m2)
    for Q in queries:
        mk, vl = half_masks(n, Q, rng)
        mask, value = torch.from_numpy(mk).to(dev), torch.from_numpy(vl).to(dev)
        out = torch.empty(Q, dtype=torch.float64, device=dev)
        key = f"log_marginals_Q{Q}"
        calls[key] = (lambda mask=mask, value=value, out=out: backend.mps_log_marginals(cores, mask, value, out=out, status=st))
        flops[key] = 2 * (Q * ((n - n // 2) * 4 + (n // 2) * 2) + n * 4) * D ** 3
        if flops[key] > 1e11:
            heavy.add(key)
    mk, vl = half_masks(n, 1, rng)
    smask, svalue = torch.from_numpy(mk).to(dev), torch.from_numpy(vl).to(dev)
    calls["sample_clamped"] = lambda: backend.mps_sample_clamped(cores, B, smask, svalue, 1, ep, out_idx=idx, out_logq=logq,
                                                                 out_logm=logm, status=st)

    def plain():
        backend.mps_environments(cores, B)
        backend.mps_sample(cores, B, 1, ep, out_idx=idx, out_logq=logq, status=st)
    calls["environments_plus_sample"] = plain
    for k, fn in calls.items():
        for _ in range(1 if k in heavy else warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, 1 if k in heavy else reps))
    out = {"n": n, "D": D, "B": B, "clamped_sites": n // 2, "blocks": blocks, "reps": reps, "reps_heavy": 1}
    for k in calls:
        out[k] = summary(t[k], flops.get(k))
    out["clamped_over_plain"] = round(statistics.median(t["sample_clamped"]) / statistics.median(t["environments_plus_sample"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=63)
    ap.add_argument("--bonds", type=int, nargs="*", default=[4, 16, 32])
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 1024, 65536])
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mps_query_time.py needs an MI355X")
    for D in args.bonds:
        print(json.dumps(measure(args.n, D, args.queries, args.samples, args.blocks, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
