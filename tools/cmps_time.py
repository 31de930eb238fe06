#!/usr/bin/env python3
"""The complex sampled MPS's three calls beside the real family's on the MI355X (GPU only: fails without one).

For each (n, D, B), in one process on one card, after warm-up: cmps_environments, cmps_sample and cmps_score_vjp at bond D, and
mps_environments, mps_sample and mps_score_vjp at bond D and at bond 2 D (capped at 32), all timed ALTERNATELY in `blocks`
blocks of `reps` calls each (device events around a block); medians over the blocks with their spread.  The yardstick of a
complex call is the real call at bond 2 D on the same card in the same run: a complex matrix-vector product at D has the 4 D^2
real multiplies of a real one at 2 D, half the matrix bytes and two right vectors' worth of slice traffic.  No ratio is fixed in
advance; the ratios are printed.  One JSON line per size; the record kept in the repository is

    python tools/cmps_time.py > profiles/cmps_time.jsonl

    python tools/cmps_time.py [--sizes 16:4:4096 63:4:65536 63:16:65536 63:16:1048576] [--blocks 10] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402

CALLS = ("environments", "sample", "score_vjp")


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


def family_calls(prefix, cores, B, dev):
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    logq = torch.empty(B, dtype=torch.float64, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    grad = torch.empty_like(cores)
    w = torch.randn(B, dtype=torch.float64, device=dev) / B
    env, samp, score = (getattr(backend, f"{prefix}_{k}") for k in CALLS)
    return {"environments": lambda: env(cores, B),
            "sample": lambda: samp(cores, B, 1, ep, out_idx=idx, out_logq=logq, status=st),
            "score_vjp": lambda: score(cores, idx, w, out=grad, out_logq=logq, status=st)}, st


def real_cores(n, D, dev):
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    return ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()


def measure(n, D, B, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    D2 = min(2 * D, backend.MPS_MAX_BOND)
    re = real_cores(n, D, dev)
    cx = torch.stack((re, 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64, device=dev) / 2.0 ** 0.5), dim=-1).contiguous()
    groups = {"complex": family_calls("cmps", cx, B, dev), "real": family_calls("mps", re, B, dev),
              "real_2D": family_calls("mps", real_cores(n, D2, dev), B, dev)}
    calls = {(g, k): fn for g, (fns, _) in groups.items() for k, fn in fns.items()}
    for _ in range(warmup):
        for g, (fns, _) in groups.items():          # a family's three calls in order: sample and score_vjp read its environments
            for k in CALLS:
                fns[k]()
    torch.cuda.synchronize()
    t = {key: [] for key in calls}
    for _ in range(blocks):
        for k in CALLS:
            for g in groups:
                t[(g, k)].append(timed(calls[(g, k)], reps))
    out = {"n": n, "D": D, "B": B, "real_2D_bond": D2, "blocks": blocks, "reps": reps,
           "status": {g: int(st.item()) for g, (_, st) in groups.items()}}
    for g in groups:
        out[g] = {k: summary(t[(g, k)]) for k in CALLS}
        out[g]["epoch_ms"] = round(sum(statistics.median(t[(g, k)]) for k in CALLS), 4)
    out["complex_over_real_2D"] = {k: round(statistics.median(t[("complex", k)]) / statistics.median(t[("real_2D", k)]), 3) for k in CALLS}
    out["complex_over_real"] = {k: round(statistics.median(t[("complex", k)]) / statistics.median(t[("real", k)]), 3) for k in CALLS}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["16:4:4096", "63:4:65536", "63:16:65536", "63:16:1048576"])
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cmps_time.py needs an MI355X")
    for s in args.sizes:
        n, D, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, B, args.blocks, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
