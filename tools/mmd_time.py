#!/usr/bin/env python3
"""The two MMD calls on the MI355X (GPU only: fails without one).  DESIGN.md section 6q.

mmd_weights at each n beside bornvi_elbo_weights in the same process on the same card, the two timed ALTERNATELY in `blocks`
blocks of `reps` calls each (device events around a block), medians over the blocks with their spread.  elbo_weights is the
yardstick: one pass over 2^n doubles (24 bytes an entry: q, log_p, w).  mmd_weights makes `passes` tile passes (bornvi_mmd_passes),
each a read and a write of 2^n doubles, the first one also reading the target: hbm_fraction = (passes * 16 * 2^n bytes) / time /
the HBM peak (8 TB/s), the bytes by construction, not by counter.  The loss-only call (want_w=False) is timed too.

hamming_pairs_rowsum at each (n, A, B): pairs / s = A B / time.  The kernel does no HBM traffic to speak of (8 (A + B) bytes in,
4 G (n + 1) A bytes of counts out); per pair it issues one LDS read, two xors, two popcounts, an address and one integer LDS add.

One JSON line per size; the record kept in the repository is

    python tools/mmd_time.py > profiles/mmd_time.jsonl

    python tools/mmd_time.py [--n 16 20 24] [--pairs 16:4096:4096 63:65536:65536 63:4096:1048576] [--blocks 10] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.hamming_kernel import HammingMixtureKernel            # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(v):
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def measure_weights(n, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(n)
    N = 1 << n
    q = torch.rand(N, dtype=torch.float64, device=dev)
    q /= q.sum()
    target = torch.bincount(torch.randint(0, N, (100000,), device=dev), minlength=N).double() / 100000
    log_p = torch.log(torch.rand(N, dtype=torch.float64, device=dev) + 1e-3)
    lam = HammingMixtureKernel(n).spectrum_on(dev)
    w = torch.empty(N, dtype=torch.float64, device=dev)
    calls = {"mmd_weights": lambda: backend.mmd_weights(q, target, lam, out=w),
             "mmd_loss_only": lambda: backend.mmd_weights(q, target, lam, want_w=False),
             "elbo_weights": lambda: backend.elbo_weights(q, log_p, out=w)}
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, reps))
    passes = backend.mmd_passes(n)
    out = {"call": "mmd_weights", "n": n, "passes": passes, "blocks": blocks, "reps": reps}
    for k in calls:
        out[k] = summary(t[k])
    med = {k: statistics.median(v) * 1e-3 for k, v in t.items()}
    out["mmd_weights"]["hbm_fraction"] = round(passes * 16 * N / med["mmd_weights"] / HBM_PEAK, 4)
    out["mmd_loss_only"]["hbm_fraction"] = round(((passes + 1) // 2 * 16 * N - 8 * N) / med["mmd_loss_only"] / HBM_PEAK, 4)
    out["elbo_weights"]["hbm_fraction"] = round(24 * N / med["elbo_weights"] / HBM_PEAK, 4)
    out["mmd_over_elbo"] = round(med["mmd_weights"] / med["elbo_weights"], 3)
    return out


def measure_pairs(n, A, B, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(n + A + B)
    top = 1 << min(n, 62)
    za, zb = torch.randint(0, top, (A,), device=dev), torch.randint(0, top, (B,), device=dev)
    kappa = HammingMixtureKernel(n).kappa_on(dev)
    fn = lambda: backend.hamming_pairs_rowsum(za, zb, kappa)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = [timed(fn, reps) for _ in range(blocks)]
    out = {"call": "hamming_pairs_rowsum", "n": n, "A": A, "B": B, "blocks": blocks, "reps": reps, **summary(t)}
    out["pairs_per_s"] = float(f"{A * B / (statistics.median(t) * 1e-3):.4g}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="*", default=[16, 20, 24])
    ap.add_argument("--pairs", nargs="*", default=["16:4096:4096", "63:65536:65536", "63:4096:1048576"])
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mmd_time.py needs an MI355X")
    for n in args.n:
        print(json.dumps(measure_weights(n, args.blocks, args.reps, args.warmup)), flush=True)
    for s in args.pairs:
        n, A, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure_pairs(n, A, B, args.blocks, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
