#!/usr/bin/env python3
"""The tree tensor network's three calls beside the real family's on the MI355X (GPU only: fails without one).

For each (n, D, B), in one process on one card, after warm-up: ttn_environments, ttn_sample and ttn_score_vjp (with the gradient,
and as `logq_only` without it) at bond D, and mps_environments / mps_sample / mps_score_vjp at bond D, all timed ALTERNATELY in
`blocks` blocks of `reps` calls each (device events around a block); medians over the blocks with their spread.  No time is fixed
in advance: the yardsticks are the real family's calls at the same (n, D, B) in the same run, and the ratios are printed.  For the
score call the achieved fraction of the fp64 matrix-core peak is printed too: per tile of 64 samples and node the sample term
issues 16 v_mfma_f64_16x16x4_f64 for each tile of 16 child pairs (max(1, DP^2 / 16) of them, DP = D padded to 2, 4, 8),
2 . 16 . 16 . 4 flops each whatever D is, against --peak-tflops (the MI355X's fp64 matrix peak, 78.6; tools/lps_time.py's); the
time it is divided by is the whole call's, sweeps included.  One JSON line per size; the record kept in the repository is

    python tools/ttn_time.py > profiles/ttn_time.jsonl

    python tools/ttn_time.py [--sizes 16:4:4096 63:4:65536 63:8:65536] [--blocks 10] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.born_machine_ttn_sampled import TreeSampledBornMachine   # noqa: E402

CALLS = ("environments", "sample", "score_vjp")
MFMA_FLOPS = 2 * 16 * 16 * 4


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


def buffers(cores, B, dev):
    return (torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev),
            torch.empty(B, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev), torch.empty_like(cores),
            torch.randn(B, dtype=torch.float64, device=dev) / B)


def real_calls(cores, B, dev):
    ep, idx, logq, st, grad, w = buffers(cores, B, dev)
    return {"environments": lambda: backend.mps_environments(cores, B),
            "sample": lambda: backend.mps_sample(cores, B, 1, ep, out_idx=idx, out_logq=logq, status=st),
            "score_vjp": lambda: backend.mps_score_vjp(cores, idx, w, out=grad, out_logq=logq, status=st)}, st


def tree_calls(cores, n, B, dev):
    ep, idx, logq, st, grad, w = buffers(cores, B, dev)
    return {"environments": lambda: backend.ttn_environments(cores, n, B),
            "sample": lambda: backend.ttn_sample(cores, n, B, 1, ep, out_idx=idx, out_logq=logq, status=st),
            "score_vjp": lambda: backend.ttn_score_vjp(cores, n, idx, w, out=grad, out_logq=logq, status=st),
            "logq_only": lambda: backend.ttn_score_vjp(cores, n, idx, out=False, out_logq=logq, status=st)}, st


def measure(n, D, B, blocks, reps, warmup, peak_tflops):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    re = ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()
    tr = TreeSampledBornMachine(n, bond_dim=D).cores.detach().to(dev).contiguous()
    groups = {"tree": tree_calls(tr, n, B, dev), "real": real_calls(re, B, dev)}
    names = {g: tuple(fns) for g, (fns, _) in groups.items()}
    for _ in range(warmup):
        for g, (fns, _) in groups.items():          # a family's calls in order: sample and score_vjp read its environments
            for k in names[g]:
                fns[k]()
    torch.cuda.synchronize()
    t = {(g, k): [] for g in groups for k in names[g]}
    for _ in range(blocks):
        for k in CALLS + ("logq_only",):
            for g, (fns, _) in groups.items():
                if k in fns:
                    t[(g, k)].append(timed(fns[k], reps))
    med = {key: statistics.median(v) for key, v in t.items()}
    out = {"n": n, "D": D, "B": B, "blocks": blocks, "reps": reps, "status": {g: int(st.item()) for g, (_, st) in groups.items()}}
    for g in groups:
        out[g] = {k: summary(t[(g, k)]) for k in names[g]}
        out[g]["epoch_ms"] = round(sum(med[(g, k)] for k in CALLS), 4)
    out["tree_over_real"] = {k: round(med[("tree", k)] / med[("real", k)], 3) for k in CALLS}
    _, L = backend.ttn_tree_shape(n)
    DP = 2 if D <= 2 else 4 if D <= 4 else 8
    flops = MFMA_FLOPS * 16.0 * max(1, DP * DP // 16) * (L - 1) * ((B + 63) // 64)
    out["score_vjp_matrix_tflops"] = round(flops / (med[("tree", "score_vjp")] * 1e-3) / 1e12, 4)
    out["score_vjp_fraction_of_fp64_matrix_peak"] = round(out["score_vjp_matrix_tflops"] / peak_tflops, 5)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["16:4:4096", "63:4:65536", "63:8:65536"])
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ttn_time.py needs an MI355X")
    for s in args.sizes:
        n, D, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, B, args.blocks, args.reps, args.warmup, args.peak_tflops)), flush=True)


if __name__ == "__main__":
    main()
