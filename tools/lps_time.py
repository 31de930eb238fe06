#!/usr/bin/env python3
"""The locally purified sampled MPS's three calls beside the real and the complex family's on the MI355X (GPU only: fails
without one).

For each (n, D, B), in one process on one card, after warm-up: lps_environments, lps_sample and lps_score_vjp (with the
gradient, and as `logq_only` without it) at bond D and purification m, mps_environments / mps_sample / mps_score_vjp at bond D and
cmps_environments / cmps_sample / cmps_score_vjp at bond D, all timed ALTERNATELY in `blocks` blocks of `reps` calls each (device
events around a block); medians over the blocks with their spread.  No time is fixed in advance: the yardsticks are the sibling
calls at the same D in the same run, and the ratios are printed.  For the score call the achieved fraction of the fp64
matrix-core peak is printed too: the kernel issues 24 v_mfma_f64_16x16x4_f64 per (sample, mu, site) (8 for the right sweep, 16
for the left sweep with the gradient), 2 . 16 . 16 . 4 flops each whatever D is, against --peak-tflops (the MI355X's fp64 matrix
peak, 78.6).  One JSON line per size; the record kept in the repository is

    python tools/lps_time.py > profiles/lps_time.jsonl

    python tools/lps_time.py [--sizes 16:4:4096 63:4:65536 63:16:65536] [--m 2] [--blocks 10] [--reps 5] [--warmup 2]
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
MFMA_FLOPS = 2 * 16 * 16 * 4
MFMAS_PER_SAMPLE_MU_SITE = 24


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


def sibling_calls(prefix, cores, B, dev):
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


def purified_calls(cores, B, dev):
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    logq = torch.empty(B, dtype=torch.float64, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    grad = torch.empty_like(cores)
    w = torch.randn(B, dtype=torch.float64, device=dev) / B
    return {"environments": lambda: backend.lps_environments(cores, B),
            "sample": lambda: backend.lps_sample(cores, B, 1, ep, out_idx=idx, status=st),
            "score_vjp": lambda: backend.lps_score_vjp(cores, idx, w, out=grad, out_logq=logq, status=st),
            "logq_only": lambda: backend.lps_score_vjp(cores, idx, out=False, out_logq=logq, status=st)}, st


def real_cores(n, D, dev):
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    return ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()


def measure(n, D, B, m, blocks, reps, warmup, peak_tflops):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    re = real_cores(n, D, dev)
    cx = torch.stack((re, 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64, device=dev) / 2.0 ** 0.5), dim=-1).contiguous()
    rest = 0.1 * torch.randn(n, 2, m - 1, D, D, dtype=torch.float64, device=dev) / 2.0 ** 0.5
    pu = torch.cat((re.unsqueeze(2), rest), dim=2).contiguous()
    groups = {"purified": purified_calls(pu, B, dev), "real": sibling_calls("mps", re, B, dev), "complex": sibling_calls("cmps", cx, B, dev)}
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
    out = {"n": n, "D": D, "m": m, "B": B, "blocks": blocks, "reps": reps, "status": {g: int(st.item()) for g, (_, st) in groups.items()}}
    for g in groups:
        out[g] = {k: summary(t[(g, k)]) for k in names[g]}
        out[g]["epoch_ms"] = round(sum(med[(g, k)] for k in CALLS), 4)
    out["purified_over_real"] = {k: round(med[("purified", k)] / med[("real", k)], 3) for k in CALLS}
    out["purified_over_complex"] = {k: round(med[("purified", k)] / med[("complex", k)], 3) for k in CALLS}
    flops = MFMAS_PER_SAMPLE_MU_SITE * MFMA_FLOPS * float(B) * m * n
    out["score_vjp_matrix_tflops"] = round(flops / (med[("purified", "score_vjp")] * 1e-3) / 1e12, 4)
    out["score_vjp_fraction_of_fp64_matrix_peak"] = round(out["score_vjp_matrix_tflops"] / peak_tflops, 5)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["16:4:4096", "63:4:65536", "63:16:65536"])
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lps_time.py needs an MI355X")
    for s in args.sizes:
        n, D, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, B, args.m, args.blocks, args.reps, args.warmup, args.peak_tflops)), flush=True)


if __name__ == "__main__":
    main()
