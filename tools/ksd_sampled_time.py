#!/usr/bin/env python3
"""The sampled KSD epoch's device calls on the MI355X (GPU only: fails without one).

For each (n, D, B), in one process on one card, after warm-up: bn_score_samples and stein_pairs_rowsum timed beside
mps_environments, mps_sample and mps_score_vjp, ALTERNATELY in `blocks` blocks of `reps` calls each (device events around a
block); medians over the blocks.  At n = 16, B = 4096 bornvi_stein_kp_pairs, the only other per-pair evaluator, runs over
the same B^2 pairs in the same alternation as the yardstick (it reads 2 B^2 (n + 1) doubles that the row-sum kernel never
forms).  Beside each time: the FLOPs and bytes of the call by construction (kernels_ksd_sampled.hip), and for the row sums
the fraction of the fp64 matrix peak (78.6 TFLOP/s), once counting the MFMAs issued (inner dimension padded to 4 KS, edge
tiles whole) and once counting the useful 2 * 3 n B^2.  Prints one JSON line per size; the record kept in the repository is

    python tools/ksd_sampled_time.py > profiles/ksd_sampled_time.jsonl

    python tools/ksd_sampled_time.py [--sizes 16:4:4096 40:4:4096 63:16:16384 63:16:65536] [--blocks 10] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network, pack_network   # noqa: E402
from mps_sampled_time import timed, summary                                   # noqa: E402

FP64_MFMA_PEAK = 78.6e12


def by_construction(n, B, k_mean):
    """(FLOPs, bytes) of the two calls as the kernels are written."""
    KS = 12 if n <= 16 else 24 if n <= 32 else 36 if n <= 48 else 48
    rb, tiles = -(-B // 64), -(-B // 32)
    per, G = backend.stein_pairs_geometry(B)
    issued = rb * 64 * tiles * 32 * 4 * KS * 2                      # MFMA flops, padding and edge tiles included
    epilogue = rb * 64 * tiles * 32 * 5                             # three additions, one product, one row-sum addition
    # a workgroup reads its 64 rows once and every tile of its range; partials once out and once in
    pair_bytes = rb * G * 64 * (8 * n + 16) + rb * tiles * 32 * (8 * n + 16) + 2 * G * B * 8 + B * (8 * n + 8) + 2 * B * 8
    # per sample: n scores of k_mean factor pairs (a quotient, a product) and a subtraction; the logs are not asked for
    score = (B * n * k_mean * 2 + B * n, B * 8 + B * n * 8)
    return {"bn_score_samples": score, "stein_pairs_rowsum": (issued + epilogue, pair_bytes)}, issued, 2 * 3 * n * B * B


def measure(n, D, B, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    cores = ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()
    bn, lat, obs, x = synthetic_network(n, 0)
    packed = pack_network(bn, lat, x)
    keep, desc = backend.bn_descriptor(packed, dev)
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    logq = torch.empty(B, dtype=torch.float64, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    grad = torch.empty_like(cores)
    w = torch.randn(B, dtype=torch.float64, device=dev) / B
    S = torch.empty(B, n, dtype=torch.float64, device=dev)
    r = torch.empty(B, dtype=torch.float64, device=dev)
    T = torch.empty(1, dtype=torch.float64, device=dev)
    calls = {"environments": lambda: backend.mps_environments(cores, B),
             "sample": lambda: backend.mps_sample(cores, B, 1, ep, out_idx=idx, out_logq=logq, status=st),
             "bn_score_samples": lambda: backend.bn_score_samples(desc, n, idx, out=S),
             "stein_pairs_rowsum": lambda: backend.stein_pairs_rowsum(idx, S, n, 1.0, out=r, total=T),
             "score_vjp": lambda: backend.mps_score_vjp(cores, idx, w, out=grad, out_logq=logq, status=st)}
    yardstick = n <= 16 and B <= 4096
    if yardstick:
        for fn in list(calls.values())[:3]:
            fn()
        zi, zj = idx.repeat_interleave(B), idx.repeat(B)
        si, sj = S.repeat_interleave(B, dim=0).contiguous(), S.repeat(B, 1).contiguous()
        calls["stein_kp_pairs"] = lambda: backend.stein_kp_pairs(n, 1.0, zi, zj, si, sj)
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, reps))
    npar = packed["n_parents"]
    k_mean = 1.0 + float(npar.sum()) / n             # a node's own factor and its children's: every parent link once
    con, issued, useful = by_construction(n, B, k_mean)
    per, G = backend.stein_pairs_geometry(B)
    out = {"n": n, "D": D, "B": B, "pairs": B * B, "blocks": blocks, "reps": reps, "status": int(st.item()),
           "tiles_per_range": per, "column_ranges": G,
           "workspace_bytes": int(backend._cached_size(backend._ext.handle_for(dev), "bornvi_stein_pairs_workspace_bytes", n, B))}
    for k in calls:
        out[k] = summary(t[k], *con.get(k, (None, None)))
    med = statistics.median(t["stein_pairs_rowsum"]) * 1e-3
    out["stein_pairs_rowsum"]["mfma_flops_issued"] = int(issued)
    out["stein_pairs_rowsum"]["frac_of_fp64_mfma_peak_issued"] = round(issued / med / FP64_MFMA_PEAK, 4)
    out["stein_pairs_rowsum"]["frac_of_fp64_mfma_peak_useful"] = round(useful / med / FP64_MFMA_PEAK, 4)
    out["stein_pairs_rowsum"]["ns_per_pair"] = round(med * 1e9 / (B * B), 5)
    if yardstick:
        out["kp_pairs_over_rowsum"] = round(statistics.median(t["stein_kp_pairs"]) / statistics.median(t["stein_pairs_rowsum"]), 2)
    out["sampled_ksd_epoch_ms"] = round(sum(statistics.median(t[k]) for k in
                                            ("environments", "sample", "bn_score_samples", "stein_pairs_rowsum", "score_vjp")), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["16:4:4096", "40:4:4096", "63:16:16384", "63:16:65536"])
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ksd_sampled_time.py needs an MI355X")
    for s in args.sizes:
        n, D, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, B, args.blocks, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
