#!/usr/bin/env python3
"""Amortised inference with the sampled MPS on the MI355X (GPU only: fails without one).

In one process on one card, after warm-up, timed ALTERNATELY in `blocks` blocks of `reps` calls each (device events around a
block; medians over the blocks), one JSON line per record:
  bn_sample            at V = 41 (synthetic_network(40), every node kept) and V = 64 (a 64-node chain, the first node drawn and
                       dropped: n = 63), B = 2^10 ... 2^20;
  log_marginals_vjp    beside log_marginals at n = 63, D in {4, 16, 32}, Q in {1, 1024, 65536}, evidences with half the sites
                       clamped (the shapes of tools/mps_query_time.py), seeded random weights;
  epoch                AmortisedMPSInference.loss_and_grad of each objective on the 41-site chain, D = 4, B = 4096.
The record kept in the repository is

    python tools/amortised_time.py > profiles/amortised_time.jsonl

    python tools/amortised_time.py [--bonds 4 16 32] [--queries 1 1024 65536] [--blocks 5] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mps_query_time import half_masks, timed                                                     # noqa: E402
from tensornetworks_amd import backend                                                           # noqa: E402
from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference                        # noqa: E402
from tensornetworks_amd.bayesian_network import BayesianNetwork, pack_network_for_sampling, synthetic_network   # noqa: E402


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def alternate(calls, heavy, blocks, reps, warmup):
    for k, fn in calls.items():
        for _ in range(1 if k in heavy else warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            t[k].append(timed(fn, 1 if k in heavy else reps))
    return {k: summary(v) for k, v in t.items()}


def chain64():
    rng = np.random.default_rng(64)
    bn = BayesianNetwork()
    bn.add_node('N0', cpt={(): {0: 0.5, 1: 0.5}})
    for v in range(1, 64):
        p = rng.uniform(0.1, 0.9, 2)
        bn.add_node(f'N{v}', cpt={(0,): {0: 1 - p[0], 1: p[0]}, (1,): {0: 1 - p[1], 1: p[1]}}, parent_names=[f'N{v - 1}'])
    return bn, [f'N{v}' for v in range(1, 64)]


def measure_bn_sample(blocks, reps, warmup):
    dev = torch.device("cuda:0")
    syn, zs, xs, _ = synthetic_network(40)
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    for bn, sites in ((syn, zs + xs), chain64()):
        n = len(sites)
        keep, desc = backend.bn_descriptor(pack_network_for_sampling(bn, sites), dev)
        calls = {}
        for lg in range(10, 21):
            B = 1 << lg
            idx = torch.empty(B, dtype=torch.int64, device=dev)
            logp = torch.empty(B, dtype=torch.float64, device=dev)
            calls[f"B{B}"] = (lambda B=B, idx=idx, logp=logp: backend.bn_sample(desc, n, B, 1, ep, out_idx=idx, out_logp=logp, status=st))
        out = {"what": "bn_sample", "V": len(bn.nodes), "n": n, "blocks": blocks, "reps": reps}
        out.update(alternate(calls, set(), blocks, reps, warmup))
        print(json.dumps(out), flush=True)


def measure_vjp(n, D, queries, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rng = np.random.default_rng([n, D])
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    cores = ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()
    st = torch.empty(1, dtype=torch.int32, device=dev)
    grad = torch.empty_like(cores)
    calls, heavy = {}, set()
    for Q in queries:
        mk, vl = half_masks(n, Q, rng)
        mask, value = torch.from_numpy(mk).to(dev), torch.from_numpy(vl).to(dev)
        c = torch.from_numpy(rng.standard_normal(Q)).to(dev)
        out = torch.empty(Q, dtype=torch.float64, device=dev)
        calls[f"log_marginals_Q{Q}"] = (lambda mask=mask, value=value, out=out:
                                        backend.mps_log_marginals(cores, mask, value, out=out, status=st))
        calls[f"log_marginals_vjp_Q{Q}"] = (lambda mask=mask, value=value, c=c, out=out:
                                            backend.mps_log_marginals_vjp(cores, mask, value, c, out=grad, out_logm=out, status=st))
        if Q * n * D ** 3 > 1e9:
            heavy |= {f"log_marginals_Q{Q}", f"log_marginals_vjp_Q{Q}"}
    out = {"what": "log_marginals_vjp", "n": n, "D": D, "clamped_sites": n // 2, "groups_at_Q65536": backend.mps_log_marginals_vjp_groups(65536),
           "blocks": blocks, "reps": reps, "reps_heavy": 1}
    out.update(alternate(calls, heavy, blocks, reps, warmup))
    print(json.dumps(out), flush=True)


def measure_epoch(blocks, reps, warmup):
    syn, zs, xs, _ = synthetic_network(40)
    torch.manual_seed(0)
    vi = AmortisedMPSInference(syn, zs, xs, {'bond_dim': 4, 'num_samples': 4096, 'seed': 0}, device='cuda:0')
    calls = {obj: (lambda obj=obj: vi.loss_and_grad(0, obj)) for obj in vi.OBJECTIVES}
    out = {"what": "epoch", "sites": vi.num_sites, "D": 4, "B": 4096, "observed_sites": 1, "blocks": blocks, "reps": reps}
    out.update(alternate(calls, set(), blocks, reps, warmup))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=63)
    ap.add_argument("--bonds", type=int, nargs="*", default=[4, 16, 32])
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 1024, 65536])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/amortised_time.py needs an MI355X")
    measure_bn_sample(args.blocks, args.reps, args.warmup)
    for D in args.bonds:
        measure_vjp(args.n, D, args.queries, args.blocks, args.reps, args.warmup)
    measure_epoch(args.blocks, args.reps, args.warmup)


if __name__ == "__main__":
    main()
