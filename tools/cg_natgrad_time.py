#!/usr/bin/env python3
"""The matrix-free CG natural gradient's three calls and the whole epoch on the MI355X (GPU only: fails without one).

For each (n, D, B), in one process on one card, after warm-up: mps_score_jvp, mps_score_vjp, cg_step (the
steps of a real recurrence, each between its own pair of events with the product F p outside them;
`timed_steps_not_frozen` says that every timed step did the whole update), and the device part of an ELBO epoch
(SampledELBOVariationalInference.loss_and_grad) with the plain gradient, with natural_gradient='sample' (where B <= 1024:
else "refused") and with natural_gradient='cg' at its defaults, timed ALTERNATELY in `blocks` blocks of `reps` calls each
(device events around a block); medians over the blocks with minima and maxima -- the method of
tools/sampled_natgrad_time.py.  `cg_iters` is the number of iterations the 'cg' epoch's solve took before it froze (of
max_iters launched), `relres` where it stopped.  Prints one JSON line per size; the record kept in the repository:

    python tools/cg_natgrad_time.py > profiles/cg_natgrad_time.jsonl

    python tools/cg_natgrad_time.py [--sizes 16:4:1024 40:4:1024 63:8:1024 63:16:1024 63:32:1024 63:16:65536 63:32:4096]
                                    [--blocks 5] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sampled_natgrad_time import summary, timed                               # noqa: E402
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference  # noqa: E402


def measure(n, D, B, blocks, reps, warmup):
    dev = torch.device("cuda:0")
    bn, lat, obs, x = synthetic_network(n, 0)
    trainers = {}
    for name, spec in (("plain", None), ("sample", "sample"), ("cg", "cg")):
        torch.manual_seed(0)
        try:
            vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 1}, device='cuda:0',
                                                 natural_gradient=spec)
        except ValueError as e:
            trainers[name] = str(e)
            continue
        vi._prepare_observation(x)
        trainers[name] = vi
    nat = trainers["cg"]
    pre = nat.natural_gradient
    cores, idx, logq, _ = nat.draw(0)
    nat.loss_and_grad(0)                                       # the preconditioner's buffers
    iters, relres, info = int(pre.iters.item()), float(pre.relres.item()), int(pre.info.item())
    v = torch.randn(tuple(cores.shape), dtype=torch.float64, device=dev)
    t = torch.empty(B, dtype=torch.float64, device=dev)
    Fp = torch.empty_like(v)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    lq = torch.empty(B, dtype=torch.float64, device=dev)
    backend.mps_environments(cores, B)
    backend.mps_score_jvp(cores, idx, v, 1.0 / B, out=t, status=st)
    backend.mps_score_vjp(cores, idx, t, out=Fp, out_logq=lq, status=st)
    xs, r, p, state, _ = backend.cg_init(v)
    calls = {"jvp": lambda: backend.mps_score_jvp(cores, idx, v, 1.0 / B, out=t, status=st),
             "vjp": lambda: backend.mps_score_vjp(cores, idx, t, out=Fp, out_logq=lq, status=st),
             "cg_step": None}
    for name, vi in trainers.items():
        if not isinstance(vi, str):
            calls["epoch_" + name] = (lambda tr: lambda: tr.loss_and_grad(0))(vi)

    def timed_steps(count):
        """`count` steps of a real recurrence (g = v, the preconditioner's damping, rel_tol 0): the product F p runs between
        the steps, outside the pairs of events; -> (ms per step, whether every step did the whole update)."""
        backend.cg_init(v, xs, r, p, state)
        pairs = []
        for _ in range(count):
            backend.mps_score_jvp(cores, idx, p, 1.0 / B, out=t, status=st)
            backend.mps_score_vjp(cores, idx, t, out=Fp, out_logq=lq, status=st)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            backend.cg_step(Fp, xs, r, p, state, pre.damping, 0.0)
            b.record()
            pairs.append((a, b))
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in pairs) / count, int(state[2].item()) == count and float(state[3].item()) == 0.0

    for _ in range(warmup):
        for k, fn in calls.items():
            timed_steps(1) if fn is None else fn()
    torch.cuda.synchronize()
    tm = {k: [] for k in calls}
    live = True
    for _ in range(blocks):
        for k, fn in calls.items():
            if fn is None:
                ms, ok = timed_steps(reps)
                tm[k].append(ms)
                live = live and ok
            else:
                tm[k].append(timed(fn, reps))
    out = {"n": n, "D": D, "B": B, "P": 2 * n * D * D, "blocks": blocks, "reps": reps, "max_iters": pre.max_iters,
           "rel_tol": pre.rel_tol, "damping": pre.damping, "cg_iters": iters, "relres": relres, "info": info,
           "timed_steps_not_frozen": live,
           "jvp": summary(tm["jvp"]), "vjp": summary(tm["vjp"]), "cg_step": summary(tm["cg_step"], nbytes=2 * n * D * D * 8 * 10)}
    for name, vi in trainers.items():
        out["epoch_" + name] = {"refused": vi} if isinstance(vi, str) else summary(tm["epoch_" + name])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="*", default=["16:4:1024", "40:4:1024", "63:8:1024", "63:16:1024", "63:32:1024", "63:16:65536",
                                                   "63:32:4096"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cg_natgrad_time.py needs an MI355X")
    for s in args.sizes:
        n, D, B = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, B, args.blocks, args.reps, args.warmup)), flush=True)
        backend.release_workspaces()


if __name__ == "__main__":
    main()
