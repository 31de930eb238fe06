#!/usr/bin/env python3
"""The quantum-natural-gradient step against the fused KSD step and the classical natural-gradient step of the quantum
trainer on the MI355X (GPU only: fails without one).

Per size (default n = 16, L = 6 and n = 20, L = 8; synthetic_network(n, 0), hardware_efficient) three trainers are built in
the same process on the same card, share one Stein side, and their device steps (ksd_and_grad) are timed in alternation
with device events: the fused step, the classical-Fisher natural-gradient step (stored rows), the quantum natural-gradient
step (fused route + P + 1 statevectors + metric + solve).  Reported per kind: the median of the block means with the
smallest and largest block.  Also: bornvi_paramshift_states alone and bornvi_qfi_gram alone (with its TFLOP/s, counting
the computed tiles: 2 x 128 x 128 x tiles x 2^(n+1) flop), on the step's own parameters.  --dump DIR writes the fused
step's loss, gradient and q as .npy files (compare two checkouts' dumps for bitwise equality).

    python tools/qng_time.py [--sizes 16:6 20:8] [--blocks 10] [--reps 10] [--warmup 5] [--dump DIR]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference         # noqa: E402


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


def measure(n, L, blocks, reps, warmup, dump):
    bn, lat, obs, x = synthetic_network(n, 0)
    vis = {}
    for name, kw in (("fused", {}), ("natgrad", {"natural_gradient": True}), ("qng", {"natural_gradient": "quantum"})):
        torch.manual_seed(0)
        vi = KSDVariationalInference(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, pytorch_device="cuda:0", **kw)
        if vis:                                   # one Stein side for the three (K_p is the largest buffer)
            for attr in ("_S", "_K", "_K_rows", "_K_pairs", "_K_sig", "_K_form", "_stein_key"):
                setattr(vi, attr, getattr(vis["fused"], attr))
        else:
            vi._prepare_stein(x)
        vis[name] = vi
    for _ in range(warmup):
        for vi in vis.values():
            vi.ksd_and_grad()
    torch.cuda.synchronize()
    if dump:
        import numpy as np
        os.makedirs(dump, exist_ok=True)
        for name, t in zip(("loss", "grad", "q"), vis["fused"].ksd_and_grad()):
            np.save(os.path.join(dump, f"fused_n{n}_L{L}_{name}.npy"), t.cpu().numpy())
    t = {k: [] for k in vis}
    for _ in range(blocks):
        for k, vi in vis.items():
            t[k].append(timed(vi.ksd_and_grad, reps))
    qng = vis["qng"]
    P = qng.born_machine.num_ansatz_params
    dev = torch.device("cuda", 0)
    theta64 = qng.born_machine.theta.detach().double().contiguous()
    states = backend.paramshift_states("hardware_efficient", n, L, theta64, 0, P)
    Q = backend.qfi_gram(states[1:], states[0])
    st = [timed(lambda: backend.paramshift_states("hardware_efficient", n, L, theta64, 0, P, out=states), reps) for _ in range(blocks)]
    gram = [timed(lambda: backend.qfi_gram(states[1:], states[0], out=Q), reps) for _ in range(blocks)]
    T = -(-(P + 2) // 128)
    flop = 2.0 * 128 * 128 * (T * (T + 1) // 2) * (2 << n)
    gm = statistics.median(gram)
    return {"n": n, "L": L, "P": P, "gram_form": qng._K_form, "blocks": blocks, "reps": reps,
            "fused_dot": bool(backend.paramshift_dot_supported("hardware_efficient", n, L, dev, P)),
            "fused_step": summary(t["fused"]), "natgrad_step": summary(t["natgrad"]), "qng_step": summary(t["qng"]),
            "paramshift_states": summary(st), "qfi_gram": summary(gram), "qfi_gram_tflops": round(flop / gm * 1e-9, 2),
            "qfi_rows_read_GBps": round(16.0 * (P + 1) * (1 << n) / gm * 1e-6, 1), "solve_info": int(qng._natgrad_info)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["16:6", "20:8"], help="n:L pairs")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dump", default=None, help="directory for the fused step's outputs (.npy)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qng_time.py needs an MI355X (torch.cuda.is_available() is False)")
    for s in args.sizes:
        n, L = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, L, args.blocks, args.reps, args.warmup, args.dump)), flush=True)
        backend.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
