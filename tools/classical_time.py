#!/usr/bin/env python3
"""Table-mode epoch of the classical KSD trainer on the MI355X (GPU only: fails without one).

For each size n (synthetic_network(n, 0), softmax table, Adam + cosine schedule, entropy weight 0.01) prints one JSON
line with, from device events over >= 200 warmed epochs of the same process:
  epoch_ms        one epoch's device work as train() enqueues it (born_table_probs, the contraction, born_table_vjp,
                  clip_grad_norm_, Adam, scheduler), without the per-epoch host read-back
  probs_ms        born_table_probs alone (q32, q64 and the entropy)
  vjp_ms          born_table_vjp alone
  contraction_ms  the contraction alone (dense K_p up to n = 16, Kronecker mat-vec beyond)
and the shares probs_ms / epoch_ms, vjp_ms / epoch_ms.

    python tools/classical_time.py [--sizes 8 12 16 20] [--epochs 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.ksd_vi import KSDVariationalInference                 # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(n, epochs, warmup):
    torch.manual_seed(0)
    bn, lat, obs, x = synthetic_network(n, 0)
    vi = KSDVariationalInference(bn, lat, obs, {'use_logits': True, 'conditioning_dim': 0}, device="cuda:0")
    vi._stein._prepare_stein(x)
    opt, sched = vi.make_optimizer(0.01, epochs + warmup)
    params = list(vi.born_machine.parameters())

    def epoch():
        opt.zero_grad()
        _, _, _, grads = vi.loss_and_grads(None, 0.01)
        vi.apply_grads(grads)
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        opt.step()
        sched.step()

    for _ in range(warmup):
        epoch()
    epoch_ms = timed(epoch, epochs)
    w = vi.born_machine.params.detach().reshape(1, -1)
    q32, q64, H = backend.born_table_probs(w, 0)
    ksd2, y = vi._stein._stein_contract(q64[0])
    y2 = y.reshape(1, -1)
    loss = torch.empty(1, dtype=torch.float64, device=w.device)
    out = torch.empty_like(w)
    probs_ms = timed(lambda: backend.born_table_probs(w, 0), epochs)
    vjp_ms = timed(lambda: backend.born_table_vjp(w, q64, 0, y=y2, ksd2=ksd2, entropy_weight=0.01, out=out,
                                                  loss_out=loss), epochs)
    contraction_ms = timed(lambda: vi._stein._stein_contract(q64[0]), epochs)
    return {"n": n, "gram": "dense" if vi._stein._K is not None else "kron", "epochs": epochs,
            "epoch_ms": round(epoch_ms, 4), "probs_ms": round(probs_ms, 4), "vjp_ms": round(vjp_ms, 4),
            "contraction_ms": round(contraction_ms, 4), "probs_share": round(probs_ms / epoch_ms, 3),
            "vjp_share": round(vjp_ms / epoch_ms, 3), "over_contraction_ms": round(epoch_ms - contraction_ms, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 12, 16, 20])
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("classical_time.py needs an MI355X (torch.cuda.is_available() is False)")
    if args.epochs < 200:
        raise SystemExit("--epochs must be >= 200")
    for n in args.sizes:
        print(json.dumps(measure(n, args.epochs, args.warmup)), flush=True)
        backend.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
