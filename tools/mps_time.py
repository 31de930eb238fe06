#!/usr/bin/env python3
"""The MPS Born machine's two calls against the table family's on the MI355X (GPU only: fails without one).

For each (n, D), in one process on one card, timed ALTERNATELY in `blocks` blocks of `reps` calls per side (device events
around a block, after warm-up):
  (a) mps_probs + mps_vjp on cores [n, 2, D, D] (small_random initialisation, seeded),
  (b) born_table_probs + born_table_vjp (y given, ksd2 = None) on a table of 2^n logits,
each with the bytes its kernels move by construction and the resulting fraction of the HBM peak (8 TB/s), and the device
part of a whole epoch (loss_and_grads) of the ELBO and the KSD trainer with either family on synthetic_network(n, 0).
Prints one JSON line per (n, D) to stdout; the record kept in the repository is

    python tools/mps_time.py > profiles/mps_time.jsonl

    python tools/mps_time.py [--sizes 16:4 16:16 20:4 20:16] [--blocks 10] [--reps 20] [--warmup 5] [--no-epochs]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi import ELBOVariationalInference               # noqa: E402
from tensornetworks_amd.ksd_vi import KSDVariationalInference                 # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(v, nbytes=None):
    out = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    if nbytes is not None:
        out["bytes"] = int(nbytes)
        out["hbm_fraction"] = round(nbytes / (statistics.median(v) * 1e-3) / HBM_PEAK, 4)
    return out


def mps_bytes(n, D):
    """Bytes the MPS kernels ask for by construction (kernels_mps.hip): levels of [2^k, DS] doubles, DS = D rounded up to even.
    The backward sweep walks a workgroup's block of G_k twice (rows, then the core gradient): both reads are counted, though
    the second can come from a cache while the block is small."""
    N, row = 1 << n, 8 * ((D + 1) & ~1)
    fwd = sum(((1 << (k - 1)) + (1 << k)) * row for k in range(1, n)) + (N // 2) * row + 8 * N      # the levels, then psi
    fwd += 8 * N + 8 * N + 4 * N                                                                   # psi -> q64, q32
    bwd = 16 * N                                                                                   # c = sum q g: psi, g
    bwd += 16 * N + (N // 2) * row                                                                 # top, rows: psi, g -> G_{n-1}
    bwd += 16 * N + (N // 2) * row                                                                 # top, dA_n: psi, g again, V_{n-1}
    bwd += sum(((1 << k) + (1 << (k - 1))) * row for k in range(1, n))                             # rows: G_k -> G_{k-1}
    bwd += sum(((1 << k) + (1 << (k - 1))) * row for k in range(1, n))                             # dA_k: G_k again, V_{k-1}
    return fwd + bwd


def table_bytes(n):
    """The table pair: w read twice (row statistics, then q32 + q64 written), the VJP's statistics pass over q64 and y,
    its second pass over w, q64 and y, the float32 gradient written."""
    N = 1 << n
    return (4 + 4 + 4 + 8) * N + (8 + 8) * N + (4 + 8 + 8 + 4) * N


def measure(n, D, blocks, reps, warmup, epochs):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    cores = ((eye + 0.1 * torch.randn(n, 2, D, D, dtype=torch.float64)) / 2.0 ** 0.5).to(dev).contiguous()
    g = torch.randn(1 << n, dtype=torch.float64).to(dev)
    w = (0.1 * torch.randn(1, 1 << n)).to(dev)
    y = g.reshape(1, -1).contiguous()
    grad = torch.empty_like(cores)

    def mps_pair():
        backend.mps_probs(cores)
        backend.mps_vjp(cores, g, out=grad)

    def table_pair():
        _, q64, _ = backend.born_table_probs(w, 0, want_entropy=False)
        backend.born_table_vjp(w, q64, 0, y=y)

    for _ in range(warmup):
        mps_pair()
        table_pair()
    torch.cuda.synchronize()
    t = {"mps": [], "table": [], "mps_probs": [], "mps_vjp": []}
    for _ in range(blocks):
        t["mps"].append(timed(mps_pair, reps))
        t["table"].append(timed(table_pair, reps))
    for _ in range(3):
        t["mps_probs"].append(timed(lambda: backend.mps_probs(cores), reps))
        backend.mps_probs(cores)
        t["mps_vjp"].append(timed(lambda: backend.mps_vjp(cores, g, out=grad), reps))
    out = {"n": n, "D": D, "parameters": cores.numel(), "blocks": blocks, "reps": reps,
           "mps_pair": summary(t["mps"], mps_bytes(n, D)), "table_pair": summary(t["table"], table_bytes(n)),
           "mps_probs": summary(t["mps_probs"]), "mps_vjp": summary(t["mps_vjp"]),
           "bytes_ratio": round(mps_bytes(n, D) / table_bytes(n), 3),
           "time_ratio": round(statistics.median(t["mps"]) / statistics.median(t["table"]), 3)}
    if epochs:
        bn, lat, obs, x = synthetic_network(n, 0)
        for name, cls in (("elbo", ELBOVariationalInference), ("ksd", KSDVariationalInference)):
            sides = {}
            for fam, cfg in (("mps", {'family': 'mps', 'bond_dim': D}), ("table", {'use_logits': True})):
                torch.manual_seed(0)
                with contextlib.redirect_stdout(sys.stderr):       # the trainers' progress lines stay out of the JSON
                    vi = cls(bn, lat, obs, cfg, device="cuda:0")
                    vi._prepare_observation(x)
                lam = 0.0 if name == "elbo" else 0.01
                sides[fam] = lambda vi=vi, lam=lam: vi.loss_and_grads(None, lam)
            for _ in range(warmup):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            te = {"mps": [], "table": []}
            for _ in range(max(3, blocks // 2)):
                for fam, fn in sides.items():
                    te[fam].append(timed(fn, max(2, reps // 2)))
            out[name + "_epoch"] = {fam: summary(v) for fam, v in te.items()}
            del sides, vi
            backend.release_workspaces()
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["16:4", "16:16", "20:4", "20:16"], help="n:D pairs")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-epochs", action="store_true", help="leave out the trainers' epochs (the KSD side builds K_p)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mps_time.py needs an MI355X (torch.cuda.is_available() is False)")
    for s in args.sizes:
        n, D = (int(v) for v in s.split(":"))
        print(json.dumps(measure(n, D, args.blocks, args.reps, args.warmup, not args.no_epochs)), flush=True)
        backend.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
