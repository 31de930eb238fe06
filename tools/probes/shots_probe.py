"""Finite-shot sampler and shots-mode step on the MI355X.

1. bornvi_shots_histogram alone: B = 577 rows at n = 16 and B = 961 rows at n = 20 (the 1 + 2P rows of a step at L = 6 / 8,
   the circuits' own probabilities at the bench's theta), S in {10^3, 10^4, 10^6}: device time per call and the rate of its
   3 B 2^n 8 bytes (two reads of the rows, one write of the frequencies) against the 8 TB/s HBM peak.
2. One training step (training_step_async: circuits, sampling, contraction, finish, optimiser) in shots mode
   (S = 10^4) against the exact mode's fused and un-fused steps, in the same process on the same K_p: n = 16, L = 6, dense.
3. The same at n = 8, L = 4 as a graph replay (make_graphed_step).
Prints one JSON object at the end; `--json PATH` also writes it to PATH.

    python tools/probes/shots_probe.py [--json PATH]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

import bench  # noqa: E402
from tensornetworks_amd import backend  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--json", default=None, help="also write the result object to this file")
args = ap.parse_args()
HBM_PEAK = 8.0e12
dev = torch.device("cuda:0")
out = {"sampler": [], "step": {}}


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def shots_on(vi, S):
    bm = vi.born_machine
    bm.shots, bm.shot_seed, bm.dev.shots = S, 1234, S


def shots_off(vi):
    bm = vi.born_machine
    bm.shots, bm.dev.shots = None, None


# ---- 1. the sampler alone ------------------------------------------------------------------------------
for workload in ("n16_L6_kron", "n20_L8_kron"):
    n, L, ansatz, _ = bench.WORKLOADS[workload]
    g = torch.Generator().manual_seed(0)
    P = backend.num_params(ansatz, n, L)
    theta = (0.1 * torch.randn(P, generator=g, dtype=torch.float64)).to(dev)
    rows = backend.paramshift_probs(ansatz, n, L, theta, 0, P, include_base=True)
    B = rows.shape[0]
    freq = torch.empty_like(rows)
    epoch = torch.zeros(1, dtype=torch.int64, device=dev)
    nbytes = 3 * B * (1 << n) * 8
    for S in (10 ** 3, 10 ** 4, 10 ** 6):
        ms = device_ms(lambda: backend.shots_histogram(rows, n, S, 7, epoch, out=freq), 5 if S < 10 ** 6 else 3)
        out["sampler"].append({"n": n, "B": B, "shots": S, "ms": round(ms, 4), "bytes": nbytes,
                               "GBps": round(nbytes / ms / 1e6, 1), "frac_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)})
        print(json.dumps(out["sampler"][-1]), flush=True)
    del rows, freq
    torch.cuda.empty_cache()

# ---- 2. eager step at n = 16, L = 6 (dense K_p) ------------------------------------------------------------
vi, x = bench.make_vi("n16_L6_dense", dev, overlap=0)
vi._prepare_stein(x)
opt = vi.make_optimizer(0.005, 10 ** 6, True, "adam", (0.9, 0.999))


def step():
    vi.training_step_async(*opt, 10.0)


res = {}
for mode in ("exact_fused", "exact_unfused", "shots_1e4", "exact_fused_again"):
    vi.fused_dot = mode != "exact_unfused"
    if mode.startswith("shots"):
        shots_on(vi, 10 ** 4)
    else:
        shots_off(vi)
    res[mode] = round(device_ms(step, 10), 4)
    print(mode, res[mode], "ms", flush=True)
shots_off(vi)
vi.fused_dot = True
vi.timers = {}
shots_on(vi, 10 ** 4)
for _ in range(3):
    vi.ksd_and_grad()
torch.cuda.synchronize(dev)
res["shots_1e4_parts_ms"] = {k: round(sum(a.elapsed_time(b) for a, b in v[1:]) / max(1, len(v) - 1), 4)
                             for k, v in vi.timers.items()}
vi.timers = None
shots_off(vi)
res["ratio_shots_to_exact_fused"] = round(res["shots_1e4"] / min(res["exact_fused"], res["exact_fused_again"]), 3)
res["ratio_shots_to_exact_unfused"] = round(res["shots_1e4"] / res["exact_unfused"], 3)
out["step"]["n16_L6_dense"] = res
print(json.dumps(res), flush=True)
del vi, opt
torch.cuda.empty_cache()

# ---- 3. graph replay at n = 8, L = 4 -----------------------------------------------------------------------
res = {}
for mode in ("exact", "shots_1e4"):
    vi, x = bench.make_vi("n8_L4_dense", dev, overlap=0)
    if mode != "exact":
        shots_on(vi, 10 ** 4)
    vi._prepare_stein(x)
    st = vi.make_graphed_step(*vi.make_optimizer(0.005, 10 ** 6, True, "adam", (0.9, 0.999), capturable=True), 10.0, warmup=3)
    for _ in range(50):
        st()
    ms = device_ms(st, 500)
    res[mode + "_replay_us"] = round(ms * 1e3, 2)
    print(mode, res[mode + "_replay_us"], "us per replay", flush=True)
res["ratio"] = round(res["shots_1e4_replay_us"] / res["exact_replay_us"], 3)
out["step"]["n8_L4_graph"] = res
print(json.dumps(out))
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
