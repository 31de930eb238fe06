#!/usr/bin/env python3
"""Host time of one quantum-trainer step with every kernel call stubbed out (no GPU needed): what the Python between
"theta" and "loss, gradient, q" costs on each route, for A/B runs of host-side changes at the latency-bound sizes, where an
eager step is a few tens of microseconds of launches and this code is the rest.

    python tools/quantum_host_step_time.py [--other DIR] [--n 8] [--layers 4] [--reps 150] [--blocks 300]

--other: a second checkout (another commit) whose tensornetworks_amd is loaded into the same process under another name
and timed in blocks ALTERNATING with this one: separate processes differ by more than the microsecond that matters here.
The stubs return preallocated CPU tensors of the right shapes; the trainers' own work -- the default theta64, the deal,
spans, hooks, finisher choice, preconditioner checks -- runs as in a real step.  Prints one JSON line: per kind and route
[10th percentile, median] microseconds per step over the blocks, for each checkout."""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

import torch


def load(name, root):
    """The package tensornetworks_amd of the checkout `root`, imported under `name`."""
    path = os.path.join(os.path.abspath(root), "tensornetworks_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    sys.modules[name] = module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return name


def stubbed_trainers(pkg, n, L):
    """(KSD trainer, ELBO trainer, [fused route on/off]) of package `pkg` with the backend's step calls stubbed."""
    backend = importlib.import_module(pkg + ".backend")
    N, P, f64 = 1 << n, backend.num_params("hardware_efficient", n, L), torch.float64
    probs, w, one, g = torch.zeros(2 * P + 1, N, dtype=f64), torch.zeros(N, dtype=f64), torch.ones(1, dtype=f64), torch.zeros(P, dtype=f64)
    state, fused = torch.zeros(N, dtype=torch.complex128), [False]
    backend.paramshift_probs = lambda *a, **k: probs
    backend.paramshift_dot_supported = lambda *a, **k: fused[0]
    backend.paramshift_dot_begin = lambda *a, **k: (probs[0], ("token",))
    backend.paramshift_dot_finish = lambda token, w, ksd2=None: (one if ksd2 is not None else None, g)
    backend.ksd_grad_finish = lambda *a, **k: (one, g, w)
    backend.shifted_dot = lambda *a, **k: g
    backend.adjoint_state = lambda *a, **k: (state, probs[0])
    backend.adjoint_vjp = lambda *a, **k: g
    bn, lat, obs, _ = importlib.import_module(pkg + ".bayesian_network").synthetic_network(n, 0)
    kw = dict(qbm_num_latent_vars=n, qbm_ansatz_layers=L)
    ksd = importlib.import_module(pkg + ".ksd_vi_quantum").KSDVariationalInference(bn, lat, obs, **kw)
    ksd._S, ksd._stein_contract = torch.zeros(N, n, dtype=f64), (lambda q: (one, w))
    elbo = importlib.import_module(pkg + ".elbo_vi_quantum").ELBOVariationalInference(bn, lat, obs, **kw)
    elbo.objective.log_p, elbo.objective.weights = torch.zeros(N, dtype=f64), (lambda q: (one, one, w))
    return ksd, elbo, fused


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other", default=None)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=150)
    ap.add_argument("--blocks", type=int, default=300)
    args = ap.parse_args()
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sides = {"here": stubbed_trainers(load("tn_here", here), args.n, args.layers)}
    if args.other:
        sides["other"] = stubbed_trainers(load("tn_other", args.other), args.n, args.layers)

    def block(fn):
        a = time.perf_counter()
        for _ in range(args.reps):
            fn()
        return (time.perf_counter() - a) / args.reps * 1e6

    out = {"tool": "quantum_host_step_time", "n": args.n, "L": args.layers, "reps": args.reps, "blocks": args.blocks,
           "unit": "us per step, kernels stubbed: [10th percentile, median] of the alternating blocks"}
    for route in ("stored", "fused", "adjoint"):
        for i, kind in enumerate(("ksd", "elbo")):
            fns = {}
            for side, trainers in sides.items():
                trainers[2][0] = route == "fused"
                trainers[i].grad_engine = "adjoint" if route == "adjoint" else "paramshift"
                fns[side] = trainers[i].ksd_and_grad if kind == "ksd" else trainers[i].elbo_and_grad
                block(fns[side])
            t = {side: [] for side in fns}
            for _ in range(args.blocks):
                for side, fn in fns.items():
                    t[side].append(block(fn))
            out[f"{kind}_{route}"] = {side: [round(sorted(v)[len(v) // 10], 2), round(statistics.median(v), 2)] for side, v in t.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
