#!/usr/bin/env python3
"""One eager step per gradient route and kind of the quantum trainers on the MI355X, for a kernel trace (GPU only):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/quantum_routes_trace.py

KSD and ELBO on synthetic_network(n, 2), seeded: stored rows at n = 3 (plain, classical Fisher, quantum Fisher), adjoint at
n = 3, fused dot at n = 14 (plain, quantum Fisher; KSD matrix-free there), then two KSD steps with 64 shots.  The kernel
names and call counts of the statistics file are the launches the steps make; profiles/quantum_routes_kernel_stats_*.csv
keep them from before and after the routes moved to quantum_trainer.py.  A new route or kind gets a row in RUNS."""
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd import backend                                        # noqa: E402
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi_quantum import ELBOVariationalInference       # noqa: E402
from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference         # noqa: E402

# (n, layers, route, natural_gradient)
RUNS = [(3, 2, "stored", None), (3, 2, "stored", True), (3, 2, "stored", "quantum"), (3, 2, "adjoint", None),
        (14, 1, "fused", None), (14, 1, "fused", "quantum")]


def make(kind, n, L, **kw):
    bn, lat, obs, x = synthetic_network(n, 2)
    if kind == "ksd":
        kw["gram_mode"] = "auto" if n < 14 else "kron"
    torch.manual_seed(7)
    with contextlib.redirect_stdout(sys.stderr):
        vi = (KSDVariationalInference if kind == "ksd" else ELBOVariationalInference)(
            bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, pytorch_device="cuda:0", **kw)
        vi._prepare_observation(x)
    return vi, (vi.ksd_and_grad if kind == "ksd" else vi.elbo_and_grad)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("quantum_routes_trace.py needs an MI355X")
    dev = torch.device("cuda", 0)
    for kind in ("ksd", "elbo"):
        for n, L, route, ng in RUNS:
            vi, step = make(kind, n, L, natural_gradient=ng)
            P = vi.born_machine.num_ansatz_params
            assert backend.paramshift_dot_supported("hardware_efficient", n, L, dev, P) == (route == "fused"), (n, L, route)
            vi.grad_engine = "adjoint" if route == "adjoint" else "paramshift"
            step()
            torch.cuda.synchronize()
            print(kind, n, route, ng, "ok")
    vi, step = make("ksd", 3, 2, qbm_shots=64, shot_seed=5)
    step(), step()
    torch.cuda.synchronize()
    print("ksd shots ok")
