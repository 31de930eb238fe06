#!/usr/bin/env python3
"""Two epochs of each classical trainer and family at n = 6 on the MI355X, for a kernel trace (GPU only):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/family_epochs_trace.py

KSD table, KSD MLP, KSD MPS, ELBO MPS and sampled ELBO on synthetic_network(6, 0), seeded.  The kernel names and call
counts of the statistics file are the launches an epoch makes; profiles/family_surface_kernel_stats_*.csv keep them from
before and after the families moved onto born_machine_base.py."""
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensornetworks_amd.bayesian_network import synthetic_network             # noqa: E402
from tensornetworks_amd.elbo_vi import ELBOVariationalInference               # noqa: E402
from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference  # noqa: E402
from tensornetworks_amd.ksd_vi import KSDVariationalInference                 # noqa: E402

RUNS = [(KSDVariationalInference, {'use_logits': True}), (KSDVariationalInference, {'conditioning_dim': 1}),
        (KSDVariationalInference, {'family': 'mps', 'bond_dim': 2}), (ELBOVariationalInference, {'family': 'mps', 'bond_dim': 2}),
        (SampledELBOVariationalInference, {'bond_dim': 2, 'num_samples': 64})]

if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("family_epochs_trace.py needs an MI355X")
    bn, lat, obs, x = synthetic_network(6, 0)
    for cls, cfg in RUNS:
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            hist = cls(bn, lat, obs, cfg, device="cuda:0").train(x, 2, 0.05, verbose=False)
        print(cls.__name__, cfg, [k for k in hist if 'loss' in k][0], hist[[k for k in hist if 'loss' in k][0]])
    torch.cuda.synchronize()
