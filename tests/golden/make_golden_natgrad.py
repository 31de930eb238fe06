"""Records tests/golden/natgrad_sprinkler_trace.npz: the float64 / float32-theta mirror's natural-gradient ELBO run on the
Sprinkler network (tests/natgrad_mirror.py: hardware_efficient, n = 3, L = 4, damping 1e-3, SGD without momentum), which
the GPU trainer test compares train() with.

Learning rate 0.3 and 40 epochs were chosen on the CPU: the GPU test asserts a final KL below KL_THRESHOLD = 1e-6, and the
mirror alone must end KL_MARGIN = 100 times below that (1e-8).  It ends at 6.2e-13; plain SGD at the same rate and epoch
count ends at 3.0e-8 (recorded beside it as kl_sgd).  This script refuses to write a trace that misses the margin.
Run from the repository root:  python tests/golden/make_golden_natgrad.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import natgrad_mirror as nm  # noqa: E402

if __name__ == "__main__":
    h, th0 = nm.sprinkler_run()
    sgd, _ = nm.sprinkler_run(natural=False)
    assert h["kl"][-1] * nm.KL_MARGIN < nm.KL_THRESHOLD, h["kl"][-1]
    assert max(h["natgrad_info"]) == 0
    print(f"natural gradient: KL {h['kl'][0]:.4e} -> {h['kl'][-1]:.4e}, TVD {h['tvd'][-1]:.4e}; "
          f"plain SGD: KL {sgd['kl'][-1]:.4e}, TVD {sgd['tvd'][-1]:.4e}")
    np.savez(os.path.join(HERE, "natgrad_sprinkler_trace.npz"), theta0=th0, loss_elbo=np.array(h["loss_elbo"]),
             kl=np.array(h["kl"]), grad_norm=np.array(h["grad_norm"]), tvd=np.array(h["tvd"]),
             theta=np.array(h["theta"]), theta_final=h["theta"][-1], kl_sgd=np.array(sgd["kl"]), tvd_sgd=np.array(sgd["tvd"]))
