"""Records tests/golden/qng_sprinkler_trace.npz: the float64 / float32-theta mirror's quantum-natural-gradient ELBO run on
the Sprinkler network (tests/qng_mirror.py), with the settings of the natural-gradient golden run
(natgrad_mirror.SPRINKLER_*: hardware_efficient, n = 3, L = 4, damping 1e-3, SGD without momentum, lr 0.3, 40 epochs) and
the quantum Fisher information in place of the classical Fisher matrix.  The GPU trainer test compares its run with it.
Run from the repository root:  python tests/golden/make_golden_qng.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import qng_mirror as qm  # noqa: E402

if __name__ == "__main__":
    h, th0 = qm.sprinkler_run()
    assert max(h["natgrad_info"]) == 0
    print(f"quantum natural gradient: KL {h['kl'][0]:.4e} -> {h['kl'][-1]:.4e}, TVD {h['tvd'][-1]:.4e}")
    np.savez(os.path.join(HERE, "qng_sprinkler_trace.npz"), theta0=th0, loss_elbo=np.array(h["loss_elbo"]),
             kl=np.array(h["kl"]), grad_norm=np.array(h["grad_norm"]), tvd=np.array(h["tvd"]),
             theta=np.array(h["theta"]), theta_final=h["theta"][-1])
