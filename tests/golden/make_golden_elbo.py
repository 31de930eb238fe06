"""Records tests/golden/elbo_sprinkler_trace.npz: the float64 mirror's 200-epoch ELBO run on the Sprinkler network
(tests/elbo_mirror.py; settings in tests/test_elbo_host.py), which the GPU trainer test compares train() with.
Run from the repository root:  python tests/golden/make_golden_elbo.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_elbo_host as t  # noqa: E402

if __name__ == "__main__":
    bn, lat, _, x = t.sprinkler()
    h, th0 = t.run(t.SPRINKLER, bn, lat, x)
    np.savez(os.path.join(HERE, "elbo_sprinkler_trace.npz"), theta0=th0, loss_elbo=np.array(h["loss_elbo"]),
             kl=np.array(h["kl"]), entropy=np.array(h["entropy"]), grad_norm=np.array(h["grad_norm"]),
             tvd=np.array(h["tvd"]), theta_final=h["theta"][-1])
