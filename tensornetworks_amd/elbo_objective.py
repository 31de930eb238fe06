"""The ELBO side of training, independent of the variational family: the log-joint table log p(x, z) of one observation
over all 2^n latent states, the evidence, and the step's device piece (loss, entropy, dL/dq from q).  Both ELBO trainers
hold one `ElboObjective`, as both KSD trainers share `stein_operator.SteinOperator`.

  L(theta) = sum_z q_theta(z) [log q_theta(z) - log p(x, z)] = KL(q_theta || p(.|x)) - log p(x)

is exact here: every engine holds q_theta for all 2^n states, and the score kernel returns p(x, z) for all of them.
Conventions: log q is log max(q, q_floor) and passes no gradient below the floor; log p is
log max(p, p_floor), finite also where the network gives a state probability zero (deterministic CPTs); a term with
q_z == 0 is exactly 0."""
import math

import torch

from . import backend
from .bayesian_network import pack_network


class ElboObjective:
    def __init__(self, bn, latent_vars_names, device, p_floor=1e-30, q_floor=1e-10):
        """Touches neither the GPU nor the library."""
        if len(latent_vars_names) < 1:
            raise ValueError("the ELBO needs at least one latent variable")
        for name, v in (("p_floor", p_floor), ("q_floor", q_floor)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
                raise ValueError(f"{name} must be a positive finite number, got {v!r}")
        self.bn = bn
        self.latent_vars_names = list(latent_vars_names)
        self.num_latent_vars = len(self.latent_vars_names)
        self.p_floor = float(p_floor)
        self.q_floor = float(q_floor)
        self._device = device
        self.log_p = None            # log max(p(x, z), p_floor) [2^n] float64 on the GPU: the table weights() reads
        self.log_evidence = None     # log p(x) = log sum_z p(x, z), a Python float
        self._key_prepared = None

    @staticmethod
    def _key(x_dict):
        return tuple(sorted((x_dict or {}).items()))

    @staticmethod
    def log_table(pxz, p_floor):
        """log max(p(x, z), p_floor) of a float64 tensor of joint probabilities (any device)."""
        return torch.log(pxz.clamp(min=p_floor))

    def prepare(self, x_dict):
        """The table and the evidence, once per observation (a second call with the same observation keeps them)."""
        key = self._key(x_dict)
        if self.log_p is not None and self._key_prepared == key:
            return
        dev = backend.compute_device(self._device)
        packed = pack_network(self.bn, self.latent_vars_names, x_dict)
        _, pxz = backend.score_from_packed(packed, self.num_latent_vars, dev)
        evidence = float(pxz.sum())
        if not evidence > 0.0:
            raise ValueError(f"the observation {dict(x_dict or {})} has probability {evidence} under the network")
        self.log_p = self.log_table(pxz, self.p_floor)
        self.log_evidence = math.log(evidence)
        self._key_prepared = key

    def weights(self, q, want_w=True, out=None):
        """q float64 [2^n] or [rows, 2^n] on the GPU -> (neg_elbo [rows], entropy [rows], w = d neg_elbo / d q like q)."""
        if self.log_p is None:
            raise ValueError("ElboObjective.weights before prepare(x_dict)")
        return backend.elbo_weights(q, self.log_p, self.q_floor, want_w=want_w, want_entropy=True, out=out)
