"""The launching entry points of include/bornvi_ttn.h held to the five assertions of tests/memory_contract.py: the case is built
by hand from mc.Buffer (the header lies outside the ROLES table of bornvi.h).  It is the sequence environments, sample, score_vjp
on one workspace of the size bornvi_ttn_workspace_bytes reports, at (n, D, B) = (5, 3, 130): cores, epoch_dev, idx and w are in;
log_Z_out and grad_cores (each may be NULL), the sampler's idx, logq and status and the score call's logq and status are out; the
workspace is never read before it is written (runs from 0x00, 0xFF and a larger call's leftovers give the same bytes), a NULL
grad_cores leaves logq as it was, and nothing is written beyond a buffer's size.  The donor is a larger shape with other values.
bornvi_ttn_workspace_bytes writes no device memory: its refusals, and those of the three above with canary buffers, are held in
test_gpu_ttn_kernel.py::test_refused_sizes_leave_everything_untouched."""
import numpy as np
import pytest
import torch

import memory_contract as mc
import ttn_mirror as tt
from tensornetworks_amd import _ext

pytestmark = pytest.mark.gpu

SHAPE, DONOR = (5, 3, 130), (9, 5, 300)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def build(shape, seed):
    n, D, B = shape
    rng = np.random.default_rng([seed, n, D, B])
    cores = tt.random_cores(n, D, 100 + seed)
    idx = rng.integers(0, 1 << n, B).astype(np.int64)
    w = rng.standard_normal(B)
    h = _ext.handle_for(dev())
    need = h.size("bornvi_ttn_workspace_bytes", n, D, B)
    bufs = [mc.Buffer("cores", "in", data=cores), mc.Buffer("epoch_dev", "in", data=np.array([3 + seed], np.int64)),
            mc.Buffer("idx_in", "in", data=idx), mc.Buffer("w", "in", data=w),
            mc.Buffer("log_Z_out", "out", nbytes=8, optional=True), mc.Buffer("idx", "out", nbytes=8 * B),
            mc.Buffer("logq_sampler", "out", nbytes=8 * B), mc.Buffer("status", "out", nbytes=4, align=4),
            mc.Buffer("logq", "out", nbytes=8 * B), mc.Buffer("grad_cores", "out", nbytes=8 * cores.size, optional=True),
            mc.Buffer("status_score", "out", nbytes=4, align=4), mc.Buffer("workspace", "workspace", nbytes=need, align=mc.WS_ALIGN)]

    def run(mem, addr):
        h.call("bornvi_ttn_environments", n, D, B, addr["cores"], addr["log_Z_out"], addr["workspace"], need, None)
        h.call("bornvi_ttn_sample", n, D, B, addr["cores"], 1234 + seed, addr["epoch_dev"], addr["idx"], addr["logq_sampler"], addr["status"],
               addr["workspace"], need, None)
        h.call("bornvi_ttn_score_vjp", n, D, B, addr["cores"], addr["idx_in"], addr["w"], addr["logq"], addr["grad_cores"],
               addr["status_score"], addr["workspace"], need, None)
    return mc.Case(bufs, run)


def test_memory_contract():
    case, donor = build(SHAPE, 0), build(DONOR, 1)
    out = mc.check_case(case, donor, dev())
    n, D, B = SHAPE
    assert int(out["status"].cpu().numpy().view(np.int32)[0]) == 0 and int(out["status_score"].cpu().numpy().view(np.int32)[0]) == 0
    logZ = out["log_Z_out"].cpu().numpy().view(np.float64)
    grad = out["grad_cores"].cpu().numpy().view(np.float64)
    logq = out["logq"].cpu().numpy().view(np.float64)
    lqs = out["logq_sampler"].cpu().numpy().view(np.float64)
    idx = out["idx"].cpu().numpy().view(np.int64)
    assert np.isfinite(logZ).all() and np.isfinite(grad).all() and np.isfinite(logq).all() and np.isfinite(lqs).all()
    assert grad.shape == (7 * D * D * D,) and np.all(idx >= 0) and np.all(idx < (1 << n))
