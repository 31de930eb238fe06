"""The entry points of include/bornvi_cmps.h held to the memory contract of tests/memory_contract.py: the cases are built by hand
from mc.Buffer (the header lies outside the ROLES table of bornvi.h).  One case is the begin / finish sequence environments,
sample, score_vjp on one workspace of the size bornvi_cmps_workspace_bytes reports: cores, epoch_dev, idx and w are in;
log_Z_out (or NULL), the sampler's idx, logq and status and the gradient's logq, grad_cores and status are out; the workspace is
never read before it is written (runs from 0x00, 0xFF and a larger call's leftovers give the same bytes) and nothing is written
beyond its reported size.  Shapes: one site and one sample; odd D with a partial second tile; D = 16 with several workgroups.
The donor of each is the next larger shape.  The fourth entry, bornvi_cmps_workspace_bytes, writes no device memory: its refusals,
and those of the three above with canary buffers, are held in test_gpu_cmps_kernel.py::test_refused_sizes_leave_everything_untouched."""
import numpy as np
import pytest
import torch

import memory_contract as mc
from tensornetworks_amd import _ext

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 65), (12, 16, 300)]
DONOR = {(1, 1, 1): (3, 5, 65), (3, 5, 65): (12, 16, 300), (12, 16, 300): (13, 16, 400)}


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def build(shape, seed):
    n, D, B = shape
    rng = np.random.default_rng([seed, n, D, B])
    cores = 0.3 * rng.standard_normal((n, 2, D, D, 2))
    cores[..., 0] += np.eye(D)
    cores /= np.sqrt(2.0)
    idx = rng.integers(0, 1 << n, B).astype(np.int64)
    w = rng.standard_normal(B)
    h = _ext.handle_for(dev())
    need = h.size("bornvi_cmps_workspace_bytes", n, D, B)
    bufs = [mc.Buffer("cores", "in", data=cores), mc.Buffer("epoch_dev", "in", data=np.array([3 + seed], np.int64)),
            mc.Buffer("idx_in", "in", data=idx), mc.Buffer("w", "in", data=w),
            mc.Buffer("log_Z_out", "out", nbytes=8, optional=True), mc.Buffer("idx", "out", nbytes=8 * B), mc.Buffer("logq", "out", nbytes=8 * B),
            mc.Buffer("status", "out", nbytes=4, align=4), mc.Buffer("logq_score", "out", nbytes=8 * B),
            mc.Buffer("grad_cores", "out", nbytes=8 * cores.size), mc.Buffer("status_score", "out", nbytes=4, align=4),
            mc.Buffer("workspace", "workspace", nbytes=need, align=mc.WS_ALIGN)]

    def run(mem, addr):
        h.call("bornvi_cmps_environments", n, D, B, addr["cores"], addr["log_Z_out"], addr["workspace"], need, None)
        h.call("bornvi_cmps_sample", n, D, B, addr["cores"], 1234 + seed, addr["epoch_dev"], addr["idx"], addr["logq"], addr["status"],
               addr["workspace"], need, None)
        h.call("bornvi_cmps_score_vjp", n, D, B, addr["cores"], addr["idx_in"], addr["w"], addr["logq_score"], addr["grad_cores"],
               addr["status_score"], addr["workspace"], need, None)
    return mc.Case(bufs, run)


@pytest.mark.parametrize("shape", SHAPES)
def test_memory_contract(shape):
    case, donor = build(shape, 0), build(DONOR[shape], 1)
    out = mc.check_case(case, donor, dev())
    n, D, B = shape
    assert int(out["status"].cpu().numpy().view(np.int32)[0]) == 0 and int(out["status_score"].cpu().numpy().view(np.int32)[0]) == 0
    logZ = out["log_Z_out"].cpu().numpy().view(np.float64)
    grad = out["grad_cores"].cpu().numpy().view(np.float64)
    idx = out["idx"].cpu().numpy().view(np.int64)
    assert np.isfinite(logZ).all() and np.isfinite(grad).all() and grad.shape == (n * 2 * D * D * 2,)
    assert np.all(idx >= 0) and np.all(idx < (1 << n))
