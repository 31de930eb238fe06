"""bornvi_mps_twosite_sweep held to the memory contract of tests/memory_contract.py: the cases are built by hand from mc.Buffer
(the entry point is declared in include/bornvi_twosite.h, outside the ROLES table of bornvi.h): cores is inout, idx and w are
in, the five outputs are out, and the workspace is never read before it is written (runs from 0x00, 0xFF and a larger call's
leftovers give the same bytes).  Shapes: one bond touching both boundaries; odd D with a partial second tile; the full
32 x 32 factorisation with a full MFMA tile.  The donor of each is the next larger shape."""
import ctypes as C

import numpy as np
import pytest
import torch

import memory_contract as mc
import mps_twosite_mirror as tm
from tensornetworks_amd import _ext

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 1), (3, 3, 65), (12, 16, 1000)]
DONOR = {(2, 1, 1): (3, 3, 65), (3, 3, 65): (12, 16, 1000), (12, 16, 1000): (13, 16, 1100)}


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def build(shape, seed):
    n, D, B = shape
    rng = np.random.default_rng([seed, n, D, B])
    cores = tm.canonical((np.eye(D) + 0.3 * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0))
    idx = rng.integers(0, 1 << n, B).astype(np.int64)
    w = rng.uniform(0.5, 1.5, B)
    w = w / w.sum()
    h = _ext.handle_for(dev())
    need = h.size("bornvi_mps_twosite_workspace_bytes", n, D, B)
    bufs = [mc.Buffer("cores", "inout", data=cores), mc.Buffer("idx", "in", data=idx), mc.Buffer("w", "in", data=w),
            mc.Buffer("loss", "out", nbytes=8 * 2 * (n - 1)), mc.Buffer("schmidt", "out", nbytes=8 * (n - 1) * D),
            mc.Buffer("discarded", "out", nbytes=8 * (n - 1)), mc.Buffer("rank", "out", nbytes=4 * (n - 1), align=4),
            mc.Buffer("status", "out", nbytes=4, align=4), mc.Buffer("workspace", "workspace", nbytes=need, align=mc.WS_ALIGN)]

    def run(mem, addr):
        h.call("bornvi_mps_twosite_sweep", n, D, B, addr["cores"], addr["idx"], addr["w"], C.c_double(0.03), 2, D, C.c_double(1e-6),
               addr["loss"], addr["schmidt"], addr["discarded"], addr["rank"], addr["status"], addr["workspace"], need, None)
    return mc.Case(bufs, run)


@pytest.mark.parametrize("shape", SHAPES)
def test_memory_contract(shape):
    case, donor = build(shape, 0), build(DONOR[shape], 1)
    out = mc.check_case(case, donor, dev())
    n = shape[0]
    status = int(out["status"].cpu().numpy().view(np.int32)[0])
    loss = out["loss"].cpu().numpy().view(np.float64)
    assert status & ~2 == 0 and loss.shape == (2 * (n - 1),) and np.all(np.isfinite(loss))      # uniform samples may meet psi = 0
