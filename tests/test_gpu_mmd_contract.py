"""The entry points of include/bornvi_mmd.h held to the memory contract of tests/memory_contract.py: the cases are built by hand
from mc.Buffer (the header lies outside the ROLES table of bornvi.h).

bornvi_mmd_weights: q, target and lam are in, loss and w (or NULL) are out, at the smallest one-pass, two-group (three passes) and
three-group (five passes) n of the library's own geometry.  q, target and w carry the 16-byte alignment the header states.
bornvi_hamming_pairs_rowsum: za, zb and kappa are in, r, total and counts (or NULL) are out, at (n, A, B) = (1, 1, 1),
(33, 65, 300), (63, 300, 4097).  The workspace is never read before it is written (runs from 0x00, 0xFF and a larger call's
leftovers give the same bytes) and nothing is written beyond its reported size.  The donor of each shape is the next larger one (of the largest
mmd_weights shape: the same size, other values).
The size functions write no device memory; their refusals and those of the two calls, with canary buffers, are held in
test_gpu_mmd_kernel.py and test_gpu_hamming_pairs_kernel.py (test_refused_sizes_leave_everything_untouched)."""
import numpy as np
import pytest
import torch

import memory_contract as mc
from tensornetworks_amd import _ext, backend
from tensornetworks_amd.hamming_kernel import HammingMixtureKernel

pytestmark = pytest.mark.gpu


def smallest_with_passes(p):
    return next(n for n in range(1, 31) if backend.mmd_passes(n) == p)


MMD_SHAPES = [smallest_with_passes(1), smallest_with_passes(3), smallest_with_passes(5)]
# (the largest shape's donor is the same size with other values: 2^22 doubles a buffer, and an arena of a few hundred MiB, is enough)
MMD_DONOR = {MMD_SHAPES[0]: MMD_SHAPES[1], MMD_SHAPES[1]: MMD_SHAPES[2], MMD_SHAPES[2]: MMD_SHAPES[2]}
PAIR_SHAPES = [(1, 1, 1), (33, 65, 300), (63, 300, 4097)]
PAIR_DONOR = {(1, 1, 1): (33, 65, 300), (33, 65, 300): (63, 300, 4097), (63, 300, 4097): (63, 400, 5000)}


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def build_mmd(n, seed):
    rng = np.random.default_rng([seed, n])
    N = 1 << n
    q = rng.random(N)
    q /= q.sum()
    target = np.bincount(rng.integers(0, N, 200), minlength=N) / 200.0
    lam = HammingMixtureKernel(n, (0.05, 1.0, 4.0)).spectrum
    h = _ext.handle_for(dev())
    need = h.size("bornvi_mmd_workspace_bytes", n)
    bufs = [mc.Buffer("q", "in", data=q, align=16), mc.Buffer("target", "in", data=target, align=16), mc.Buffer("lam", "in", data=lam),
            mc.Buffer("loss", "out", nbytes=8), mc.Buffer("w", "out", nbytes=8 * N, align=16, optional=True),
            mc.Buffer("workspace", "workspace", nbytes=need, align=mc.WS_ALIGN)]

    def run(mem, addr):
        h.call("bornvi_mmd_weights", n, addr["q"], addr["target"], addr["lam"], addr["loss"], addr["w"], addr["workspace"], need, None)
    return mc.Case(bufs, run)


@pytest.mark.parametrize("n", MMD_SHAPES)
def test_mmd_weights_memory_contract(n):
    out = mc.check_case(build_mmd(n, 0), build_mmd(MMD_DONOR[n], 1), dev())
    loss = out["loss"].cpu().numpy().view(np.float64)
    w = out["w"].cpu().numpy().view(np.float64)
    assert np.isfinite(loss).all() and loss[0] > 0 and np.isfinite(w).all() and w.shape == (1 << n,)


def build_pairs(shape, seed):
    n, A, B = shape
    rng = np.random.default_rng([seed, n, A, B])
    top = 1 << min(n, 62)
    za = rng.integers(0, top, A, dtype=np.int64)
    zb = rng.integers(0, top, B, dtype=np.int64)
    if n == 63:
        za |= rng.integers(0, 2, A, dtype=np.int64) << 62
    kappa = HammingMixtureKernel(n).kappa
    h = _ext.handle_for(dev())
    need = h.size("bornvi_hamming_pairs_workspace_bytes", n, A, B)
    bufs = [mc.Buffer("za", "in", data=za), mc.Buffer("zb", "in", data=zb), mc.Buffer("kappa", "in", data=kappa),
            mc.Buffer("r", "out", nbytes=8 * A), mc.Buffer("total", "out", nbytes=8),
            mc.Buffer("counts", "out", nbytes=4 * A * (n + 1), align=4, optional=True),
            mc.Buffer("workspace", "workspace", nbytes=need, align=mc.WS_ALIGN)]

    def run(mem, addr):
        h.call("bornvi_hamming_pairs_rowsum", n, A, addr["za"], B, addr["zb"], 0, addr["kappa"], addr["r"], addr["total"], addr["counts"],
               addr["workspace"], need, None)
    return mc.Case(bufs, run)


@pytest.mark.parametrize("shape", PAIR_SHAPES)
def test_hamming_pairs_memory_contract(shape):
    out = mc.check_case(build_pairs(shape, 0), build_pairs(PAIR_DONOR[shape], 1), dev())
    n, A, B = shape
    counts = out["counts"].cpu().numpy().view(np.int32).reshape(A, n + 1)
    r = out["r"].cpu().numpy().view(np.float64)
    assert np.all(counts.sum(axis=1) == B) and np.all(counts >= 0) and np.isfinite(r).all() and np.all(r > 0)
