"""bornvi_hamming_pairs_rowsum on the GPU against the NumPy mirror (tests/mmd_mirror.py).

n in {1, 31, 32, 33, 63}: the 32-bit word boundary and the top bit.  (A, B) in {(1, 1), (2, 2), (65, 1), (3, 300), (300, 4097)}: one
lane, a partial wave, several row blocks, a partial column tile, more than one column range; with skip_same_index the square
shapes (A, A) on the same array.  Duplicates on both sides.  The counts are exact, r is the mirror's ascending sum bit for
bit, total is within (A - 1) eps sum |r| of math.fsum(r); r does not depend on the order of zb or on A."""
import functools
import math

import numpy as np
import pytest
import torch

import mmd_mirror as mm
from tensornetworks_amd import _ext, backend
from tensornetworks_amd.hamming_kernel import HammingMixtureKernel

pytestmark = pytest.mark.gpu

EPS = mm.EPS64
NS = [1, 31, 32, 33, 63]
SHAPES = [(1, 1), (2, 2), (65, 1), (3, 300), (300, 4097)]
SQUARE = [1, 2, 3, 65, 300]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def states(rng, n, count):
    """int64 states below 2^n (the top bit of n = 63 set in about half), with duplicates when count > 2."""
    z = rng.integers(0, 1 << min(n, 62), count, dtype=np.int64)
    if n == 63:
        z |= rng.integers(0, 2, count, dtype=np.int64) << 62
    if count > 2:
        z[count // 2] = z[0]
        z[-1] = z[1]
    return z


@functools.lru_cache(maxsize=None)
def case(n, A, B, skip):
    rng = np.random.default_rng([n, A, B, int(skip)])
    za = states(rng, n, A)
    zb = za if skip else states(rng, n, B)
    if not skip and B > 4 and A > 1:
        zb[3] = za[0]                               # a state on both sides
    k = HammingMixtureKernel(n)
    cnt = mm.pair_counts_fast(za, zb, n, skip)
    return za, zb, k, cnt, mm.rowsum(cnt, k.kappa)


def run(za, zb, k, skip, counts=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return backend.hamming_pairs_rowsum(t(za), t(zb), k.kappa_on(dev()), skip, counts)


def check(n, A, B, skip):
    za, zb, k, cnt, r_ref = case(n, A, B, skip)
    r, total, counts = run(za, zb, k, skip)
    counts = counts.cpu().numpy()
    assert counts.dtype == np.int32 and counts.shape == (A, n + 1)
    assert np.array_equal(counts, cnt) and np.all(counts.sum(axis=1) == (B - 1 if skip else B))
    r = r.cpu().numpy()
    assert np.array_equal(r, r_ref)                 # bit for bit: ascending d, multiply and add rounded separately
    assert abs(total.item() - math.fsum(r)) <= (A - 1) * EPS * np.abs(r).sum()
    # without the counts: the same bits; a second call: the same bits
    r2, total2, none = run(za, zb, k, skip, counts=False)
    assert none is None and np.array_equal(r2.cpu().numpy(), r) and torch.equal(total2, total)
    return r, total


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", NS)
def test_counts_rows_and_total(n, shape):
    check(n, shape[0], shape[1], False)


@pytest.mark.parametrize("A", SQUARE)
@pytest.mark.parametrize("n", NS)
def test_skip_same_index(n, A):
    check(n, A, A, True)


@pytest.mark.parametrize("n", [1, 33, 63])
def test_rows_do_not_depend_on_the_order_of_zb_or_on_A(n):
    A, B = 300, 4097
    za, zb, k, cnt, r_ref = case(n, A, B, False)
    perm = np.random.default_rng(5).permutation(B)
    r_perm, _, _ = run(za, zb[perm], k, False, counts=False)
    assert np.array_equal(r_perm.cpu().numpy(), r_ref)
    for prefix in (1, 65, 129):
        r_pre, total_pre, _ = run(za[:prefix], zb, k, False, counts=False)
        assert np.array_equal(r_pre.cpu().numpy(), r_ref[:prefix])
        assert abs(total_pre.item() - math.fsum(r_ref[:prefix])) <= (prefix - 1) * EPS * np.abs(r_ref[:prefix]).sum()


def test_the_top_word_is_counted():
    """n = 63: states that differ in the bits 32 .. 62 only."""
    n = 63
    za = np.array([0, (1 << 63) - 1, 1 << 62, 1 << 32], dtype=np.int64)
    zb = np.array([0, 1 << 62, (1 << 62) | (1 << 31)], dtype=np.int64)
    k = HammingMixtureKernel(n)
    _, _, counts = run(za, zb, k, False)
    want = mm.pair_counts(za, zb, n)
    assert np.array_equal(counts.cpu().numpy(), want) and want[1, 63] == 1 and want[2, 0] == 1


def test_refused_sizes_leave_everything_untouched():
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    UNSUPPORTED = _ext._ENUMS["BORNVI_ERR_UNSUPPORTED"]
    size = lib.bornvi_hamming_pairs_workspace_bytes
    bad = ((0, 8, 8), (64, 8, 8), (8, 0, 8), (8, (1 << 17) + 1, 8), (8, 8, 0), (8, 8, (1 << 20) + 1))
    for n, A, B in bad:
        assert size(h.h, n, A, B) == 0
    n, A, B = 8, 8, 8
    need = size(h.h, n, A, B)
    assert need > 0
    canary = lambda count, dtype: torch.full((count,), 77, dtype=dtype, device=dev())
    ws, r, total, counts = canary(need, torch.uint8), canary(A, torch.float64), canary(1, torch.float64), canary(A * (n + 1), torch.int32)
    z = torch.arange(A, dtype=torch.int64, device=dev())
    kappa = torch.ones(n + 1, dtype=torch.float64, device=dev())
    P = lambda t: t.data_ptr()
    for nn, AA, BB, bytes_ in tuple(b + (need,) for b in bad) + ((n, A, B, need - 1), (n, A, B, 0)):
        for skip in (0, 1):
            assert lib.bornvi_hamming_pairs_rowsum(h.h, nn, AA, P(z), BB, P(z), skip, P(kappa), P(r), P(total), P(counts), P(ws), bytes_,
                                                   None) == UNSUPPORTED
    assert lib.bornvi_hamming_pairs_rowsum(h.h, n, A, P(z), B, P(z), 0, P(kappa), P(r), P(total), P(counts), None, need, None) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (ws, r, total, counts):
        assert bool((t == 77).all())
    with pytest.raises(backend.BornviError):
        backend.hamming_pairs_rowsum(z.to(torch.int32), z, kappa)
    with pytest.raises(backend.BornviError):
        backend.hamming_pairs_rowsum(z, z, kappa.to(torch.float32))


def test_capture_and_replay():
    n, A, B = 33, 65, 300
    za, zb, k, cnt, r_ref = case(n, A, B, False)
    kappa = k.kappa_on(dev())
    a, b = torch.from_numpy(za).to(dev()), torch.from_numpy(zb).to(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        backend.hamming_pairs_rowsum(a, b, kappa)             # (the workspace of this stream exists before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        r, total, _ = backend.hamming_pairs_rowsum(a, b, kappa)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy(), r_ref)
    b.copy_(torch.roll(b, 7))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy(), r_ref)            # (a permutation of zb: the same rows)
