"""bornvi_mmd_weights on the GPU against the extended-precision mirror (tests/mmd_mirror.py).

Shapes: n = 1 and 2, then every n at which the number of tile passes changes with the n just below it, read from the library's
own geometry (backend.mmd_passes: 1, 3 and 5 passes), so one three-pass and one five-pass n are among them.  q is a normalised
random vector with a few exact zeros; the target a 200-point empirical distribution, or NULL; one length scale, and three with a
narrow 0.05.

Bound per entry against the longdouble mirror:  |w_z - ref_z| <= 2 (2 n + 4) eps kappa[0] ||d||_1 -- each transform of n
butterfly stages has |error| <= gamma_n ||d||_1 per entry (every entry of H is +-1), the scale adds two roundings, the
spectrum sums to 2^-n sum lam = kappa[0] so the second transform amplifies by at most that, and w carries the factor 2.
Loss:  |L - ref| <= (2 n + 6) eps kappa[0] ||d||_1^2.  The references are computed once per (n, kernel) and shared."""
import functools

import numpy as np
import pytest
import torch

import mmd_mirror as mm
from tensornetworks_amd import _ext, backend
from tensornetworks_amd.hamming_kernel import HammingMixtureKernel

pytestmark = pytest.mark.gpu

EPS = mm.EPS64
SCALES = {"one": (1.0,), "three": (0.05, 1.0, 4.0)}


def pass_change_shapes():
    """n = 1, 2, and each n whose pass count differs from n - 1's, with that n - 1 (host only: the library's geometry)."""
    ns = {1, 2}
    for n in range(2, 31):
        if backend.mmd_passes(n) != backend.mmd_passes(n - 1):
            ns.update((n - 1, n))
    return sorted(ns)


SHAPES = pass_change_shapes()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def inputs(n):
    rng = np.random.default_rng([7, n])
    N = 1 << n
    q = rng.random(N)
    if N > 8:
        q[rng.choice(N, 3, replace=False)] = 0.0
    q /= q.sum()
    t = np.bincount(rng.integers(0, N, 200), minlength=N) / 200.0
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


def reference(n, kind, with_target):
    """(L, w) of the longdouble mirror, ||d||_1 and the kernel; the two forward transforms are computed once per n and shared."""
    q, t = inputs(n)
    k = HammingMixtureKernel(n, SCALES[kind])
    _, lam = mm.tables(n, SCALES[kind])
    qh, th = forward(n)                              # the transform is linear: H (q - t) = H q - H t in extended precision
    dh = qh - th if with_target else qh
    y = lam[mm.popcounts(n)] * dh
    L = (y * dh).sum() / mm.LD(2) ** n
    w = mm.wht(y, mm.LD) * (mm.LD(2) / mm.LD(2) ** n)
    d1 = float(np.abs(q - t).sum()) if with_target else float(np.abs(q).sum())
    return L, w, d1, k


@functools.lru_cache(maxsize=None)
def forward(n):
    q, t = inputs(n)
    return mm.wht(q, mm.LD), mm.wht(t, mm.LD)


def test_the_shapes_cover_every_pass_count():
    counts = [backend.mmd_passes(n) for n in SHAPES]
    assert set(counts) == {1, 3, 5} and SHAPES[:2] == [1, 2]
    t = backend.MMD_TILE_BITS
    assert t in SHAPES and t + 1 in SHAPES and backend.mmd_passes(t) == 1 and backend.mmd_passes(t + 1) == 3


@pytest.mark.parametrize("with_target", [True, False])
@pytest.mark.parametrize("kind", ["one", "three"])
@pytest.mark.parametrize("n", SHAPES)
def test_weights_and_loss_within_the_bound(n, kind, with_target):
    q, t = inputs(n)
    L_ref, w_ref, d1, k = reference(n, kind, with_target)
    qd = torch.from_numpy(q).to(dev())
    td = torch.from_numpy(t).to(dev()) if with_target else None
    lam = k.spectrum_on(dev())
    loss, w = backend.mmd_weights(qd, td, lam)
    err = float(np.abs(w.cpu().numpy().astype(mm.LD) - w_ref).max())
    bound = 2 * (2 * n + 4) * EPS * k.kappa[0] * d1
    lerr = abs(float(mm.LD(loss.item()) - L_ref))
    lbound = (2 * n + 6) * EPS * k.kappa[0] * d1 * d1
    print(f"n={n} {kind} target={with_target}: w err {err / (EPS * k.kappa[0] * d1):.3f} of eps kappa0 |d|_1 (bound {2 * (2 * n + 4)}), "
          f"loss err {lerr / (EPS * k.kappa[0] * d1 * d1):.3f} (bound {2 * n + 6})")
    assert err <= bound
    assert lerr <= lbound and loss.item() >= 0.0
    # the loss alone: the same bits; a second call: the same bits
    loss_only, none = backend.mmd_weights(qd, td, lam, want_w=False)
    assert none is None and torch.equal(loss_only, loss)
    loss2, w2 = backend.mmd_weights(qd, td, lam)
    assert torch.equal(loss2, loss) and torch.equal(w2, w)
    # out= is written in place
    out = torch.full_like(qd, 3.0)
    assert backend.mmd_weights(qd, td, lam, out=out)[1] is out and torch.equal(out, w)


@pytest.mark.parametrize("n", SHAPES)
def test_loss_is_exactly_zero_at_the_target(n):
    q, _ = inputs(n)
    k = HammingMixtureKernel(n, SCALES["three"])
    qd = torch.from_numpy(q).to(dev())
    for target in (qd, qd.clone()):                 # the same buffer, and a copy
        loss, w = backend.mmd_weights(qd, target, k.spectrum_on(dev()))
        assert loss.item() == 0.0 and not bool(w.any())


def test_w_is_the_gradient_of_the_loss():
    """A central difference of the loss along a random direction against w . direction (n with three passes)."""
    n = backend.MMD_TILE_BITS + 1
    q, t = inputs(n)
    k = HammingMixtureKernel(n, SCALES["three"])
    lam = k.spectrum_on(dev())
    qd, td = torch.from_numpy(q).to(dev()), torch.from_numpy(t).to(dev())
    _, w = backend.mmd_weights(qd, td, lam)
    v = torch.from_numpy(np.random.default_rng(1).standard_normal(1 << n) / (1 << n)).to(dev())
    lp = backend.mmd_weights(qd + v, td, lam, want_w=False)[0].item()
    lm = backend.mmd_weights(qd - v, td, lam, want_w=False)[0].item()
    dd = float(w @ v)
    assert abs((lp - lm) / 2 - dd) <= 1e-9 * abs(dd)        # (the loss is quadratic: the central difference is exact to rounding)


def test_refused_sizes_leave_everything_untouched():
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    UNSUPPORTED = _ext._ENUMS["BORNVI_ERR_UNSUPPORTED"]
    size = lib.bornvi_mmd_workspace_bytes
    assert size(h.h, 0) == 0 and size(h.h, 31) == 0 and lib.bornvi_mmd_passes(0) == 0 and lib.bornvi_mmd_passes(31) == 0
    n = backend.MMD_TILE_BITS + 1
    need = size(h.h, n)
    assert need >= (8 << n)                          # (room for the 2^n doubles between passes when w is NULL)
    canary = lambda count, dtype: torch.full((count,), 77, dtype=dtype, device=dev())
    ws, w, loss = canary(need, torch.uint8), canary(1 << n, torch.float64), canary(1, torch.float64)
    q = torch.full((1 << n,), 2.0 ** -n, dtype=torch.float64, device=dev())
    lam = torch.ones(n + 1, dtype=torch.float64, device=dev())
    P = lambda t: t.data_ptr()
    for nn, bytes_ in ((0, need), (31, need), (-1, need), (n, need - 1), (n, 0)):
        assert lib.bornvi_mmd_weights(h.h, nn, P(q), None, P(lam), P(loss), P(w), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_mmd_weights(h.h, nn, P(q), P(q), P(lam), P(loss), None, P(ws), bytes_, None) == UNSUPPORTED
    assert lib.bornvi_mmd_weights(h.h, n, P(q), None, P(lam), P(loss), P(w), None, need, None) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (ws, w, loss):
        assert bool((t == 77).all())


def test_capture_and_replay():
    """The call inside a HIP graph: a replay on new q gives the eager call's bits (three-pass n, with and without w)."""
    n = backend.MMD_TILE_BITS + 1
    q, t = inputs(n)
    k = HammingMixtureKernel(n, SCALES["three"])
    lam = k.spectrum_on(dev())
    qd, td = torch.from_numpy(q).to(dev()), torch.from_numpy(t).to(dev())
    other = torch.roll(qd, 5)
    eager = [(l.clone(), w.clone()) for l, w in (backend.mmd_weights(x, td, lam) for x in (qd, other))]
    buf = qd.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        backend.mmd_weights(buf, td, lam)                     # (the workspace of this stream exists before the capture)
        backend.mmd_weights(buf, td, lam, want_w=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        loss, w = backend.mmd_weights(buf, td, lam)
        loss_only, _ = backend.mmd_weights(buf, td, lam, want_w=False)
    for x, (l_e, w_e) in zip((qd, other), eager):
        buf.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, l_e) and torch.equal(w, w_e) and torch.equal(loss_only, l_e)
