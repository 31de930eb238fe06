"""bornvi_qfi_gram against extended precision, per entry (hp_reference.py arithmetic), and its contract: Q == Q^T bitwise,
bitwise reproducible, non-finite input ends, refused arguments, capturable.

Inputs are random complex rows, not circuit states, so that P and n vary freely (nothing in the kernel assumes unit norm).

Error bound, derived from the shipped layout (kernels_qfi.hip), units of EPS64 = 2^-52 (a correctly rounded operation errs
by at most 1/2).  With S_ab = sum_k |phi_a[k] phi_b[k]| over the K = 2^(n+1) real columns, S_a^re = sum_k |phi_a[k] psi[k]|,
S_a^im the same against i psi, and S^p_ab = S_a^re S_b^re + S_a^im S_b^im:

  |Q_ab - ref| <= eps ((C_TERM + C_CHAIN) S_ab + (2 (C_TERM + C_CHAIN) + C_PROJ) S^p_ab).

  C_TERM = 1: the rows go into LDS as they are (row i psi: an exchange and a sign), so a term carries the product inside
      the MFMA alone (1/2, counted although a fused multiply-add would not round it); the other 1/2 is the final
      subtraction's rounding, at most 1/2 eps |Q_ab| <= 1/2 eps (S_ab + S^p_ab).
  C_CHAIN = (slab + per_wg + G) / 2: every slab starts from a zero accumulator and its MFMAs add at most `slab` products on
      a path; the workgroup adds its per_wg slab results to its partial tile in order, the finishing launch the G partial
      tiles in index order.  syrk::geom: slab = K up to 256 columns, else K / 64 clamped to [256, 4096];
      G = min(K / slab, max(64, K / slab / 1024)); per_wg = K / slab / G (hp_reference.syrk_geometry).  n = 13:
      (256 + 1 + 64) / 2 = 160.5; the largest case here (n = 18, the first with per_wg = 2): (4096 + 2 + 64) / 2 = 2081;
      the largest the library accepts (n = 30): (4096 + 1024 + 512) / 2 = 2816.
  Projection: each of re_a, im_a is such a sum (relative error (C_TERM + C_CHAIN) eps of its S), a product of two carries
      both factors' errors -- the factor 2 --, and C_PROJ = 2 covers the product's rounding (1/2), the sum of the two
      products (1/2), the final subtraction's share (1/2) and the second-order terms.
Neither constant was fitted.  Worst observed ratio of error to bound on an MI355X: 0.26 (P = 288, n = 1), 0.10 at n = 3,
0.011 at n = 9, 0.0086 at n = 13.  The float64 mirror (qng_mirror.qfi) is held to the same bound on the same inputs, on the CPU."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import qng_mirror as qm

C_TERM, C_PROJ = 1.0, 2.0
PS, NS = (1, 2, 17, 64, 65, 288), (1, 3, 9, 13)
# (127, 3): R = 129 rows, psi is the last row of tile 0 and i psi the first of tile 1 -- the projection columns come from two
# tiles; (2, 18): the first n with per_wg = 2
SHAPES = [(P, n) for n in NS for P in PS] + [(127, 3), (2, 18)]
LONGDOUBLE_MAX_N = 20       # the long-double reference costs P^2 2^n products: seconds at the largest shape here


def geometry(n):
    return hp.syrk_geometry(2 << n)


def c_chain(n):
    return hp.syrk_chain(2 << n)


def test_constants():
    assert geometry(1) == (4, 1, 1) and geometry(9) == (256, 1, 4) and geometry(13) == (256, 1, 64)
    assert geometry(3) == (16, 1, 1) and geometry(17) == (4096, 1, 64) and geometry(18) == (4096, 2, 64)
    assert c_chain(13) == 160.5 and c_chain(18) == 2081.0 and c_chain(30) == 2816.0
    assert all(C_TERM + c_chain(n) <= 8 + 4096 for n in range(1, 31))


_cache = {}


def inputs(P, n):
    """(phi [P, N], psi [N]) complex128 and their extended-precision (Q, S, S^p), computed once per shape."""
    if (P, n) not in _cache:
        N = 1 << n
        rng = np.random.default_rng([P, n, 23])
        phi = (rng.standard_normal((P, N)) + 1j * rng.standard_normal((P, N))) / np.sqrt(2 * N)
        psi = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / np.sqrt(2 * N)
        X = hp.arithmetic()
        R = X.arr(qm.real_rows(phi))
        vr, vi = X.arr(qm.real_rows(psi)), X.arr(qm.real_rows(1j * psi))
        rows = reference_rows(P, n)
        re, im = R @ vr, R @ vi
        ref = R[rows] @ R.T - (np.outer(re[rows], re) + np.outer(im[rows], im))
        A = np.abs(R)
        sre, sim = A @ np.abs(vr), A @ np.abs(vi)
        S, Sp = A[rows] @ A.T, np.outer(sre[rows], sre) + np.outer(sim[rows], sim)
        for a in (phi, psi):
            a.setflags(write=False)
        _cache[(P, n)] = (phi, psi, ref, S, Sp, X, rows)
    return _cache[(P, n)]


def reference_rows(P, n):
    """The rows a of Q whose entries (a, every b) are compared: all of them, except at the one shape whose extended-precision
    Gram would take 15 s on the host (P = 288, n = 13: 1.4e9 long-double products, twice) -- there the first and last row
    of every 128-row tile and of every 64-row wave tile, and 12 random ones (24 rows x 288 columns)."""
    if P * P << n <= 1 << 28:
        return np.arange(P)
    edges = [r for t in range(0, P, 64) for r in (t, min(t + 63, P - 1))]
    extra = np.random.default_rng([P, n]).choice(P, 12, replace=False)
    return np.unique(np.concatenate([edges, extra, [P - 1]]))


def check(Q, P, n, what):
    phi, psi, ref, S, Sp, X, rows = inputs(P, n)
    why = hp.unavailable(n, X, longdouble_max_n=LONGDOUBLE_MAX_N)
    if why:
        pytest.skip(why)
    c = C_TERM + c_chain(n)
    bound = S * X.num(c) + Sp * X.num(2 * c + C_PROJ)
    r = hp.worst(hp.ratio(np.asarray(Q)[rows], ref, bound, X=X))
    print(f"{what} P={P} n={n}: worst |Q - ref| / (eps x bound) {r[0]:.4f} at {r[1]} (C_TERM + C_CHAIN = {c})")
    assert r[0] <= 1.0, (what, r)
    return r[0]


@pytest.mark.parametrize("P,n", SHAPES)
def test_mirror_is_inside_the_bound(P, n):
    phi, psi = inputs(P, n)[:2]
    check(qm.qfi(phi, psi), P, n, "mirror")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def run(phi, psi, dev, **kw):
    from tensornetworks_amd import backend
    return backend.qfi_gram(torch.from_numpy(np.array(phi)).to(dev), torch.from_numpy(np.array(psi)).to(dev), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("P,n", SHAPES)
def test_kernel_against_extended_precision(dev, P, n):
    phi, psi = inputs(P, n)[:2]
    Q = run(phi, psi, dev)
    assert Q.shape == (P, P) and Q.dtype == torch.float64
    check(Q.cpu().numpy(), P, n, "kernel")
    assert torch.equal(Q, Q.t())                                  # the lower triangle is the bitwise mirror
    assert torch.equal(Q, run(phi, psi, dev))                     # two calls are bitwise equal


@pytest.mark.gpu
def test_non_finite_input_ends(dev):
    """A NaN and an Inf in the rows: the call returns, the entries of the clean rows among themselves stay finite only
    where psi is clean too (the projection couples every entry to psi), and a NaN row poisons its row and column."""
    P, n = 17, 9
    phi, psi = (np.array(a) for a in inputs(P, n)[:2])
    phi[3, 5] = np.nan
    phi[9, 100] = np.inf
    Q = run(phi, psi, dev).cpu().numpy()
    assert np.isnan(Q[3]).all() and np.isnan(Q[:, 3]).all()
    assert not np.isfinite(Q[9, 9])
    clean = [a for a in range(P) if a not in (3, 9)]
    assert np.isfinite(Q[np.ix_(clean, clean)]).all()
    psi[0] = np.nan
    assert np.isnan(run(phi, psi, dev).cpu().numpy()).all()


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(dev):
    import ctypes as C
    from tensornetworks_amd import _ext, backend
    h = _ext.handle_for(dev)
    lib = _ext.lib()
    n, P = 3, 2
    phi = torch.randn(P, 8, dtype=torch.complex128, device=dev)
    psi = torch.randn(8, dtype=torch.complex128, device=dev)
    Q = torch.full((P, P), 7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(h.size("bornvi_qfi_workspace_bytes", n, P), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(n_=n, P_=P, phi_=phi, psi_=psi, Q_=Q, ws_bytes=None):
        return lib.bornvi_qfi_gram(h.h, n_, P_, p(phi_), p(psi_), p(Q_), p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                   _ext.stream_ptr(dev))
    INVALID, WORKSPACE = -1, -3
    for rc in (call(P_=0), call(P_=1025), call(n_=0), call(n_=31), call(phi_=None), call(psi_=None), call(Q_=None)):
        assert rc == INVALID and lib.bornvi_last_error(h.h)
    assert call(ws_bytes=8) == WORKSPACE and b"workspace" in lib.bornvi_last_error(h.h)
    assert lib.bornvi_qfi_workspace_bytes(h.h, n, 0) == 0 and lib.bornvi_qfi_workspace_bytes(h.h, 31, 1) == 0
    assert lib.bornvi_qfi_workspace_bytes(h.h, n, 1025) == 0
    torch.cuda.synchronize()
    assert bool((Q == 7.0).all())                                 # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose(Q.cpu().numpy(), qm.qfi(phi.cpu().numpy(), psi.cpu().numpy()), rtol=0, atol=1e-13)
    for bad in (lambda: backend.qfi_gram(phi.to(torch.complex64), psi), lambda: backend.qfi_gram(phi, psi.cpu()),
                lambda: backend.qfi_gram(phi[:, :7], psi), lambda: backend.qfi_gram(phi.real.contiguous(), psi)):
        with pytest.raises(backend.BornviError):
            bad()


@pytest.mark.gpu
def test_capture_and_replay(dev):
    """The call inside a torch.cuda.graph capture (P = 288, n = 9: three tile rows, four slab groups): the replay's Q is
    the eager call's, bit for bit, and follows the inputs' current values."""
    from tensornetworks_amd import backend
    phi, psi = inputs(288, 9)[:2]
    eager = run(phi, psi, dev)
    pd, sd = torch.from_numpy(np.array(phi)).to(dev), torch.from_numpy(np.array(psi)).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        backend.qfi_gram(pd, sd)                      # the side stream's workspace exists before the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = backend.qfi_gram(pd, sd)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, eager)
    pd.copy_(torch.from_numpy(np.array(phi[::-1])).to(dev))       # the parameters in reverse order
    graph.replay()
    torch.cuda.synchronize(dev)
    np.testing.assert_allclose(out.cpu().numpy(), eager.cpu().numpy()[::-1, ::-1], rtol=0, atol=1e-13)
    assert torch.equal(out, out.t())
