"""bornvi_fisher_gram against extended precision, per entry (hp_reference.py arithmetic), and its contract: F == F^T
bitwise, bitwise reproducible, floor entries contribute nothing, refused arguments, capturable.

Inputs are synthetic rows, not circuits, so that P and n vary freely: each (+, -) pair of rows is two Dirichlet draws, q a
third with every seventh entry at 1e-30 (under the floor) and every eleventh exactly 0.

Error bound, derived from the shipped layout (kernels_fisher.hip), units of EPS64 = 2^-52 (a correctly rounded operation
errs by at most 1/2):  |F_ab - ref| <= eps (C_TERM + C_CHAIN) sum_z |d_a d_b| r_z.
  C_TERM = 3: a term is (d_a r) d_b with d = 1/2 (plus - minus): the subtraction of d_a (1/2; the halving is exact), the
      subtraction of d_b (1/2), the IEEE division r = 1 / q (1/2), the product e = d_a r stored to LDS (1/2) and the product
      e d_b inside the MFMA (1/2, counted although a fused multiply-add would not round it): 5/2, rounded up to 3, which
      also covers the second-order terms of (1 + eps/2)^(5 + chain) for every chain below 10^4.
  C_CHAIN = (slab + per_wg + G) / 2: every slab starts from a zero accumulator and its MFMAs add at most `slab` products
      one after the other (whatever order the matrix core uses inside one instruction, a path holds no more additions than
      products); the workgroup then adds its per_wg slab results in order, and the finishing launch the G partial tiles in
      index order.  slab, per_wg and G are syrk::geom's: slab = N up to 256 entries, else N / 64 clamped to [256, 4096];
      G = min(N / slab, max(64, N / slab / 1024)); per_wg = N / slab / G (hp_reference.syrk_geometry).  n = 13:
      (256 + 1 + 32) / 2 = 144.5; the largest case here (n = 19, the first with per_wg = 2): (4096 + 2 + 64) / 2 = 2081;
      the largest the library accepts (n = 30): (4096 + 1024 + 256) / 2 = 2688; C_TERM + C_CHAIN
      stays under the cap 8 + 4096 for every n.
The float64 mirror (natgrad_mirror.py) is held to the same bound on the same inputs, on the CPU."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import natgrad_mirror as nm

Q_FLOOR = 1e-10
C_TERM = 3.0
SHAPES = [(1, 1), (3, 2), (2, 5), (17, 5), (17, 13), (65, 9), (130, 9), (288, 9), (2, 19)]      # (n_shift, n)
LONGDOUBLE_MAX_N = 20       # the long-double reference costs P^2 2^n products: seconds at the largest shape here


def geometry(n):
    return hp.syrk_geometry(1 << n)


def c_chain(n):
    return hp.syrk_chain(1 << n)


def test_constants_stay_under_the_cap():
    assert all(C_TERM + c_chain(n) <= 8 + 4096 for n in range(1, 31))
    assert c_chain(13) == 144.5 and c_chain(30) == 2688.0 and geometry(9) == (256, 1, 2) and geometry(5) == (32, 1, 1)
    assert geometry(18) == (4096, 1, 64) and geometry(19) == (4096, 2, 64) and c_chain(19) == 2081.0


_cache = {}


def inputs(P, n):
    """(shifted [2 P, N], q [N]) float64, and their extended-precision (F, bound), computed once per shape."""
    if (P, n) not in _cache:
        N = 1 << n
        rng = np.random.default_rng([P, n, 17])
        shifted = rng.dirichlet(np.ones(N), size=2 * P)
        q = rng.dirichlet(np.ones(N))
        q[3::7] = 1e-30
        q[5::11] = 0.0
        X = hp.arithmetic()
        d = (X.arr(shifted[0::2]) - X.arr(shifted[1::2])) / 2
        keep = q >= Q_FLOOR
        r = np.where(keep, 1 / np.where(keep, X.arr(q), X.num(1)), X.num(0))
        ref = (d * r[None, :]) @ d.T
        bound = (np.abs(d) * r[None, :]) @ np.abs(d).T
        for a in (shifted, q):
            a.setflags(write=False)
        _cache[(P, n)] = (shifted, q, ref, bound, X)
    return _cache[(P, n)]


def check(F, P, n, what):
    shifted, q, ref, bound, X = inputs(P, n)
    why = hp.unavailable(n, X, longdouble_max_n=LONGDOUBLE_MAX_N)
    if why:
        pytest.skip(why)
    c = C_TERM + c_chain(n)
    r = hp.worst(hp.ratio(F, ref, bound, X=X))
    print(f"{what} P={P} n={n}: worst ratio {r[0]:.3f} / {c} at {r[1]}")
    assert r[0] <= c, (what, r)
    return r[0]


@pytest.mark.parametrize("P,n", SHAPES)
def test_mirror_is_inside_the_bound(P, n):
    shifted, q = inputs(P, n)[:2]
    assert (n < 3) or (((q > 0) & (q < Q_FLOOR)).any() and (q == 0).any())
    check(nm.fisher(shifted, q, Q_FLOOR), P, n, "mirror")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def run(shifted, q, dev, **kw):
    from tensornetworks_amd import backend
    return backend.fisher_gram(torch.from_numpy(np.array(shifted, dtype=np.float64)).to(dev), torch.from_numpy(np.array(q, dtype=np.float64)).to(dev),
                               Q_FLOOR, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("P,n", SHAPES)
def test_kernel_against_extended_precision(dev, P, n):
    shifted, q = inputs(P, n)[:2]
    F = run(shifted, q, dev)
    assert F.shape == (P, P) and F.dtype == torch.float64
    check(F.cpu().numpy(), P, n, "kernel")
    assert torch.equal(F, F.t())                                  # the lower triangle is the bitwise mirror
    assert torch.equal(F, run(shifted, q, dev))                   # two calls are bitwise equal
    # floor entries contribute exactly nothing: whatever their rows hold, no bit of F changes
    under = q < Q_FLOOR
    z = shifted.copy()
    z[:, under] = 0.0
    assert torch.equal(F, run(z, q, dev))
    z[:, under] = 1e300
    assert torch.equal(F, run(z, q, dev))


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(dev):
    import ctypes as C
    from tensornetworks_amd import _ext, backend
    h = _ext.handle_for(dev)
    lib = _ext.lib()
    n, P = 3, 2
    shifted = torch.rand(2 * P, 8, dtype=torch.float64, device=dev)
    q = torch.full((8,), 0.125, dtype=torch.float64, device=dev)
    F = torch.full((P, P), 7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(h.size("bornvi_fisher_workspace_bytes", n, P), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(n_=n, P_=P, floor=Q_FLOOR, sh=shifted, q_=q, F_=F, ws_bytes=None):
        return lib.bornvi_fisher_gram(h.h, n_, p(sh), P_, p(q_), floor, p(F_), p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                      _ext.stream_ptr(dev))
    INVALID, WORKSPACE = -1, -3
    for rc, word in ((call(P_=0), "n_shift"), (call(P_=1025), "n_shift"), (call(floor=0.0), "q_floor"),
                     (call(floor=-1e-10), "q_floor"), (call(floor=float("nan")), "q_floor"), (call(n_=0), "n"), (call(n_=31), "n"),
                     (call(sh=None), "null"), (call(q_=None), "null"), (call(F_=None), "null")):
        assert rc == INVALID and lib.bornvi_last_error(h.h), word
    assert b"q_floor" in (call(floor=0.0), lib.bornvi_last_error(h.h))[1]
    assert call(ws_bytes=8) == WORKSPACE and b"workspace" in lib.bornvi_last_error(h.h)
    assert lib.bornvi_fisher_workspace_bytes(h.h, n, 0) == 0 and lib.bornvi_fisher_workspace_bytes(h.h, 31, 1) == 0
    assert lib.bornvi_fisher_workspace_bytes(h.h, n, 1025) == 0
    torch.cuda.synchronize()
    assert bool((F == 7.0).all())                                 # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose(F.cpu().numpy(), nm.fisher(shifted.cpu().numpy(), q.cpu().numpy()), rtol=1e-13)
    for bad in (lambda: backend.fisher_gram(shifted.float(), q), lambda: backend.fisher_gram(shifted, q.cpu()),
                lambda: backend.fisher_gram(shifted[:3], q), lambda: backend.fisher_gram(shifted, q, 0.0)):
        with pytest.raises(backend.BornviError):
            bad()


@pytest.mark.gpu
def test_capture_and_replay(dev):
    """The call inside a torch.cuda.graph capture (P = 65, n = 9: two tile rows, two slabs); the replay's F is the eager
    call's, bit for bit, and follows the inputs' current values."""
    from tensornetworks_amd import backend
    shifted, q = inputs(65, 9)[:2]
    eager = run(shifted, q, dev)
    sd, qd = torch.from_numpy(shifted.copy()).to(dev), torch.from_numpy(q.copy()).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        backend.fisher_gram(sd, qd, Q_FLOOR)          # the side stream's workspace exists before the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = backend.fisher_gram(sd, qd, Q_FLOOR)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, eager)
    perm = np.arange(2 * 65).reshape(65, 2)[::-1].reshape(-1).copy()      # the parameters in reverse order
    sd.copy_(torch.from_numpy(shifted[perm]).to(dev))
    graph.replay()
    torch.cuda.synchronize(dev)
    np.testing.assert_allclose(out.cpu().numpy(), eager.cpu().numpy()[::-1, ::-1], rtol=1e-12, atol=1e-18)
    assert torch.equal(out, out.t())
