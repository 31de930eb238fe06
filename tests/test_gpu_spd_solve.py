"""bornvi_spd_solve: backward-stable residuals in extended precision, the failure rule, A untouched, bitwise reproducible,
refused arguments, capturable.

Bound (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4 with eq. 10.7; the Frobenius norm stands in as
an upper bound of the 2-norm):  ||(A + lam I) x - b||_2 <= gamma P ||A + lam I||_F ||x||_2,
gamma = (3P + 1) u / (1 - (3P + 1) u), u = 2^-53.  It holds for any order of the sums, so it is derived, not fitted."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import natgrad_mirror as nm

SIZES = [1, 2, 3, 17, 64, 65, 288]
U = 2.0 ** -53

_cache = {}


def system(P, cond):
    """A = G G^T / m + delta I with G [P, m], m = max(1, P // 2) (rank deficient from P = 2 on), delta = lambda_max / cond;
    b random.  Computed once per case."""
    if (P, cond) not in _cache:
        rng = np.random.default_rng([P, int(np.log10(cond)), 5])
        m = max(1, P // 2)
        G = rng.standard_normal((P, m))
        A0 = G @ G.T / m
        A0 = 0.5 * (A0 + A0.T)
        A = A0 + np.eye(P) * (np.linalg.eigvalsh(A0).max() / cond)
        b = rng.standard_normal(P)
        A.setflags(write=False)
        b.setflags(write=False)
        _cache[(P, cond)] = (A, b)
    return _cache[(P, cond)]


def residual_ratio(A, lam, x, b):
    X = hp.arithmetic()
    P = b.size
    M = X.arr(A) + X.arr(np.eye(P)) * X.num(lam)
    res = M @ X.arr(x) - X.arr(b)
    g = (3 * P + 1) * U / (1 - (3 * P + 1) * U)
    bound = g * P * float(np.sqrt((M * M).sum())) * float(np.linalg.norm(x))
    return float(np.sqrt((res * res).sum())) / bound


@pytest.mark.parametrize("P", SIZES)
def test_mirror_is_inside_the_bound(P):
    for cond in (1e2, 1e8):
        for lam in (0.0, 1e-3):
            A, b = system(P, cond)
            x, info = nm.spd_solve(A, b, lam)
            assert info == 0 and residual_ratio(A, lam, x, b) <= 1.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def solve(A, b, lam, dev):
    from tensornetworks_amd import backend
    Ad = torch.from_numpy(np.array(A, dtype=np.float64)).to(dev)
    keep = Ad.clone()
    x, info = backend.spd_solve(Ad, torch.from_numpy(np.array(b, dtype=np.float64)).to(dev), lam)
    assert torch.equal(Ad.view(torch.int64), keep.view(torch.int64))          # A is left untouched
    return x, info


def same_bits(x, b):
    return np.array_equal(x.cpu().numpy().view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("P", SIZES)
def test_residual_in_extended_precision(dev, P):
    for cond in (1e2, 1e8):
        for lam in (0.0, 1e-3):
            A, b = system(P, cond)
            x, info = solve(A, b, lam, dev)
            assert int(info) == 0 and x.shape == (P,)
            r = residual_ratio(A, lam, x.cpu().numpy(), b)
            x_m, _ = nm.spd_solve(A, b, lam)
            print(f"P={P} cond={cond:.0e} damping={lam}: residual / bound {r:.3e}; max |x - mirror| / max |x| "
                  f"{np.abs(x.cpu().numpy() - x_m).max() / np.abs(x_m).max():.3e}")
            assert r <= 1.0, (P, cond, lam, r)
            x2, info2 = solve(A, b, lam, dev)
            assert torch.equal(x, x2) and int(info2) == 0                     # two calls are bitwise equal
            # only the upper triangle is read
            junk = np.triu(A) + np.tril(np.full((P, P), 1e9), -1)
            x3, info3 = solve(junk, b, lam, dev)
            assert torch.equal(x, x3) and int(info3) == 0


@pytest.mark.gpu
def test_failure_rule(dev):
    b = np.array([1.5, -2.5])
    x, info = solve(np.diag([1.0, -1.0]), b, 0.0, dev)
    assert int(info) == 2 and same_bits(x, b)
    x, info = solve(np.diag([1.0, -1.0]), b, 2.0, dev)                        # damped past the negative pivot
    assert int(info) == 0
    np.testing.assert_allclose(x.cpu().numpy(), [0.5, -2.5], rtol=1e-15)
    x, info = solve(np.zeros((2, 2)), b, 0.0, dev)
    assert int(info) == 1 and same_bits(x, b)
    for P in (3, 65, 288):
        A, b = system(P, 1e2)
        for k, bad in ((0, np.nan), (P // 2, np.nan), (P - 1, np.inf), (P - 1, -np.inf)):
            An = A.copy()
            An[0 if k == 0 else k - 1, k] = bad                               # in the upper triangle
            x, info = solve(An, b, 1e-3, dev)
            assert 0 < int(info) <= k + 1 and same_bits(x, b), (P, k, bad, int(info))
            assert nm.spd_solve(An, b, 1e-3)[1] == int(info)
            bn = b.copy()
            bn[k] = bad
            x, info = solve(A, bn, 1e-3, dev)
            assert int(info) == P + 1 and same_bits(x, bn), (P, k, bad, int(info))
        # an indefinite matrix: the first non-positive pivot is the mirror's
        Ai = A - np.eye(P) * 0.5 * np.linalg.eigvalsh(A).max()
        x, info = solve(Ai, b, 0.0, dev)
        assert int(info) == nm.spd_solve(Ai, b, 0.0)[1] > 0 and same_bits(x, b)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(dev):
    import ctypes as C
    from tensornetworks_amd import _ext, backend
    h = _ext.handle_for(dev)
    lib = _ext.lib()
    A = torch.eye(2, dtype=torch.float64, device=dev)
    b = torch.ones(2, dtype=torch.float64, device=dev)
    x = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    info = torch.full((1,), 7, dtype=torch.int32, device=dev)
    ws = torch.empty(h.size("bornvi_spd_solve_workspace_bytes", 2), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(P=2, lam=0.0, A_=A, b_=b, x_=x, info_=info, ws_bytes=None):
        return lib.bornvi_spd_solve(h.h, P, p(A_), lam, p(b_), p(x_), p(info_), p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                    _ext.stream_ptr(dev))
    for rc in (call(P=0), call(P=1025), call(lam=-1e-3), call(lam=float("nan")), call(lam=float("inf")), call(A_=None),
               call(b_=None), call(x_=None), call(info_=None)):
        assert rc == -1 and lib.bornvi_last_error(h.h)
    assert call(ws_bytes=8) == -3
    assert lib.bornvi_spd_solve_workspace_bytes(h.h, 0) == 0 and lib.bornvi_spd_solve_workspace_bytes(h.h, 1025) == 0
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and int(info) == 7                          # nothing ran
    assert call(lam=3.0) == 0                                                 # 4 I: the square root is exact
    torch.cuda.synchronize()
    assert int(info) == 0 and bool((x == 0.25).all())
    for bad in (lambda: backend.spd_solve(A.float(), b), lambda: backend.spd_solve(A, b.cpu()), lambda: backend.spd_solve(A, b[:1]),
                lambda: backend.spd_solve(A, b, -1.0), lambda: backend.spd_solve(A[:1], b)):
        with pytest.raises(backend.BornviError):
            bad()


@pytest.mark.gpu
def test_capture_and_replay(dev):
    from tensornetworks_amd import backend
    A, b = system(65, 1e2)
    eager, _ = solve(A, b, 1e-3, dev)
    Ad, bd = torch.from_numpy(A.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        backend.spd_solve(Ad, bd, 1e-3)               # the side stream's workspace exists before the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        x, info = backend.spd_solve(Ad, bd, 1e-3)
    x.zero_()
    info.fill_(9)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(x, eager) and int(info) == 0
    bd.mul_(2.0)                                      # the replay reads the inputs' current values (a power of two: exact)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(x, 2.0 * eager) and int(info) == 0
