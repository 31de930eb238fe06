"""bornvi_cg_init / _step / _finish and CGFisherPreconditioner on the MI355X against the mirrors (cg_natgrad_mirror.py on
sampled_fisher_mirror.py): the first iterate in closed form, convergence judged by the TRUE residual in extended precision,
the shape no other full-matrix step takes, frozen iterations, the fallbacks, the refused arguments, capturable."""
import functools

import numpy as np
import pytest
import torch

import cg_natgrad_mirror as cm
import hp_reference as hp
import mps_sampled_mirror as sm
import sampled_fisher_mirror as fm
from tensornetworks_amd import backend
from tensornetworks_amd.backend import cg_finish, cg_init, cg_step, mps_score_jvp  # noqa: F401  (fails without the feature)
from tensornetworks_amd.natural_gradient import CGFisherPreconditioner, SampledFisherPreconditioner
from test_gpu_mps_sampled_kernel import c_score, make_cores
from test_gpu_sampled_natgrad_kernel import rows_inputs

pytestmark = pytest.mark.gpu
EPS = hp.EPS64
LD = sm.LD


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def problem(n, D, B, seed=8):
    """cores, samples and the gradient g = mps_score_vjp(w) of a random w on the device, with the mirror's rows X [P, B] in
    extended precision and in float64; computed once per shape."""
    cores = make_cores(n, D, seed=seed).to(dev())
    bits = rows_inputs(n, D, B)
    idx = torch.from_numpy(sm.idx_of_bits(bits)).to(dev())
    w = torch.from_numpy(np.random.default_rng(seed).standard_normal(B)).to(dev())
    backend.mps_environments(cores, B)
    g, _, _ = backend.mps_score_vjp(cores, idx, w)
    env = sm.environments(cores.cpu().numpy())
    sr = fm.score_rows(cores.cpu().numpy(), bits, env)
    X = sr["rows"].reshape(-1, B)
    return dict(cores=cores, bits=bits, idx=idx, g=g.clone(), gn=g.cpu().numpy().reshape(-1), env=env, sr=sr, X=X, X64=hp.to_f64(X))


@functools.lru_cache(maxsize=None)
def solve(n, D, B, lam, K, tol):
    """One device solve -> (x, info, iters, relres, status) on the host."""
    Q = problem(n, D, B)
    pre = CGFisherPreconditioner(damping=lam, max_iters=K, rel_tol=tol)
    backend.mps_environments(Q["cores"], B)
    x, info = pre.precondition(Q["cores"], Q["idx"], Q["g"])
    return (x.cpu().numpy().copy(), int(info.item()), int(pre.iters.item()), float(pre.relres.item()), int(pre.status.item()))


def test_the_first_iterate_in_closed_form():
    """max_iters = 1: x = alpha_0 g, alpha_0 = g^T g / g^T (F^ + lam I) g from the mirror in extended precision.  Per-entry bound,
    units of EPS64 on |alpha_0 g_i|, every rounding a whole unit, from the three reductions involved:
      g^T g: positive terms; a thread's chain of m = ceil(P / 1024) fmas, 6 butterfly levels, 16 waves: C_DOT = m + 22;
      F p = O^T (O p / B): the sum over the samples inside mps_score_vjp (C_SCORE on grad_abs at the weights |t|) on top of the
        jvp's own error (C_JVP on t_abs), both against A_i = sum_b rows_abs[i, b] t_abs_b;
      p^T q, q = fma(lam, p, Fp) (1): C_PQ = C_DOT + 1 + C_SCORE + C_JVP on pq_abs = sum_i |g_i| (A_i + lam |g_i|), relative to
        pq through kappa_pq = pq_abs / pq;
      the quotient and the product alpha p_i: 2.
    C = C_DOT + C_PQ kappa_pq + 2, printed, not fitted."""
    n, D, B, lam = 5, 3, 130, 1e-2
    Q = problem(n, D, B)
    x, info, iters, relres, status = solve(n, D, B, lam, 1, 0.0)
    assert (info, iters, status) == (0, 1, 0) and relres > 0.0 and np.isfinite(relres)
    g, X = Q["gn"].astype(LD), Q["X"]
    Fg = cm.matvec(X)(g)
    pq = g @ (Fg + LD(lam) * g)
    alpha0 = (g @ g) / pq
    P = g.size
    kZ = float(Q["env"]["Z_abs"] / Q["env"]["Z"])
    kappa = hp.to_f64(Q["sr"]["kappa"])
    t_abs = cm.jvp(Q["cores"].cpu().numpy(), Q["bits"], Q["gn"].reshape(n, 2, D, D), sr=Q["sr"])["t_abs"] / LD(B)
    A = Q["sr"]["rows_abs"].reshape(P, B) @ t_abs
    pq_abs = np.abs(g) @ (A + LD(lam) * np.abs(g))
    c_dot = -(-P // 1024) + 22
    c_pq = c_dot + 1 + c_score(n, D, B, float(kappa.max()), kZ) + float(cm.c_jvp(n, D, kappa, kZ).max())
    C = c_dot + c_pq * float(pq_abs / pq) + 2
    r = hp.ratio(x.reshape(-1), alpha0 * g, np.abs(alpha0 * g), X=hp._LongDouble) / C
    w, at = hp.worst(r)
    print(f"K = 1: alpha_0 = {float(alpha0):.6e}, worst |x - alpha_0 g| / (C EPS |alpha_0 g|) = {w:.4f} at {at}, C = {C:.0f} "
          f"(C_DOT {c_dot}, C_PQ {c_pq:.0f}, kappa_pq {float(pq_abs / pq):.2f})")
    assert w <= 1.0


def true_residual_rule(Q, x, lam, K, tol):
    """(rho, rho_mirror, bound): the device x's true residual, the float64 mirror CG's on the same inputs at the same K, and
    max(2 rel_tol, 4 rho_mirror) (4: another order of summation)."""
    rho = cm.residual(Q["X"], Q["gn"], x.reshape(-1), lam)
    mir = cm.cg(cm.matvec(Q["X64"]), Q["gn"], lam, K, tol, np.float64)
    rho_m = cm.residual(Q["X"], Q["gn"], mir["x"], lam)
    return rho, rho_m, max(2 * tol, 4 * rho_m), mir


def test_convergence_by_the_true_residual():
    """(5, 3, 130): P = 90, lam = 1e-2, rel_tol = 1e-10, max_iters = 200.  On the CPU the float64 mirror converges in 56
    iterations (relres 5.3e-12, true residual 5.3e-12; the extended-precision recurrence takes 49).  The device: info 0,
    relres <= rel_tol, true residual rho <= max(2 rel_tol, 4 rho_mirror); and delta against the device's own blocks='full'
    Cholesky step within (amp rel_tol + 1e3 EPS amp) ||ref||_inf, amp = (||F^||_inf + lam) / lam from the mirror."""
    n, D, B, lam, K, tol = 5, 3, 130, 1e-2, 200, 1e-10
    Q = problem(n, D, B)
    x, info, iters, relres, status = solve(n, D, B, lam, K, tol)
    rho, rho_m, bound, mir = true_residual_rule(Q, x, lam, K, tol)
    print(f"(5, 3, 130): {iters} iterations (float64 mirror {mir['iters']}), relres {relres:.3e}, true residual {rho:.3e} "
          f"(mirror {rho_m:.3e}), bound {bound:.3e}")
    assert (info, status) == (0, 0) and mir["done"] and 0 < iters < K
    assert relres <= tol and rho <= bound
    full, finfo = SampledFisherPreconditioner(damping=lam, blocks='full').precondition(Q["cores"], Q["idx"], Q["g"])
    ref = full.cpu().numpy().reshape(-1)
    amp = (float(np.abs(Q["X64"] @ Q["X64"].T).sum(axis=1).max()) / B + lam) / lam
    err = np.abs(x.reshape(-1) - ref).max() / np.abs(ref).max()
    print(f"  against the device's blocks='full' delta: {err:.3e}, bound {amp * tol + 1e3 * EPS * amp:.3e} (amp {amp:.3e})")
    assert finfo.tolist() == [0] and err <= amp * tol + 1e3 * EPS * amp


def test_the_shape_nothing_else_takes():
    """(9, 8, 1100): P = 1152 > 1024 and B > 1024, so blocks='full' and 'sample' both refuse it.  lam = 1e-2, rel_tol = 1e-8.
    F^ has rank 257 here and a condition number of 3e7 after damping; on the CPU the float64 mirror needs 2090 iterations
    (true residual 8.1e-9), so max_iters = 3200 leaves half as many again.  info 0, converged, and the true residual, formed
    matrix-free in extended precision, by the rule of the test above."""
    n, D, B, lam, K, tol = 9, 8, 1100, 1e-2, 3200, 1e-8
    for spec in (SampledFisherPreconditioner(blocks='full'), SampledFisherPreconditioner.coerce('sample')):
        with pytest.raises(ValueError):
            spec.plan(n, D, B)
    Q = problem(n, D, B)
    x, info, iters, relres, status = solve(n, D, B, lam, K, tol)
    rho, rho_m, bound, mir = true_residual_rule(Q, x, lam, K, tol)
    print(f"(9, 8, 1100): {iters} iterations (float64 mirror {mir['iters']}), relres {relres:.3e}, true residual {rho:.3e} "
          f"(mirror {rho_m:.3e}), bound {bound:.3e}")
    assert (info, status) == (0, 0) and mir["done"] and 0 < iters < K
    assert relres <= tol and rho <= bound


def test_converged_iterations_are_frozen():
    """Once converged, max_iters = K and K + 7 give the same bits of x, iters and relres."""
    a = solve(5, 3, 130, 1e-2, 200, 1e-10)
    b = solve(5, 3, 130, 1e-2, 207, 1e-10)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and a[1:] == b[1:]


def test_fallbacks():
    n, D, B, lam = 5, 3, 130, 1e-2
    Q = problem(n, D, B)
    cores, idx = Q["cores"], Q["idx"]
    backend.mps_environments(cores, B)
    pre = CGFisherPreconditioner(damping=lam, max_iters=5, rel_tol=1e-6)
    # one NaN in g: info 1 and x = g bit for bit
    g = Q["g"].clone()
    g.view(-1)[17] = float('nan')
    x, info = pre.precondition(cores, idx, g)
    assert info.tolist() == [1] and pre.iters.tolist() == [0]
    assert np.array_equal(x.cpu().numpy().view(np.int64), g.cpu().numpy().view(np.int64))
    # g = 0: x = 0 is the solution, no iteration
    x, info = pre.precondition(cores, idx, torch.zeros_like(g))
    assert info.tolist() == [0] and pre.iters.tolist() == [0] and pre.relres.tolist() == [0.0]
    assert int(x.count_nonzero().item()) == 0
    # a huge damping: x = g / lam up to ||F^||_inf / lam, in one or two iterations
    big = 1e12
    pre = CGFisherPreconditioner(damping=big, max_iters=5, rel_tol=1e-10)
    x, info = pre.precondition(cores, idx, Q["g"])
    Fn = float(np.abs(Q["X64"] @ Q["X64"].T).sum(axis=1).max()) / B
    want = Q["gn"] / big
    err = np.abs(x.cpu().numpy().reshape(-1) - want).max()
    bound = 2 * Fn / big * np.abs(want).max() + 1e-10 * np.linalg.norm(Q["gn"]) / big
    print(f"lam = 1e12: {pre.iters.item()} iterations, |x - g / lam| = {err:.3e}, bound {bound:.3e}")
    assert info.tolist() == [0] and pre.iters.item() in (1, 2) and pre.relres.item() <= 1e-10 and err <= bound


def test_refused_arguments():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    buf = torch.zeros(1 << 12, dtype=torch.uint8, device=dev())
    p = buf.data_ptr()
    INVALID = -1
    for P in (0, -3, 1 << 31):
        assert lib.bornvi_cg_init(h.h, P, p, p, p, p, p, p, None) == INVALID
        assert lib.bornvi_cg_step(h.h, P, 1e-3, 1e-6, p, p, p, p, p, None) == INVALID
        assert lib.bornvi_cg_finish(h.h, P, p, p, p, p, p, p, None) == INVALID
    for lam in (0.0, -1e-3, float('nan'), float('inf')):
        assert lib.bornvi_cg_step(h.h, 8, lam, 1e-6, p, p, p, p, p, None) == INVALID
    for tol in (-1e-9, float('nan'), float('inf')):
        assert lib.bornvi_cg_step(h.h, 8, 1e-3, tol, p, p, p, p, p, None) == INVALID
    assert lib.bornvi_cg_init(h.h, 8, p, p, p, None, p, p, None) == INVALID
    assert lib.bornvi_cg_step(h.h, 8, 1e-3, 1e-6, None, p, p, p, p, None) == INVALID
    assert lib.bornvi_cg_finish(h.h, 8, p, p, p, p, None, p, None) == INVALID
    torch.cuda.synchronize()
    assert int(buf.count_nonzero().item()) == 0                                       # nothing was launched
    g = torch.ones(8, dtype=torch.float64, device=dev())
    x, r, pp, state, info = backend.cg_init(g)
    assert state.tolist()[:6] == [8.0, 8.0, 0.0, 0.0, 1.0, 0.0] and info.tolist() == [0]
    with pytest.raises(backend.BornviError):
        backend.cg_step(g, x, r, pp, state, 0.0)
    with pytest.raises(backend.BornviError):
        backend.cg_step(g, x, r, pp, state, 1e-3, rel_tol=-1.0)
    with pytest.raises(backend.BornviError):
        backend.cg_step(g[:4], x, r, pp, state, 1e-3)
    with pytest.raises(backend.BornviError):
        backend.cg_init(g.float())
    with pytest.raises(backend.BornviError):
        backend.cg_finish(g, x, state[:4])
    # F = 0: one step solves lam x = g exactly
    backend.cg_step(torch.zeros_like(g), x, r, pp, state, 0.5, 0.0)
    x, info, iters, relres = backend.cg_finish(g, x, state)
    assert x.tolist() == [2.0] * 8 and info.tolist() == [0] and iters.tolist() == [1] and relres.tolist() == [0.0]


def test_precondition_under_capture():
    """The whole precondition (cg_init, 40 x (jvp, vjp, cg_step), cg_finish) under torch.cuda.graph on a side stream, replayed
    twice: equal to the eager result bit for bit."""
    n, D, B, lam = 5, 3, 130, 1e-2
    Q = problem(n, D, B)
    cores, idx, g = Q["cores"], Q["idx"], Q["g"]
    pre = CGFisherPreconditioner(damping=lam, max_iters=40, rel_tol=1e-6)
    backend.mps_environments(cores, B)
    x, info = pre.precondition(cores, idx, g)
    eager = (x.clone(), info.clone(), pre.iters.clone(), pre.relres.clone(), pre.status.clone())
    assert eager[1].tolist() == [0] and 0 < int(eager[2].item()) <= 40
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # the side stream's workspaces exist before the capture
        backend.mps_environments(cores, B)
        pre.precondition(cores, idx, g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.mps_environments(cores, B)
        out, oinfo = pre.precondition(cores, idx, g)
    for _ in range(2):
        out.zero_()
        oinfo.fill_(-1)
        pre.iters.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        got = (out, oinfo, pre.iters, pre.relres, pre.status)
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
