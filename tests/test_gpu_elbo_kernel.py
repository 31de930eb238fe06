"""bornvi_elbo_weights against extended precision, per entry (hp_reference.py), and its contract: bitwise reproducible,
optional outputs, refused arguments, capturable.

Error bounds, derived (units of EPS64 = 2^-52; a correctly rounded operation errs by at most 1/2, the device's double
`log` by at most 1 ulp <= 1 unit of its result, as the HIP math API documents it):
  w_z = (l - log_p) + [q >= floor], l = log max(q, floor):  the log (1), the subtraction (1/2), the addition (1/2):
      |err| <= C_W eps (|l| + |log_p| + 1),  C_W = 2;
  a term q (l - log_p) of the loss: the log (1), the subtraction (1/2), the product (1/2) = C_W, relative to
      |q| (|l| + |log_p|) -- the term with its parts made absolute, since l - log_p may cancel (it does on the row
      q = p / sum p); a term q l of the entropy: 3/2 <= C_W, relative to |q| |l|;
  the sum: a thread adds at most 16 terms one after the other, a wave adds 6 butterfly levels, the workgroup its 4 wave
      totals, the finishing launch the same over the G <= 1024 partials -- never more roundings on a path than
      2 (ceil(log2 N) + C_TREE) with C_TREE = 1 for every n <= 22 (the worst case is n = 12: 16 + 6 + 3 = 25 additions),
      and a path cannot hold more additions than there are terms:
      |err| <= eps (C_W + ceil(log2 N) + C_TREE) sum |terms|.
Products with a q below 2^-1022 / |l - log_p| underflow: N units of the subnormal grid are added to the sum bounds.
The float64 mirror (elbo_mirror.py) is held to the same bounds on the same inputs, on the CPU."""
import math

import numpy as np
import pytest
import torch

import elbo_mirror as em
import hp_reference as hp

C_W = 2.0
C_TREE = 1.0
Q_FLOOR = 1e-10
SHAPES = [(n, rows) for n in (1, 3, 6, 8, 11, 14) for rows in (1, 3)]


def inputs(n, rows):
    """(q [rows, N], log_p [N]) float64.  log_p: the log of a random joint of evidence 0.37 with every seventh state at the
    1e-30 floor.  rows = 3: q = p / sum p (l - log_p cancels to -log sum p on every state above q_floor), the `onehot`
    family (every other entry 1e-30: below q_floor) and the `odd` family (exact zeros on the even states).  rows = 1: the
    `onehot` row with exact zeros on the states 2, 6, 10, ... (but the hot one)."""
    N = 1 << n
    rng = np.random.default_rng([n, 41])
    p = rng.dirichlet(np.ones(N)) * 0.37
    p[3::7] = 1e-30
    log_p = np.log(p)
    one = hp.qvec("onehot", n)
    if rows == 1:
        hot = int(np.argmax(one))
        one[2::4] = 0.0
        one[hot] = 1.0 - 1e-9
        return one[None, :].copy(), log_p
    return np.stack([p / p.sum(), one, hp.qvec("odd", n)]), log_p


def reference(q, log_p, X):
    """Extended precision: (w, w_bound, loss, loss_bound, entropy, entropy_bound) per row."""
    log = np.log if X.name == "longdouble" else np.frompyfunc(X.mp.log, 1, 1)
    ql, pl = X.arr(q), X.arr(log_p)
    l = log(np.where(q < Q_FLOOR, X.num(Q_FLOOR), ql))
    d = l - pl[None, :]
    w = d + X.arr((q >= Q_FLOOR).astype(np.float64))
    wb = np.abs(l) + np.abs(pl)[None, :] + X.num(1)
    zero = q == 0.0
    t_loss = np.where(zero, X.num(0), ql * d)
    t_ent = np.where(zero, X.num(0), ql * l)
    b_loss = np.abs(ql) * (np.abs(l) + np.abs(pl)[None, :])
    b_ent = np.abs(ql) * np.abs(l)
    return w, wb, t_loss.sum(axis=1), b_loss.sum(axis=1), -t_ent.sum(axis=1), b_ent.sum(axis=1)


def check(got, q, log_p, what):
    """Asserts (loss [rows], entropy [rows], w [rows, N]) against the reference; returns the worst ratios."""
    X = hp.arithmetic()
    n = int(log_p.size).bit_length() - 1
    if hp.unavailable(n, X):
        pytest.skip(hp.unavailable(n, X))
    loss, ent, w = got
    w_ref, w_b, l_ref, l_b, e_ref, e_b = reference(q, log_p, X)
    c_sum = C_W + math.ceil(math.log2(log_p.size)) + C_TREE
    floor = log_p.size * hp.TINY64
    r_w = hp.worst(hp.ratio(w, w_ref, w_b, X=X))
    r_l = hp.worst(hp.ratio(loss, l_ref, l_b, floor, X=X))
    r_e = hp.worst(hp.ratio(ent, e_ref, e_b, floor, X=X))
    print(f"{what} n={n} rows={q.shape[0]}: w {r_w[0]:.3f}/{C_W} loss {r_l[0]:.3f}/{c_sum} entropy {r_e[0]:.3f}/{c_sum}")
    assert r_w[0] <= C_W, (what, "w", r_w)
    assert r_l[0] <= c_sum, (what, "loss", r_l)
    assert r_e[0] <= c_sum, (what, "entropy", r_e)
    return r_w[0], r_l[0], r_e[0]


@pytest.mark.parametrize("n,rows", SHAPES)
def test_inputs_hold_what_they_are_for(n, rows):
    q, log_p = inputs(n, rows)
    assert np.isfinite(log_p).all() and (q == 0.0).any() == (n > 1 or rows == 3)
    assert ((q > 0) & (q < Q_FLOOR)).any() and (q >= Q_FLOOR).any()
    if rows == 3:
        loss, _, _ = em.weights(q[0], log_p)
        # the cancelling row: every term above q_floor is q (log q - log p) = -q log sum p; the others weigh < 1e-27 each
        assert abs(loss + math.log(np.exp(log_p).sum())) < 1e-11


@pytest.mark.parametrize("n,rows", SHAPES)
def test_mirror_is_inside_the_bounds(n, rows):
    """The float64 mirror on the CPU, same inputs, same bounds (NumPy's pairwise sum and glibc's log)."""
    q, log_p = inputs(n, rows)
    m = [em.weights(r, log_p) for r in q]
    check((np.array([v[0] for v in m]), np.array([v[1] for v in m]), np.stack([v[2] for v in m])), q, log_p, "mirror")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def run(q, log_p, dev, **kw):
    from tensornetworks_amd import backend
    return backend.elbo_weights(torch.from_numpy(q).to(dev), torch.from_numpy(log_p).to(dev), Q_FLOOR, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("n,rows", SHAPES)
def test_kernel_against_extended_precision(dev, n, rows):
    q, log_p = inputs(n, rows)
    loss, ent, w = run(q, log_p, dev)
    assert loss.shape == (rows,) and ent.shape == (rows,) and w.shape == q.shape
    check((loss.cpu().numpy(), ent.cpu().numpy(), w.cpu().numpy()), q, log_p, "kernel")
    # a term with q == 0 is exactly 0 whatever log_p holds there; elsewhere a non-finite log_p reaches the loss
    z = np.flatnonzero(q[-1] == 0.0)
    if len(z):
        bad = log_p.copy()
        bad[z[0]] = -np.inf
        loss_b, ent_b, _ = run(q[-1:], bad, dev)
        loss_1, ent_1, _ = run(q[-1:], log_p, dev)
        assert torch.equal(loss_b, loss_1) and torch.equal(ent_b, ent_1)
    bad = log_p.copy()
    bad[int(np.flatnonzero(q[-1] != 0.0)[0])] = np.nan
    loss_b, ent_b, _ = run(q[-1:], bad, dev)
    assert torch.isnan(loss_b).all() and torch.isfinite(ent_b).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,rows", SHAPES)
def test_two_calls_are_bitwise_equal_and_outputs_are_optional(dev, n, rows):
    q, log_p = inputs(n, rows)
    a, b = run(q, log_p, dev), run(q, log_p, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    loss, ent, w = run(q, log_p, dev, want_w=False)
    assert w is None and torch.equal(loss, a[0]) and torch.equal(ent, a[1])
    loss, ent, w = run(q, log_p, dev, want_entropy=False)
    assert ent is None and torch.equal(loss, a[0]) and torch.equal(w, a[2])
    out = torch.empty(q.shape, dtype=torch.float64, device=dev)
    assert run(q, log_p, dev, out=out)[2] is out and torch.equal(out, a[2])
    # an unaligned view (the scalar path) computes the same entries
    N = log_p.size
    buf_q = torch.zeros(rows * N + 1, dtype=torch.float64, device=dev)
    buf_q[1:] = torch.from_numpy(q).to(dev).reshape(-1)
    from tensornetworks_amd import backend
    c = backend.elbo_weights(buf_q[1:].view(rows, N), torch.from_numpy(log_p).to(dev), Q_FLOOR)
    assert torch.equal(c[2], a[2])
    torch.testing.assert_close(c[0], a[0], rtol=1e-13, atol=1e-300)


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(dev):
    import ctypes as C
    from tensornetworks_amd import _ext, backend
    h = _ext.handle_for(dev)
    n = 3
    q = torch.full((8,), 0.125, dtype=torch.float64, device=dev)
    log_p = torch.zeros(8, dtype=torch.float64, device=dev)
    w = torch.full((8,), 7.0, dtype=torch.float64, device=dev)
    loss = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(h.size("bornvi_elbo_workspace_bytes", n, 1), dtype=torch.uint8, device=dev)
    lib = _ext.lib()

    def call(n_, rows, floor, q_=q, lp=log_p, loss_=loss, ws_=ws, ws_bytes=None):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return lib.bornvi_elbo_weights(h.h, n_, rows, p(q_), p(lp), floor, p(w), p(loss_), None, p(ws_),
                                       ws_.numel() if ws_bytes is None else ws_bytes, _ext.stream_ptr(dev))
    INVALID, WORKSPACE = -1, -3
    assert call(n, 0, Q_FLOOR) == INVALID and call(n, 65536, Q_FLOOR) == INVALID and call(n, -1, Q_FLOOR) == INVALID
    assert call(n, 1, 0.0) == INVALID and call(n, 1, -1e-10) == INVALID and call(n, 1, float("nan")) == INVALID
    assert call(31, 1, Q_FLOOR) == INVALID and call(0, 1, Q_FLOOR) == INVALID
    assert call(n, 1, Q_FLOOR, q_=None) == INVALID and call(n, 1, Q_FLOOR, lp=None) == INVALID
    assert call(n, 1, Q_FLOOR, loss_=None) == INVALID
    assert call(n, 1, Q_FLOOR, ws_bytes=8) == WORKSPACE
    assert lib.bornvi_elbo_workspace_bytes(h.h, 31, 1) == 0 and lib.bornvi_elbo_workspace_bytes(h.h, n, 0) == 0
    torch.cuda.synchronize()
    assert bool((w == 7.0).all()) and float(loss) == 7.0             # nothing ran
    assert call(n, 1, Q_FLOOR) == 0
    torch.cuda.synchronize()
    assert abs(float(loss) - math.log(0.125)) < 1e-15
    with pytest.raises(backend.BornviError):
        backend.elbo_weights(q.float(), log_p)
    with pytest.raises(backend.BornviError):
        backend.elbo_weights(q, log_p.cpu())


@pytest.mark.gpu
def test_capture_and_replay(dev):
    """The call inside a torch.cuda.graph capture at n = 8; the replay's outputs are the eager call's bits."""
    q, log_p = inputs(8, 3)
    eager = run(q, log_p, dev)                      # (also sizes the workspace of this stream)
    qd, pd = torch.from_numpy(q).to(dev), torch.from_numpy(log_p).to(dev)
    from tensornetworks_amd import backend
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        backend.elbo_weights(qd, pd, Q_FLOOR)       # the side stream's workspace exists before the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = backend.elbo_weights(qd, pd, Q_FLOOR)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    qd.copy_(torch.from_numpy(q[[1, 2, 0]]).to(dev))           # the replay reads the inputs' current values
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0], eager[0][[1, 2, 0]]) and torch.equal(out[2], eager[2][[1, 2, 0]])
