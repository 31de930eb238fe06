"""bornvi_mps_score_rows / bornvi_score_fisher_gram / bornvi_spd_solve_batched against the extended-precision mirror
(sampled_fisher_mirror.py), per entry the hp_reference.ratio way, and their contract: exact zeros, padded columns, a site
sub-range bit for bit, the status word, F == F^T, bitwise reproducible, site blocks = diagonal blocks, a batched system =
the single solve bit for bit, capturable, chunking.

Shapes: rows n in {1, 2, 3, 63}, D in {1, 2, 3, 5, 16, 17, 22} (every DP template and the 16 / 17 edge), B in {2, 63, 64, 65,
130} and one B = 16384 + 65 whose workgroups walk more than one tile; Gram R in {2, 8, 32, 50, 65, 968} (both sides of the
64-row tile edge), nblocks in {1, 3}, ld in {64, 256, 512, 8192} (one slab, several slabs, several groups); solve P in
{1, 17, 288}.

Error bounds (units of EPS64 = 2^-52, every rounding a whole unit, derived in sampled_fisher_mirror: c_rows, c_gram):
  a score-row entry against its absolute-term value: 1 + max((n - 1) D + (n D + 2) kappa_b + 3,
                                                              (n - 1)(3 D + 1) + 2 D + n (3 D + 1) kappa_Z + 2);
  a Gram entry against sum_b |o_a| |o_b| / B of the rows it was given: slab + per_wg + G + 1.
The constants are not fitted: each test prints the worst ratio beside its C."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_sampled_mirror as sm
import sampled_fisher_mirror as fm
from tensornetworks_amd import backend
from tensornetworks_amd.backend import mps_score_rows, score_fisher_gram, spd_solve_batched  # noqa: F401  (fails without the feature)
from tensornetworks_amd.natural_gradient import SampledFisherPreconditioner
from test_gpu_mps_sampled_kernel import c_score, make_cores

pytestmark = pytest.mark.gpu
EPS = hp.EPS64

ROWS_CASES = [(1, 1, 2), (1, 3, 63), (2, 2, 64), (3, 5, 65), (3, 16, 130), (2, 17, 65), (3, 22, 64), (63, 2, 130), (63, 16, 63),
              (63, 22, 2), (63, 3, 65), (3, 2, 16384 + 65)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def rows_inputs(n, D, B):
    rng = np.random.default_rng([n, D, B, 9])
    bits = rng.integers(0, 2, size=(B, n))
    bits[0] = 0
    bits[-1] = 1
    if B > 8:
        bits[3] = bits[5] = bits[B // 2]           # repeated samples
    return bits


@pytest.mark.parametrize("n,D,B", ROWS_CASES)
def test_score_rows_against_the_mirror(n, D, B):
    cores = make_cores(n, D, seed=4)
    bits = rows_inputs(n, D, B)
    idx = torch.from_numpy(sm.idx_of_bits(bits)).to(dev())
    c = cores.to(dev())
    backend.mps_environments(c, B)
    rows, status = backend.mps_score_rows(c, idx)
    rows2, _ = backend.mps_score_rows(c, idx)
    ld, R = backend.score_rows_ld(B), 2 * D * D
    assert tuple(rows.shape) == (n, R, ld) and ld >= max(B, 64) and ld & (ld - 1) == 0 and ld < 2 * max(B, 64)
    assert torch.equal(rows, rows2) and int(status.item()) == 0
    got = rows.cpu().numpy()
    assert np.all(got[:, :, B:] == 0.0)                                              # padded columns
    env = sm.environments(cores.numpy())
    ref = fm.score_rows(cores.numpy(), bits, env)
    kZ = float(env["Z_abs"] / env["Z"])
    C = fm.c_rows(n, D, hp.to_f64(ref["kappa"]), kZ)                                 # [B]: per sample
    r = hp.ratio(got[:, :, :B], ref["rows"], ref["rows_abs"], X=hp._LongDouble) / C[None, None, :]
    w, at = hp.worst(r)
    print(f"n={n} D={D} B={B}: worst rows error / (C EPS rows_abs) = {w:.3f} at {at}, C up to {C.max():.0f} "
          f"(kappa_max {float(ref['kappa'].max()):.2f}, kappa_Z {kZ:.2f})")
    assert w <= 1.0
    g5 = got.reshape(n, 2, D, D, ld)
    if D > 1:
        assert np.all(g5[0][:, 1:, :, :] == 0.0) and np.all(g5[n - 1][:, :, 1:, :] == 0.0)   # the boundary cores
    # a sub-range of sites is the same slice, bit for bit
    k0, cnt = (n // 2, max(1, n // 4)) if n > 1 else (0, 1)
    sub, st = backend.mps_score_rows(c, idx, k0, cnt)
    assert tuple(sub.shape) == (cnt, R, ld) and torch.equal(sub, rows[k0:k0 + cnt]) and int(st.item()) == 0
    if n > 1:
        last, _ = backend.mps_score_rows(c, idx, n - 1, 1)
        assert torch.equal(last[0], rows[n - 1])


@pytest.mark.parametrize("n,D,B", [(3, 5, 65), (63, 3, 65), (3, 2, 16384 + 65)])
def test_score_rows_contract_to_the_score_vjp(n, D, B):
    """sum_b w_b o_b (in extended precision, from the GPU's rows) against bornvi_mps_score_vjp, within the sum of both
    bounds, for a w with sum w = 0 up to rounding: the two differ by -(sum w) mu, which is added to the bound."""
    cores = make_cores(n, D, seed=4)
    bits = rows_inputs(n, D, B)
    w = np.random.default_rng([n, D, B]).standard_normal(B)
    w -= w.mean()
    idx = torch.from_numpy(sm.idx_of_bits(bits)).to(dev())
    c = cores.to(dev())
    backend.mps_environments(c, B)
    grad, _, _ = backend.mps_score_vjp(c, idx, torch.from_numpy(w).to(dev()))
    rows, _ = backend.mps_score_rows(c, idx)
    env = sm.environments(cores.numpy())
    ref = sm.score_gradient(cores.numpy(), bits, w, env)
    rr = fm.score_rows(cores.numpy(), bits, env)
    kZ = float(env["Z_abs"] / env["Z"])
    wl = w.astype(sm.LD)
    contracted = (rows.cpu().numpy()[:, :, :B].astype(sm.LD) * wl[None, None, :]).sum(axis=2).reshape(cores.shape)
    Cr = fm.c_rows(n, D, hp.to_f64(rr["kappa"]), kZ)
    bound = EPS * (c_score(n, D, B, float(ref["kappa"].max()), kZ) * ref["grad_abs"]
                   + (rr["rows_abs"] * (np.abs(wl) * Cr)[None, None, :]).sum(axis=2).reshape(cores.shape)) \
        + abs(wl.sum()) * rr["mu_abs"]
    err = np.abs(contracted - grad.cpu().numpy().astype(sm.LD))
    worst = float(np.max(hp.to_f64(err / np.where(bound > 0, bound, 1))))
    print(f"n={n} D={D} B={B}: worst |rows w - score_vjp| / bound = {worst:.3f}")
    assert np.all(err <= bound)


def test_score_rows_zero_amplitude():
    """A sample with psi = 0: an all-zero column and status 2; the other columns against the mirror."""
    n, D = 4, 2
    cores = make_cores(n, D, seed=2)
    cores[1, 1] = 0.0                                   # every z with z_2 = 1 has psi = 0
    bits = np.array([[0, 0, 1, 0], [0, 1, 0, 1], [1, 0, 0, 1]])
    c = cores.to(dev())
    backend.mps_environments(c, 3)
    rows, status = backend.mps_score_rows(c, torch.from_numpy(sm.idx_of_bits(bits)).to(dev()))
    got = rows.cpu().numpy()
    assert int(status.item()) == 2 and np.all(got[:, :, 1] == 0.0) and np.any(got[:, :, 0] != 0.0) and np.any(got[:, :, 2] != 0.0)
    env = sm.environments(cores.numpy())
    ref = fm.score_rows(cores.numpy(), bits, env)
    assert np.all(ref["rows"][:, :, 1] == 0)
    C = fm.c_rows(n, D, np.where(np.isfinite(hp.to_f64(ref["kappa"])), hp.to_f64(ref["kappa"]), 1.0), float(env["Z_abs"] / env["Z"]))
    r = hp.ratio(got[:, :, :3], ref["rows"], ref["rows_abs"], X=hp._LongDouble) / C[None, None, :]
    assert hp.worst(r)[0] <= 1.0


# ------------------------------------------------------------------------------------------------------------ Gram
GRAM_CASES = [(2, 1, 64, 2), (8, 3, 256, 130), (32, 3, 512, 512), (50, 1, 8192, 8000), (65, 3, 64, 63), (65, 1, 8192, 8192),
              (968, 1, 64, 64)]


def gram_rows(R, nb, ld, B):
    rng = np.random.default_rng([R, nb, ld, B])
    X = rng.standard_normal((nb, R, ld)) * 10.0 ** rng.uniform(-3, 3, (nb, R, 1))      # rows of very different sizes
    X[:, :, B:] = 0.0
    if R > 3:
        X[:, 3, :] = 0.0                                                                # an all-zero row (a boundary entry)
    return X


@pytest.mark.parametrize("R,nb,ld,B", GRAM_CASES)
def test_score_fisher_gram_against_the_mirror(R, nb, ld, B):
    X = gram_rows(R, nb, ld, B)
    Xd = torch.from_numpy(X).to(dev())
    F = backend.score_fisher_gram(Xd, B)
    F2 = backend.score_fisher_gram(Xd, B)
    assert tuple(F.shape) == (nb, R, R) and torch.equal(F, F2)                          # bitwise reproducible
    assert torch.equal(F, F.transpose(1, 2))                                            # F == F^T bitwise
    got = F.cpu().numpy()
    assert np.all(np.diagonal(got, axis1=1, axis2=2) >= 0.0)
    C = fm.c_gram(ld)
    worst = 0.0
    for j in range(nb):
        Xl = X[j].astype(sm.LD)
        ref, mag = Xl @ Xl.T / sm.LD(B), np.abs(Xl) @ np.abs(Xl).T / sm.LD(B)
        w, at = hp.worst(hp.ratio(got[j], ref, mag, X=hp._LongDouble))
        worst = max(worst, w)
        if R > 3:
            assert np.all(got[j][3] == 0.0) and np.all(got[j][:, 3] == 0.0)
    print(f"R={R} nblocks={nb} ld={ld} B={B}: worst Gram ratio {worst:.2f}, C_GRAM = {C:.0f} {hp.syrk_geometry(ld)}")
    assert worst <= C


@pytest.mark.parametrize("D,n,B", [(2, 3, 130), (4, 3, 512), (5, 2, 65)])
def test_site_blocks_equal_the_diagonal_blocks_of_the_whole(D, n, B):
    """R = 2 D^2 = 8, 32, 50 with 3, 3, 2 blocks: the whole matrix has 24, 96, 100 rows (the last two cross a tile edge).  An
    entry's order of summation depends on ld only, so on this build the site blocks are the diagonal blocks BIT FOR BIT;
    the Gram bound is asserted as well."""
    cores = make_cores(n, D, seed=6)
    bits = rows_inputs(n, D, B)
    idx = torch.from_numpy(sm.idx_of_bits(bits)).to(dev())
    c = cores.to(dev())
    backend.mps_environments(c, B)
    rows, _ = backend.mps_score_rows(c, idx)
    R, ld = 2 * D * D, rows.shape[2]
    site = backend.score_fisher_gram(rows, B)
    full = backend.score_fisher_gram(rows.reshape(1, n * R, ld), B)[0]
    Xl = rows.cpu().numpy().astype(sm.LD).reshape(n * R, ld)
    ref, mag = Xl @ Xl.T / sm.LD(B), np.abs(Xl) @ np.abs(Xl).T / sm.LD(B)
    assert hp.worst(hp.ratio(full.cpu().numpy(), ref, mag, X=hp._LongDouble))[0] <= fm.c_gram(ld)
    for k in range(n):
        blk = full[k * R:(k + 1) * R, k * R:(k + 1) * R]
        assert hp.worst(hp.ratio(site[k].cpu().numpy(), ref[k * R:(k + 1) * R, k * R:(k + 1) * R],
                                 mag[k * R:(k + 1) * R, k * R:(k + 1) * R], X=hp._LongDouble))[0] <= fm.c_gram(ld)
        assert torch.equal(site[k], blk)
    # and against the mirror's own rows: the rows' error enters twice, the Gram's once
    env = sm.environments(cores.numpy())
    mr = fm.score_rows(cores.numpy(), bits, env)
    Fm = fm.fisher(mr["rows"], B, mr["rows_abs"])
    Cr = float(fm.c_rows(n, D, hp.to_f64(mr["kappa"]), float(env["Z_abs"] / env["Z"])).max())
    w, at = hp.worst(hp.ratio(full.cpu().numpy(), Fm["full"], Fm["full_abs"], X=hp._LongDouble))
    print(f"D={D} n={n} B={B}: worst F^ error against the mirror / (EPS sum |o||o| / B) = {w:.2f}, C = {2 * Cr + 1 + fm.c_gram(ld):.0f}")
    assert w <= 2 * Cr + 1 + fm.c_gram(ld)


# ------------------------------------------------------------------------------------------------------------ batched solve
def spd_systems(P, nb, seed):
    rng = np.random.default_rng([P, nb, seed])
    M = rng.standard_normal((nb, P, P + 3))
    A = M @ M.transpose(0, 2, 1) / (P + 3) + 0.1 * np.eye(P)[None]
    A = 0.5 * (A + A.transpose(0, 2, 1))
    return A, rng.standard_normal((nb, P))


@pytest.mark.parametrize("P", [1, 17, 288])
def test_batched_solve_is_the_single_solve(P):
    nb = 3
    A, b = spd_systems(P, nb, 0)
    Ad, bd = torch.from_numpy(A).to(dev()), torch.from_numpy(b).to(dev())
    x, info = backend.spd_solve_batched(Ad, bd, 1e-3)
    x2, info2 = backend.spd_solve_batched(Ad, bd, 1e-3)
    assert torch.equal(x, x2) and torch.equal(info, info2) and info.tolist() == [0, 0, 0]
    for j in range(nb):
        xs, infos = backend.spd_solve(Ad[j], bd[j], 1e-3)
        assert torch.equal(xs, x[j]) and int(infos.item()) == 0
        resid = (A[j] + 1e-3 * np.eye(P)) @ x[j].cpu().numpy() - b[j]
        assert np.abs(resid).max() <= 1e-9 * max(1.0, np.abs(b[j]).max())
    # the middle system indefinite at pivot p: its own info = p + 1 and x = b bit for bit; the neighbours are solved
    p = P // 2
    Ai = A.copy()
    Ai[1, p, p] = -5.0
    Aid = torch.from_numpy(Ai).to(dev())
    xi, infoi = backend.spd_solve_batched(Aid, bd, 1e-3)
    assert infoi.tolist() == [0, p + 1, 0]
    assert torch.equal(xi[1], bd[1]) and torch.equal(xi[0], x[0]) and torch.equal(xi[2], x[2])
    xs, infos = backend.spd_solve(Aid[1], bd[1], 1e-3)
    assert int(infos.item()) == p + 1 and torch.equal(xs, xi[1])
    # a NaN in one b: info = P + 1 for that system only
    bn = b.copy()
    bn[2, P - 1] = np.nan
    bnd = torch.from_numpy(bn).to(dev())
    xn, infon = backend.spd_solve_batched(Ad, bnd, 1e-3)
    assert infon.tolist() == [0, 0, P + 1]
    assert torch.equal(xn[0], x[0]) and torch.equal(xn[1], x[1])
    assert np.array_equal(xn[2].cpu().numpy().view(np.int64), bn[2].view(np.int64))


def test_refused_sizes():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    p = buf.data_ptr()
    UNSUPPORTED = -4
    assert lib.bornvi_score_fisher_workspace_bytes(h.h, 1025, 1, 64) == 0 and lib.bornvi_score_fisher_workspace_bytes(h.h, 8, 1, 96) == 0
    assert lib.bornvi_score_fisher_workspace_bytes(h.h, 8, 0, 64) == 0 and lib.bornvi_score_fisher_workspace_bytes(h.h, 8, 1, 32) == 0
    assert lib.bornvi_spd_solve_batched_workspace_bytes(h.h, 1025, 1) == 0 and lib.bornvi_spd_solve_batched_workspace_bytes(h.h, 8, 0) == 0
    assert lib.bornvi_score_fisher_gram(h.h, 1026, 1, 64, 64, p, p, p, buf.numel(), None) == UNSUPPORTED
    assert lib.bornvi_score_fisher_gram(h.h, 8, 1, 1, 64, p, p, p, buf.numel(), None) == UNSUPPORTED          # B = 1
    assert lib.bornvi_score_fisher_gram(h.h, 8, 1, 65, 64, p, p, p, buf.numel(), None) == UNSUPPORTED         # B > ld
    assert lib.bornvi_mps_score_rows(h.h, 64, 4, 8, p, p, 0, 1, 64, p, p, p, buf.numel(), None) == UNSUPPORTED
    assert lib.bornvi_mps_score_rows(h.h, 8, 4, 1, p, p, 0, 1, 64, p, p, p, buf.numel(), None) == UNSUPPORTED  # B = 1
    assert lib.bornvi_mps_score_rows(h.h, 8, 4, 8, p, p, 0, 1, 96, p, p, p, buf.numel(), None) == UNSUPPORTED  # ld
    assert lib.bornvi_spd_solve_batched(h.h, 1025, 1, p, 0.0, p, p, p, p, buf.numel(), None) == UNSUPPORTED
    with pytest.raises(backend.BornviError):
        backend.mps_score_rows(make_cores(3, 2).to(dev()), torch.zeros(1, dtype=torch.int64, device=dev()))
    with pytest.raises(backend.BornviError):
        backend.score_fisher_gram(torch.zeros(1, 8, 96, dtype=torch.float64, device=dev()), 64)


# ------------------------------------------------------------------------------------------------------------ preconditioner
def precondition_inputs(n, D, B, seed):
    cores = make_cores(n, D, seed=seed).to(dev())
    idx = torch.from_numpy(sm.idx_of_bits(rows_inputs(n, D, B))).to(dev())
    grad = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 2, D, D))).to(dev())
    return cores, idx, grad


@pytest.mark.parametrize("blocks", ["site", "full"])
def test_precondition_against_the_mirror_and_under_capture(blocks):
    """delta against the mirror's solve in extended precision (loosely: the solve amplifies rounding by at most
    (||F^|| + damping) / damping), then the same call under torch.cuda.graph on one stream, replayed twice: equal to the
    eager result bit for bit."""
    n, D, B, lam = 5, 3, 130, 1e-3
    cores, idx, grad = precondition_inputs(n, D, B, 8)
    pre = SampledFisherPreconditioner(damping=lam, blocks=blocks)
    backend.mps_environments(cores, B)
    delta, info = pre.precondition(cores, idx, grad)
    eager, einfo = delta.clone(), info.clone()
    assert tuple(eager.shape) == tuple(cores.shape) and einfo.tolist() == [0] * (n if blocks == "site" else 1)
    assert int(pre.status.item()) == 0
    ref, rinfo = fm.precondition(cores.cpu().numpy(), sm.bits_of_idx(idx.cpu().numpy(), n), grad.cpu().numpy(), lam, blocks)
    F = fm.fisher(fm.score_rows(cores.cpu().numpy(), sm.bits_of_idx(idx.cpu().numpy(), n))["rows"])
    amp = (float(np.abs(F["full"]).sum(axis=1).max()) + lam) / lam
    err = np.abs(eager.cpu().numpy() - hp.to_f64(ref)).max() / np.abs(hp.to_f64(ref)).max()
    print(f"blocks={blocks}: relative error of delta {err:.3e}, amplification bound {amp:.3e}")
    assert np.all(rinfo == 0) and err <= 1e3 * EPS * amp
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # the side stream's workspaces exist before the capture
        backend.mps_environments(cores, B)
        pre.precondition(cores, idx, grad)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.mps_environments(cores, B)
        out, oinfo = pre.precondition(cores, idx, grad)
    for _ in range(2):
        out.zero_()
        oinfo.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(oinfo, einfo)


def test_chunks_do_not_change_the_bits():
    """A budget that holds one site's rows: n chunks of one site give the same delta as one chunk, bit for bit."""
    n, D, B = 6, 4, 257
    cores, idx, grad = precondition_inputs(n, D, B, 9)
    backend.mps_environments(cores, B)
    one = SampledFisherPreconditioner(damping=1e-2)
    assert one.plan(n, D, B)[2] == n
    d1, i1 = one.precondition(cores, idx, grad)
    d1, i1 = d1.clone(), i1.clone()
    site_bytes = 2 * D * D * backend.score_rows_ld(B) * 8
    many = SampledFisherPreconditioner(damping=1e-2, rows_budget_bytes=site_bytes)
    assert many.plan(n, D, B)[2] == 1
    d2, i2 = many.precondition(cores, idx, grad)
    assert torch.equal(d1, d2) and torch.equal(i1, i2) and i1.tolist() == [0] * n
    assert many._rows.shape[0] == 1 and int(many.status.item()) == 0
    with pytest.raises(ValueError, match="rows of one site"):
        SampledFisherPreconditioner(rows_budget_bytes=site_bytes - 1).precondition(cores, idx, grad)
