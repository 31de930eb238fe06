"""bornvi_mps_score_jvp against the extended-precision mirror (cg_natgrad_mirror.py on sampled_fisher_mirror.py), per entry the
hp_reference.ratio way, and the call's contract: bitwise reproducible, an entry independent of B and of its tile, exact
scaling and zeros, the gauge direction, adjoint to bornvi_mps_score_vjp, a dead sample, the refused sizes, capturable.

Error bound of one t_b (units of EPS64 = 2^-52 on t_abs = rows_abs . |v|, every rounding a whole unit, derived in
cg_natgrad_mirror.c_jvp): 2 + max(2 n D + (n D + 2) kappa_b + 1, the mu entry's constant + 2 D^2 + n).  The constant is not
fitted: each test prints the worst ratio beside its C."""
import functools

import numpy as np
import pytest
import torch

import cg_natgrad_mirror as cm
import hp_reference as hp
import mps_sampled_mirror as sm
from tensornetworks_amd import backend
from tensornetworks_amd.backend import mps_score_jvp  # noqa: F401  (fails without the feature)
from test_gpu_mps_sampled_kernel import c_score, make_cores
from test_gpu_sampled_natgrad_kernel import rows_inputs

pytestmark = pytest.mark.gpu
EPS = hp.EPS64

# the last case is past 256 x 64 samples: a workgroup walks two tiles
CASES = [(1, 1, 2), (3, 2, 64), (3, 2, 65), (5, 3, 130), (4, 5, 257), (6, 16, 192), (2, 32, 64), (63, 4, 128), (3, 2, 16449)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def direction(n, D, seed=0):
    return torch.from_numpy(np.random.default_rng([n, D, seed, 31]).standard_normal((n, 2, D, D)))


def jvp_on_device(cores, bits, v, scale=1.0):
    B = bits.shape[0]
    idx = torch.from_numpy(sm.idx_of_bits(bits)).to(dev())
    c = cores.to(dev())
    backend.mps_environments(c, B)
    t, status = backend.mps_score_jvp(c, idx, v.to(dev()), scale)
    return c, idx, t, status


@functools.lru_cache(maxsize=None)
def reference(n, D, B, seed=4):
    """The case's inputs and the mirror's rows, computed once and shared."""
    cores = make_cores(n, D, seed=seed)
    bits = rows_inputs(n, D, B)
    env = sm.environments(cores.numpy())
    v = direction(n, D)
    ref = cm.jvp(cores.numpy(), bits, v.numpy(), env)
    kZ = float(env["Z_abs"] / env["Z"])
    C = cm.c_jvp(n, D, hp.to_f64(ref["sr"]["kappa"]), kZ)
    return dict(cores=cores, bits=bits, v=v, ref=ref, kZ=kZ, C=C)


@pytest.mark.parametrize("n,D,B", CASES)
def test_score_jvp_against_the_mirror(n, D, B):
    R = reference(n, D, B)
    cores, bits, v, ref, C = R["cores"], R["bits"], R["v"], R["ref"], R["C"]
    c, idx, t, status = jvp_on_device(cores, bits, v)
    t2, _ = backend.mps_score_jvp(c, idx, v.to(dev()))
    assert tuple(t.shape) == (B,) and int(status.item()) == 0
    assert torch.equal(t, t2)                                                        # bitwise reproducible
    got = t.cpu().numpy()
    r = hp.ratio(got, ref["t"], ref["t_abs"], X=hp._LongDouble) / C
    w, at = hp.worst(r)
    print(f"n={n} D={D} B={B}: worst t error / (C EPS t_abs) = {w:.4f} at {at}, C up to {C.max():.0f} "
          f"(kappa_max {float(ref['sr']['kappa'].max()):.2f}, kappa_Z {R['kZ']:.2f})")
    assert w <= 1.0
    if B > 8:                                                                        # rows_inputs repeats sample B // 2 at 3 and 5
        assert got[3] == got[5] == got[B // 2]
    # scale = 0.5 halves every entry exactly; v = 0 gives exact zeros
    half, _ = backend.mps_score_jvp(c, idx, v.to(dev()), 0.5)
    assert np.array_equal(half.cpu().numpy(), 0.5 * got)
    zero, st = backend.mps_score_jvp(c, idx, torch.zeros_like(c))
    assert np.all(zero.cpu().numpy() == 0.0) and int(st.item()) == 0
    # v = cores is the gauge direction: q is invariant under a common scale of the cores, so t = 0 up to the bound
    gauge, _ = backend.mps_score_jvp(c, idx, c)
    gref = cm.jvp(cores.numpy(), bits, cores.numpy(), sr=ref["sr"])
    rg = np.abs(gauge.cpu().numpy()) / (EPS * hp.to_f64(gref["t_abs"]) * C)
    print(f"  gauge direction: worst |t| / (C EPS t_abs) = {rg.max():.4f} (t_abs up to {float(gref['t_abs'].max()):.1f})")
    assert rg.max() <= 1.0


def test_an_entry_does_not_depend_on_the_batch_or_the_tile():
    """The first 64 entries of a B = 130 call against a B = 64 call on those samples: another grid, other tiles, the same
    bits."""
    n, D = 5, 3
    cores = make_cores(n, D, seed=4)
    bits = rows_inputs(n, D, 130)
    v = direction(n, D)
    _, _, t130, _ = jvp_on_device(cores, bits, v)
    _, _, t64, _ = jvp_on_device(cores, bits[:64].copy(), v)
    assert torch.equal(t130[:64], t64)
    # and across the tiles of one workgroup: sample 16448 of the two-tile case alone with one other sample
    bits2 = rows_inputs(3, 2, 16449)
    c2, v2 = make_cores(3, 2, seed=4), direction(3, 2)
    _, _, big, _ = jvp_on_device(c2, bits2, v2)
    _, _, small, _ = jvp_on_device(c2, bits2[[16448, 7]].copy(), v2)
    assert torch.equal(big[[16448, 7]], small)


@pytest.mark.parametrize("n,D,B", [(5, 3, 130), (63, 4, 128), (3, 2, 16449)])
def test_score_jvp_is_the_adjoint_of_the_score_vjp(n, D, B):
    """<t, w> with t = jvp(v) against <v, mps_score_vjp(w)> for a random w, both dot products formed in extended precision from
    the device's outputs: within the sum of the two calls' bounds, sum_b |w_b| C_jvp EPS t_abs_b + sum_i |v_i| C_SCORE EPS
    grad_abs_i."""
    R = reference(n, D, B)
    cores, bits, v, ref = R["cores"], R["bits"], R["v"], R["ref"]
    w = np.random.default_rng([n, D, B, 2]).standard_normal(B)
    c, idx, t, _ = jvp_on_device(cores, bits, v)
    grad, _, _ = backend.mps_score_vjp(c, idx, torch.from_numpy(w).to(dev()))
    LD = sm.LD
    lhs = (t.cpu().numpy().astype(LD) * w.astype(LD)).sum()
    rhs = (grad.cpu().numpy().astype(LD) * v.numpy().astype(LD)).sum()
    sg = sm.score_gradient(cores.numpy(), bits, w)
    Cs = c_score(n, D, B, float(sg["kappa"].max()), R["kZ"])
    bound = EPS * ((np.abs(w).astype(LD) * R["C"] * ref["t_abs"]).sum() + Cs * (np.abs(v.numpy()).astype(LD) * sg["grad_abs"]).sum())
    print(f"n={n} D={D} B={B}: |<t, w> - <v, vjp(w)>| = {float(abs(lhs - rhs)):.3e}, bound {float(bound):.3e} "
          f"(<t, w> = {float(lhs):.6f})")
    assert abs(lhs - rhs) <= bound


def test_score_jvp_zero_amplitude():
    """A sample with psi = 0 (built as test_sample_gram_zero_amplitude builds it): t_b = 0.0 exactly and status 2; every other
    entry within its bound."""
    n, D = 4, 2
    cores = make_cores(n, D, seed=2)
    cores[1, 1] = 0.0                                   # every z with z_2 = 1 has psi = 0
    bits = np.array([[0, 0, 1, 0], [0, 1, 0, 1], [1, 0, 0, 1], [0, 0, 1, 1]])
    v = direction(n, D)
    _, _, t, status = jvp_on_device(cores, bits, v)
    got = t.cpu().numpy()
    assert int(status.item()) == 2 and got[1] == 0.0 and not np.signbit(got[1])
    assert np.all(got[[0, 2, 3]] != 0.0)
    env = sm.environments(cores.numpy())
    ref = cm.jvp(cores.numpy(), bits, v.numpy(), env)
    assert ref["t"][1] == 0
    kappa = hp.to_f64(ref["sr"]["kappa"])
    C = cm.c_jvp(n, D, np.where(np.isfinite(kappa), kappa, 1.0), float(env["Z_abs"] / env["Z"]))
    w, at = hp.worst(hp.ratio(got, ref["t"], ref["t_abs"], X=hp._LongDouble) / C)
    print(f"zero amplitude: worst ratio {w:.4f} at {at}")
    assert w <= 1.0


def test_refused_sizes():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    p, nb = buf.data_ptr(), buf.numel()
    UNSUPPORTED, INVALID = -4, -1
    need = lib.bornvi_mps_sample_workspace_bytes(h.h, 8, 4, 8)
    assert 0 < need <= nb
    call = lib.bornvi_mps_score_jvp
    assert call(h.h, 8, 4, 1, p, p, p, 1.0, p, p, p, nb, None) == UNSUPPORTED               # B = 1
    assert call(h.h, 8, 4, (1 << 24) + 1, p, p, p, 1.0, p, p, p, nb, None) == UNSUPPORTED   # B = 2^24 + 1
    assert call(h.h, 64, 4, 8, p, p, p, 1.0, p, p, p, nb, None) == UNSUPPORTED              # n = 64
    assert call(h.h, 8, 33, 8, p, p, p, 1.0, p, p, p, nb, None) == UNSUPPORTED              # D = 33
    assert call(h.h, 0, 4, 8, p, p, p, 1.0, p, p, p, nb, None) == UNSUPPORTED
    assert call(h.h, 8, 0, 8, p, p, p, 1.0, p, p, p, nb, None) == UNSUPPORTED
    assert call(h.h, 8, 4, 8, p, p, p, 1.0, p, p, p, need - 1, None) == UNSUPPORTED         # a short workspace
    assert call(h.h, 8, 4, 8, p, p, p, 1.0, p, p, None, nb, None) == UNSUPPORTED
    assert call(h.h, 8, 4, 8, p, p, None, 1.0, p, p, p, nb, None) == INVALID                # a null pointer
    assert call(h.h, 8, 4, 8, p, p, p, float('inf'), p, p, p, nb, None) == INVALID
    torch.cuda.synchronize()
    assert int(buf.count_nonzero().item()) == 0                                             # nothing was launched
    # the size the existing callers allocate by has not moved: the layout of kernels_mps_sample.hip, restated
    up = lambda b: (b + 255) & ~255
    for n, D, B in ((8, 4, 8), (63, 32, 1 << 24), (5, 3, 130)):
        G, DS = min(-(-B // 64), 256), (D + 1) & ~1
        want = 256 + 2 * up(8 * (n + 1) * D * D) + 2 * up(4 * (n + 1)) + up(8 * G * n * 64 * DS) + up(4 * G * n * 64) \
            + up(8 * G * n * 2 * D * D) + up(8 * 256) + up(8 * n * 2 * D * D) + 256
        assert lib.bornvi_mps_sample_workspace_bytes(h.h, n, D, B) == want
    c = make_cores(3, 2).to(dev())
    with pytest.raises(backend.BornviError):
        backend.mps_score_jvp(c, torch.zeros(1, dtype=torch.int64, device=dev()), c)
    with pytest.raises(backend.BornviError):
        backend.mps_score_jvp(c, torch.zeros(8, dtype=torch.int64, device=dev()), c[:2])
    with pytest.raises(backend.BornviError):
        backend.mps_score_jvp(c, torch.zeros(8, dtype=torch.int64, device=dev()), c, scale=float('nan'))


def test_capture_and_replay():
    """environments + jvp under torch.cuda.graph on a side stream, replayed twice: equal to the eager result bit for bit,
    the status word cleared and set again by every replay."""
    n, D, B = 5, 3, 130
    R = reference(n, D, B)
    c, idx, t, status = jvp_on_device(R["cores"], R["bits"], R["v"], 1.0 / B)
    eager = t.clone()
    v = R["v"].to(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # the side stream's workspace exists before the capture
        backend.mps_environments(c, B)
        out, st = backend.mps_score_jvp(c, idx, v, 1.0 / B)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.mps_environments(c, B)
        backend.mps_score_jvp(c, idx, v, 1.0 / B, out=out, status=st)
    for _ in range(2):
        out.zero_()
        st.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and int(st.item()) == 0
