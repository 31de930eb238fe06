"""bornvi_mps_score_sample_gram and SampleSpaceFisherPreconditioner against the extended-precision mirrors
(sample_gram_mirror.py on sampled_fisher_mirror.py), per entry the hp_reference.ratio way, and the call's contract: T == T^T
bitwise, bitwise reproducible, an entry independent of B and of its tile, exact zeros for a dead sample, the refused sizes,
capturable, and the fallback to the plain gradient.

Error bound of one T entry (units of EPS64 = 2^-52 on T_abs = rows_abs^T rows_abs / B, every rounding a whole unit, derived in
sample_gram_mirror.c_sample_gram): 4 + the largest of the pair term's, the two m terms' and M's constants.  The constant
is not fitted: each test prints the worst ratio beside its C."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_sampled_mirror as sm
import sample_gram_mirror as gm
import sampled_fisher_mirror as fm
from tensornetworks_amd import backend
from tensornetworks_amd.backend import mps_score_sample_gram  # noqa: F401  (fails without the feature)
from tensornetworks_amd.natural_gradient import SampledFisherPreconditioner, SampleSpaceFisherPreconditioner
from test_gpu_mps_sampled_kernel import make_cores
from test_gpu_sampled_natgrad_kernel import rows_inputs

pytestmark = pytest.mark.gpu
EPS = hp.EPS64

CASES = [(1, 1, 2), (3, 2, 64), (3, 2, 65), (5, 3, 130), (4, 5, 257), (6, 16, 192), (2, 32, 64), (63, 4, 128), (3, 2, 1024)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def gram_on_device(cores, bits):
    B = bits.shape[0]
    idx = torch.from_numpy(sm.idx_of_bits(bits)).to(dev())
    c = cores.to(dev())
    backend.mps_environments(c, B)
    T, status = backend.mps_score_sample_gram(c, idx)
    return c, idx, T, status


def entry_constants(n, D, ref, env):
    kappa = hp.to_f64(ref["kappa"])
    kappa = np.where(np.isfinite(kappa), kappa, 1.0)                                 # a dead sample: its entries are exact zeros
    kZ = float(env["Z_abs"] / env["Z"])
    return gm.c_sample_gram(n, D, kappa[:, None], kappa[None, :], kZ), kZ


@pytest.mark.parametrize("n,D,B", CASES)
def test_sample_gram_against_the_mirror(n, D, B):
    cores = make_cores(n, D, seed=4)
    bits = rows_inputs(n, D, B)
    c, idx, T, status = gram_on_device(cores, bits)
    T2, _ = backend.mps_score_sample_gram(c, idx)
    assert tuple(T.shape) == (B, B) and int(status.item()) == 0
    assert torch.equal(T, T2)                                                        # bitwise reproducible
    assert torch.equal(T, T.t())                                                     # T == T^T bitwise
    got = T.cpu().numpy()
    assert np.all(np.diagonal(got) >= 0.0)
    env = sm.environments(cores.numpy())
    G = gm.sample_gram(cores.numpy(), bits, env)
    C, kZ = entry_constants(n, D, G["sr"], env)
    r = hp.ratio(got, G["T"], G["T_abs"], X=hp._LongDouble) / C
    w, at = hp.worst(r)
    print(f"n={n} D={D} B={B}: worst T error / (C EPS T_abs) = {w:.4f} at {at}, C up to {C.max():.0f} "
          f"(kappa_max {float(G['sr']['kappa'].max()):.2f}, kappa_Z {kZ:.2f})")
    assert w <= 1.0
    if B > 8:                                                                        # rows_inputs repeats sample B // 2 at 3 and 5
        assert np.array_equal(got[3, 3:4], got[5, 5:6]) and np.array_equal(got[3, 6:], got[5, 6:])


def test_sample_gram_against_the_device_rows():
    """B T against X^T X with X the rows bornvi_mps_score_rows wrote, the product formed on the host in float64: within
    c_sample_gram + c_rows(b) + c_rows(b') + P (the host's P-term chain), in units of EPS64 on B T_abs."""
    n, D, B = 5, 3, 130
    cores = make_cores(n, D, seed=4)
    bits = rows_inputs(n, D, B)
    c, idx, T, _ = gram_on_device(cores, bits)
    rows, _ = backend.mps_score_rows(c, idx)
    X = rows.cpu().numpy()[:, :, :B].reshape(-1, B)
    host = X.T @ X                                                                   # float64
    env = sm.environments(cores.numpy())
    G = gm.sample_gram(cores.numpy(), bits, env)
    C, kZ = entry_constants(n, D, G["sr"], env)
    Cr = fm.c_rows(n, D, hp.to_f64(G["sr"]["kappa"]), kZ)
    bound = C + Cr[:, None] + Cr[None, :] + X.shape[0]
    BT = T.cpu().numpy().astype(sm.LD) * sm.LD(B)
    err = np.abs(BT - host.astype(sm.LD))
    r = hp.to_f64(err / (G["T_abs"] * sm.LD(B) * sm.LD(EPS))) / bound
    w, at = hp.worst(r)
    print(f"n={n} D={D} B={B}: worst |B T - X^T X| / (bound EPS B T_abs) = {w:.4f} at {at}, bound up to {bound.max():.0f}")
    assert w <= 1.0


def test_an_entry_does_not_depend_on_the_batch_or_the_tile():
    """B T of the first 64 of 128 samples against B T of those 64 alone: other tiles, another grid, the same bits up to the
    one division (2 units; both divisors are powers of two here, so the difference printed is 0)."""
    n, D = 5, 3
    cores = make_cores(n, D, seed=4)
    bits = rows_inputs(n, D, 128)
    _, _, T128, _ = gram_on_device(cores, bits)
    _, _, T64, _ = gram_on_device(cores, bits[:64].copy())
    a, b = T128.cpu().numpy()[:64, :64] * 128.0, T64.cpu().numpy() * 64.0
    units = np.abs(a - b) / (EPS * np.maximum(np.abs(a), np.abs(b)).clip(min=np.finfo(np.float64).tiny))
    print(f"worst |128 T128 - 64 T64| = {units.max():.3f} units; bitwise equal: {np.array_equal(a, b)}")
    assert units.max() <= 2.0
    # and at a B that is no power of two: rows 0 .. 63 of B = 65 (the 65th sample sits in a tile of its own)
    _, _, T65, _ = gram_on_device(cores, np.concatenate([bits[:64], bits[100:101]]))
    c65 = T65.cpu().numpy()[:64, :64] * 65.0
    units = np.abs(c65 - b) / (EPS * np.maximum(np.abs(c65), np.abs(b)).clip(min=np.finfo(np.float64).tiny))
    print(f"worst |65 T65 - 64 T64| = {units.max():.3f} units")
    assert units.max() <= 2.0


def test_sample_gram_zero_amplitude():
    """A sample with psi = 0 (built as test_score_rows_zero_amplitude builds it): status 2 and a row and a column of exactly
    0.0; every other entry within its bound."""
    n, D = 4, 2
    cores = make_cores(n, D, seed=2)
    cores[1, 1] = 0.0                                   # every z with z_2 = 1 has psi = 0
    bits = np.array([[0, 0, 1, 0], [0, 1, 0, 1], [1, 0, 0, 1], [0, 0, 1, 1]])
    _, _, T, status = gram_on_device(cores, bits)
    got = T.cpu().numpy()
    assert int(status.item()) == 2 and np.all(got[1] == 0.0) and np.all(got[:, 1] == 0.0)
    assert not np.signbit(got[1]).any() and not np.signbit(got[:, 1]).any()
    keep = [0, 2, 3]
    assert np.all(got[np.ix_(keep, keep)] != 0.0)
    env = sm.environments(cores.numpy())
    G = gm.sample_gram(cores.numpy(), bits, env)
    assert np.all(G["T"][1] == 0) and np.all(G["T"][:, 1] == 0)
    C, _ = entry_constants(n, D, G["sr"], env)
    w, at = hp.worst(hp.ratio(got, G["T"], G["T_abs"], X=hp._LongDouble) / C)
    print(f"zero amplitude: worst ratio {w:.4f} at {at}")
    assert w <= 1.0


def test_refused_sizes():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    p, nb = buf.data_ptr(), buf.numel()
    UNSUPPORTED = -4
    size = lib.bornvi_mps_score_sample_gram_workspace_bytes
    assert size(h.h, 8, 4, 1) == 0 and size(h.h, 8, 4, 1025) == 0 and size(h.h, 64, 4, 8) == 0 and size(h.h, 8, 33, 8) == 0
    assert size(h.h, 0, 4, 8) == 0 and size(h.h, 8, 0, 8) == 0
    need, env_need = size(h.h, 8, 4, 8), lib.bornvi_mps_sample_workspace_bytes(h.h, 8, 4, 8)
    assert 0 < need <= nb and 0 < env_need <= nb
    call = lib.bornvi_mps_score_sample_gram
    assert call(h.h, 8, 4, 1, p, p, p, p, p, nb, p, nb, None) == UNSUPPORTED          # B = 1
    assert call(h.h, 8, 4, 1025, p, p, p, p, p, nb, p, nb, None) == UNSUPPORTED       # B = 1025
    assert call(h.h, 64, 4, 8, p, p, p, p, p, nb, p, nb, None) == UNSUPPORTED         # n = 64
    assert call(h.h, 8, 33, 8, p, p, p, p, p, nb, p, nb, None) == UNSUPPORTED         # D = 33
    assert call(h.h, 8, 4, 8, p, p, p, p, p, nb, p, need - 1, None) == UNSUPPORTED    # a short workspace
    assert call(h.h, 8, 4, 8, p, p, p, p, p, env_need - 1, p, nb, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.count_nonzero().item()) == 0                                       # nothing was launched
    c = make_cores(3, 2).to(dev())
    with pytest.raises(backend.BornviError):
        backend.mps_score_sample_gram(c, torch.zeros(1, dtype=torch.int64, device=dev()))
    with pytest.raises(backend.BornviError):
        backend.mps_score_sample_gram(c, torch.zeros(1025, dtype=torch.int64, device=dev()))


# ------------------------------------------------------------------------------------------------------------ preconditioner
def weights_inputs(n, D, B, seed):
    cores = make_cores(n, D, seed=seed).to(dev())
    idx = torch.from_numpy(sm.idx_of_bits(rows_inputs(n, D, B))).to(dev())
    w = torch.from_numpy(np.random.default_rng(seed).standard_normal(B)).to(dev())
    return cores, idx, w


def test_precondition_weights_against_the_mirror_and_under_capture():
    """delta against the mirror's PRIMAL blocks='full' solve in extended precision, in the form of
    test_precondition_against_the_mirror_and_under_capture: err <= 1e3 EPS amp, amp = (||T||_inf + lam) / lam from the
    mirror's T.  On the CPU the float64 mirror of the dual formula has error 1.3e-11 at this shape against a bound of 2.1e-5
    (amp = 9.5e7): far more than the 10 times inside it that was required before the bound was used here, and asserted
    again below.  Then the same check (the same bound) against the device's own
    blocks='full' delta, and the same call under torch.cuda.graph on a side stream, replayed twice: equal to
    the eager result bit for bit."""
    n, D, B, lam = 5, 3, 130, 1e-3
    cores, idx, w = weights_inputs(n, D, B, 8)
    pre = SampleSpaceFisherPreconditioner(damping=lam)
    backend.mps_environments(cores, B)
    delta, info = pre.precondition_weights(cores, idx, w)
    eager, einfo = delta.clone(), info.clone()
    assert tuple(eager.shape) == tuple(cores.shape) and einfo.tolist() == [0] and int(pre.status.item()) == 0
    bits = sm.bits_of_idx(idx.cpu().numpy(), n)
    cn, wn = cores.cpu().numpy(), w.cpu().numpy()
    g = sm.score_gradient(cn, bits, wn)["grad"]
    ref, rinfo = fm.precondition(cn, bits, g, lam, "full")
    Tm = gm.sample_gram(cn, bits)["T"]
    amp = (float(np.abs(Tm).sum(axis=1).max()) + lam) / lam
    scale = np.abs(hp.to_f64(ref)).max()
    err = np.abs(eager.cpu().numpy() - hp.to_f64(ref)).max() / scale
    d64, _ = gm.precondition(cn, bits, wn, lam, dtype=np.float64)
    err64 = np.abs(d64 - hp.to_f64(ref)).max() / scale
    print(f"relative error of delta {err:.3e} (float64 mirror of the dual: {err64:.3e}), bound {1e3 * EPS * amp:.3e}, amp {amp:.3e}")
    assert np.all(rinfo == 0) and 10 * err64 <= 1e3 * EPS * amp and err <= 1e3 * EPS * amp
    # the device's own primal solve
    plain, _, _ = backend.mps_score_vjp(cores, idx, w)
    full, finfo = SampledFisherPreconditioner(damping=lam, blocks='full').precondition(cores, idx, plain)
    errd = float((eager - full).abs().max().item()) / scale
    print(f"against the device's blocks='full' delta: {errd:.3e}")
    assert finfo.tolist() == [0] and errd <= 1e3 * EPS * amp
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # the side stream's workspaces exist before the capture
        backend.mps_environments(cores, B)
        pre.precondition_weights(cores, idx, w)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.mps_environments(cores, B)
        out, oinfo = pre.precondition_weights(cores, idx, w)
    for _ in range(2):
        out.zero_()
        oinfo.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(oinfo, einfo)


def test_a_failed_solve_keeps_the_plain_gradient():
    """A NaN in one w_b: info = B + 1 = 1025 (spd_solve: b is not finite), u = w and delta is mps_score_vjp(cores, idx, w) bit
    for bit, NaNs compared as bits."""
    n, D, B = 3, 2, 1024
    cores, idx, w = weights_inputs(n, D, B, 5)
    w[17] = float('nan')
    backend.mps_environments(cores, B)
    plain, _, _ = backend.mps_score_vjp(cores, idx, w)
    plain = plain.clone()
    pre = SampleSpaceFisherPreconditioner()
    delta, info = pre.precondition_weights(cores, idx, w)
    assert info.tolist() == [1025]
    assert np.array_equal(delta.cpu().numpy().view(np.int64), plain.cpu().numpy().view(np.int64))
    assert np.array_equal(pre._u.cpu().numpy().view(np.int64), w.cpu().numpy().view(np.int64))
