"""bornvi_cmps_environments / _sample / _score_vjp (complex cores, kernels_cmps.hip) against the extended-precision mirror
(cmps_mirror.py), per entry the hp_reference.ratio way, and their contract: draws that do not depend on the batch, exact
power-of-two rescaling, Hermitian environments, exact zeros, the status word, bitwise reproducible, refused sizes, capturable,
the real family at zero imaginary parts, and an independent oracle through from_statevector.

Shapes: n in {1, 2, 3, 12, 33, 63}, D in {1, 2, 3, 4, 5, 8, 9, 16} (the odd pad and both sides of every DP template edge
2 | 4 | 8 | 16), B in {1, 63, 64, 65, 257, 4099}, not their cross product, and one score case with more than 256 tiles.

Error bounds, derived from the kernels' operation chains (units of EPS64 = 2^-52, every rounding counted as a whole unit; the
power-of-two rescalings add none).  A complex D-term chain is two real 2 D-term chains (one per part), so every count of
test_gpu_mps_sampled_kernel.py holds with 2 D for D, against the majorants of cmps_mirror.py (M = |X| + |Y|):
  E_k, L_k after j steps: a 2 D-term chain (T_s) and a 4 D-term one:  C_ENV(j) = j (6 D + 1);  kappa_Z = Z_abs / Z.
  psi of a sample: n 2 D-term chains: C_PSI = 2 n D + 2 against psi_abs;  kappa_b = psi_abs / |psi|.
  logq = 2 log hypot(l_n[0]) - log E^_0[0,0] + (2 el - eE[0]) ln 2:  2 C_PSI kappa_b + C_ENV(n) kappa_Z and the assembly: the
    hypot (one unit of |psi|: two of the log), two logs, one product with ln 2 and three additions, each at most a unit of the
    largest partial result:  ASSEMBLE = 8 (|log psi^2| + |log Z| + 4) + 2.
  grad against grad_abs, C_SCORE = 1 + the larger of
    the sample term: l_{k-1} and r_k (2 (n - 1) D together), g = 2 w / psi (C_PSI kappa_max, the hypot, two quotients and two
      products: 5), the complex product g l (3), and the sum over samples: two products of 64 terms in the matrix core per
      tile (128), the workgroup's tiles and the G partials in order:  2 (n - 1) D + C_PSI kappa_max + 8 + 128 + tiles + G;
    the environment term: L_{k-1} and E_k (C_ENV(n - 1) together), the two 2 D-term chains (4 D), 1 / Z (C_ENV(n) kappa_Z),
      sum w (6 butterfly levels, the tiles, the G totals: 6 + tiles + ceil(G / 256) + 9) and four more operations.
  The gradient's bound goes through hp.measured_constant: max(16, 8 x what the float64 mirror shows on the same samples), never
  above C_SCORE.  Nothing is fitted to the device: each test prints the worst ratio beside its C."""
import functools
import math

import numpy as np
import pytest
import torch

import cmps_mirror as cx
import hp_reference as hp
import mps_sampled_mirror as sm
from cmps_mirror import c_env, c_score, geometry, logq_bound          # the counts derived above, as functions
from tensornetworks_amd import backend

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
SEED = 20240
EPOCH = 3
CASES = [(1, 1, 1), (1, 3, 63), (2, 2, 64), (3, 5, 65), (3, 9, 1), (12, 3, 257), (12, 8, 64), (12, 4, 65), (33, 2, 257),
         (33, 16, 64), (63, 4, 4099), (63, 16, 63), (63, 1, 65), (2, 9, 257)]
SCORE_CASES = CASES + [(2, 5, 16500)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def make_cores(n, D, seed=0, spread=0.3):
    gen = torch.Generator().manual_seed(9000 * n + 17 * D + seed)
    c = spread * torch.randn(n, 2, D, D, 2, dtype=torch.float64, generator=gen)
    c[..., 0] += torch.eye(D, dtype=torch.float64)
    return (c / math.sqrt(2.0)).contiguous()


def workspace_view(n, D, B):
    """(E^ complex [n + 1, D, D], eE [n + 1], L^, eL) read back from the cached workspace (the layout of kernels_cmps.hip)."""
    d = dev()
    buf = backend._workspaces[backend._ws_key(d, f"cmps_{n}_{D}_{B}")]
    base = (-buf.data_ptr()) % 256
    up = lambda b: (b + 255) & ~255
    raw = buf.cpu().numpy()[base:]
    o = 256
    ne = (n + 1) * 2 * D * D
    out = []
    for _ in range(2):
        planes = raw[o:o + 8 * ne].view(np.float64).reshape(n + 1, 2, D, D).copy()
        o += up(8 * ne)
        out.append(planes)
    eE = raw[o:o + 4 * (n + 1)].view(np.int32).copy(); o += up(4 * (n + 1))
    eL = raw[o:o + 4 * (n + 1)].view(np.int32).copy()
    return out[0], eE, out[1], eL


@functools.lru_cache(maxsize=None)
def sampled(n, D, B):
    """One run of environments + sample of a case and the mirror's evaluation on the GPU's own prefixes, shared by the tests."""
    cores = make_cores(n, D)
    c = cores.to(dev())
    ep = torch.tensor([EPOCH], dtype=torch.int64, device=dev())
    logZ = backend.cmps_environments(c, B)
    idx, logq, status = backend.cmps_sample(c, B, SEED, ep)
    torch.cuda.synchronize()
    envs = workspace_view(n, D, B)
    env = cx.environments(cores.numpy())
    bits = cx.bits_of_idx(idx.cpu().numpy(), n)
    cond = cx.conditionals(cores.numpy(), bits, env)
    return dict(cores=cores, logZ=float(logZ.item()), idx=idx.cpu().numpy(), logq=logq.cpu().numpy(), status=int(status.item()),
                envs=envs, env=env, bits=bits, cond=cond)


@pytest.mark.parametrize("n,D,B", CASES)
def test_environments_and_log_z(n, D, B):
    r = sampled(n, D, B)
    Eh, eE, Lh, eL = r["envs"]
    env = r["env"]
    worst = 0.0
    for k in range(n + 1):
        for planes, ex, ref, ab, C in ((Eh[k], eE[k], env["E"][k], env["E_abs"][k], c_env(n - k, D)),
                                       (Lh[k], eL[k], env["L"][k], env["L_abs"][k], c_env(k, D))):
            # Hermitian bit for bit, and the power-of-two rescaling: the largest |re| or |im| of a stored matrix lies in [1, 2)
            assert np.array_equal(planes[0], planes[0].T) and np.array_equal(planes[1], -planes[1].T) and np.all(np.diag(planes[1]) == 0)
            assert 1.0 <= np.abs(planes).max() < 2.0
            scale = cx.LD(2.0) ** int(ex)
            for got, want in ((planes[0].astype(cx.LD) * scale, ref.real), (planes[1].astype(cx.LD) * scale, ref.imag)):
                err = np.abs(got - want)
                if C == 0:
                    assert np.all(err == 0)
                    continue
                den = ab * cx.LD(EPS)
                ratio = float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), np.where(err == 0, 0, np.inf)))) / C
                worst = max(worst, ratio)
    kZ = float(env["Z_abs"] / env["Z"])
    logZ_ref = float(np.log(env["Z"]))
    bound = EPS * (c_env(n, D) * kZ + 8 * (abs(logZ_ref) + 4))
    print(f"n={n} D={D}: worst environment ratio / C_ENV = {worst:.3f}; |logZ err| / bound = {abs(r['logZ'] - logZ_ref) / bound:.3f}")
    assert worst <= 1.0
    assert abs(r["logZ"] - logZ_ref) <= bound


@pytest.mark.parametrize("n,D,B", CASES)
def test_sampler_bits_and_logq(n, D, B):
    r = sampled(n, D, B)
    assert r["status"] == 0
    U = cx.uniforms(SEED, EPOCH, np.arange(B), n)
    p1 = hp.to_f64(r["cond"]["p1"])
    p0 = hp.to_f64(1 - r["cond"]["p1"])
    undecided = int(((np.abs(U - p1) <= 2.0 ** -40) | (np.abs(U - p0) <= 2.0 ** -40)).sum())
    assert undecided == 0
    assert np.array_equal(r["bits"], (U >= p0).astype(np.int64))
    assert np.all(r["idx"] >= 0) and (n == 63 or np.all(r["idx"] < (1 << n)))
    env = r["env"]
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(r["cond"]["psi_abs"] / np.abs(r["cond"]["psi"]))
    ref = r["cond"]["logq"]
    bound = logq_bound(n, D, kb, kZ, hp.to_f64(ref), float(np.log(env["Z"])))
    ratio = np.abs(hp.to_f64(r["logq"].astype(cx.LD) - ref)) / (EPS * bound)
    print(f"n={n} D={D} B={B}: worst logq ratio = {ratio.max():.3f} (bound in units of eps: up to {bound.max():.0f})")
    assert ratio.max() <= 1.0


def test_draws_do_not_depend_on_the_batch():
    n, D = 63, 4
    big = sampled(n, D, 4099)
    c = big["cores"].to(dev())
    ep = torch.tensor([EPOCH], dtype=torch.int64, device=dev())
    backend.cmps_environments(c, 64)
    idx, logq, _ = backend.cmps_sample(c, 64, SEED, ep)
    assert np.array_equal(idx.cpu().numpy(), big["idx"][:64]) and np.array_equal(logq.cpu().numpy(), big["logq"][:64])
    idx2, logq2, _ = backend.cmps_sample(c, 64, SEED, ep)
    assert torch.equal(idx, idx2) and torch.equal(logq, logq2)          # two calls are bitwise equal
    other_epoch, _, _ = backend.cmps_sample(c, 64, SEED, torch.tensor([EPOCH + 1], dtype=torch.int64, device=dev()))
    other_seed, _, _ = backend.cmps_sample(c, 64, SEED + 1, ep)
    assert not torch.equal(idx, other_epoch) and not torch.equal(idx, other_seed)


@pytest.mark.parametrize("n,D,B", SCORE_CASES)
def test_score_vjp_against_the_mirror(n, D, B):
    """The gradient on the GPU's own samples, weights from a generator."""
    cores = make_cores(n, D)
    c = cores.to(dev())
    ep = torch.tensor([EPOCH], dtype=torch.int64, device=dev())
    w = np.random.default_rng([n, D, B, 5]).standard_normal(B)
    wt = torch.from_numpy(w).to(dev())
    backend.cmps_environments(c, B)
    idx, _, _ = backend.cmps_sample(c, B, SEED, ep)
    grad, logq, status = backend.cmps_score_vjp(c, idx, wt)
    grad2, logq2, _ = backend.cmps_score_vjp(c, idx, wt)
    torch.cuda.synchronize()
    assert torch.equal(grad, grad2) and torch.equal(logq, logq2)                # bitwise reproducible
    assert int(status.item()) == 0 and tuple(grad.shape) == (n, 2, D, D, 2)
    bits = cx.bits_of_idx(idx.cpu().numpy(), n)
    env = cx.environments(cores.numpy())
    ref = cx.score_gradient(cores.numpy(), bits, w, env)
    f64 = cx.score_gradient(cores.numpy(), bits, w, dtype=np.float64)
    kZ = float(env["Z_abs"] / env["Z"])
    kmax = float(ref["kappa"].max())
    oracle, _ = hp.worst(hp.ratio(f64["grad"], ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    derived = c_score(n, D, B, kmax, kZ)
    C = hp.measured_constant(oracle, derived)
    g = grad.cpu().numpy()
    r, at = hp.worst(hp.ratio(g, ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    print(f"n={n} D={D} B={B}: worst grad ratio {r:.2f} at {at}, C = {C:.0f} (float64 mirror {oracle:.2f}, derived {derived:.0f}, "
          f"kappa_max {kmax:.2f}, kappa_Z {kZ:.2f})")
    assert r <= C
    if D > 1:
        assert np.all(g[0][:, 1:] == 0.0) and np.all(g[n - 1][:, :, 1:] == 0.0)
    bound = logq_bound(n, D, hp.to_f64(ref["kappa"]), kZ, hp.to_f64(ref["logq"]), float(np.log(env["Z"])))
    assert np.all(np.abs(hp.to_f64(logq.cpu().numpy().astype(cx.LD) - ref["logq"])) <= EPS * bound)


def test_power_of_two_scaling_and_status():
    """n = 63, D = 4: cores times 2^12 (2^-12) multiply |psi|^2 by 2^(+-1512): beyond float64 without the rescaling.  idx stays
    bitwise the same, logq within the bound.  A zero core: status 1, idx 0, logZ -inf; then status 2 from the gradient."""
    n, D, B = 63, 4, 4099
    r = sampled(n, D, B)
    ep = torch.tensor([EPOCH], dtype=torch.int64, device=dev())
    env = r["env"]
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(r["cond"]["psi_abs"] / np.abs(r["cond"]["psi"]))
    for p in (12, -12):
        c = (r["cores"] * 2.0 ** p).to(dev())
        logZ = backend.cmps_environments(c, B)
        idx, logq, status = backend.cmps_sample(c, B, SEED, ep)
        assert int(status.item()) == 0 and np.array_equal(idx.cpu().numpy(), r["idx"])
        shift = 2 * n * p * math.log(2.0)
        assert abs(float(logZ.item()) - (float(np.log(env["Z"])) + shift)) <= EPS * (c_env(n, D) * kZ + 8 * (abs(shift) + abs(r["logZ"]) + 4))
        bound = logq_bound(n, D, kb, kZ, hp.to_f64(r["cond"]["logq"]), float(np.log(env["Z"])) + shift) + 16 * abs(shift)
        assert np.all(np.abs(hp.to_f64(logq.cpu().numpy().astype(cx.LD) - r["cond"]["logq"])) <= EPS * bound)
        grad, lq, st = backend.cmps_score_vjp(c, idx, torch.ones(B, dtype=torch.float64, device=dev()) / B)
        assert int(st.item()) == 0 and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(lq).all())
    z = r["cores"].clone()
    z[40] = 0.0
    c = z.to(dev())
    logZ = backend.cmps_environments(c, B)
    idx, logq, status = backend.cmps_sample(c, B, SEED, ep)
    assert int(status.item()) == 1 and bool((idx == 0).all()) and float(logZ.item()) == -math.inf and bool(torch.isnan(logq).all())
    grad, lq, st = backend.cmps_score_vjp(c, idx, torch.zeros(B, dtype=torch.float64, device=dev()))
    assert int(st.item()) == 2


def test_score_vjp_zero_amplitude():
    """A sample with psi = 0: logq -inf, no contribution to the sample term, status 2."""
    n, D = 4, 2
    cores = make_cores(n, D, seed=2)
    cores[1, 1] = 0.0                                   # every z with z_2 = 1 has psi = 0
    bits = np.array([[0, 0, 1, 0], [0, 1, 0, 1], [1, 0, 0, 1]])
    w = np.array([0.5, -2.0, 1.5])
    c = cores.to(dev())
    backend.cmps_environments(c, 3)
    grad, logq, status = backend.cmps_score_vjp(c, torch.from_numpy(cx.idx_of_bits(bits)).to(dev()), torch.from_numpy(w).to(dev()))
    assert int(status.item()) == 2 and float(logq[1].item()) == -math.inf and bool(torch.isfinite(logq[[0, 2]]).all())
    env = cx.environments(cores.numpy())
    ref = cx.score_gradient(cores.numpy(), bits, w, env)
    C = c_score(n, D, 3, float(ref["kappa"][[0, 2]].max()), float(env["Z_abs"] / env["Z"]))
    r, at = hp.worst(hp.ratio(grad.cpu().numpy(), ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    assert r <= C, (r, at)


@pytest.mark.parametrize("value", [math.inf, math.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("part", [0, 1], ids=["re", "im"])
def test_non_finite_core_entry(value, part):
    """The real contract for a non-finite number, n = 12, D = 3, one Inf or NaN in the real or the imaginary part of
    A_8[0][0, 0]: log Z is not finite; every environment left of the site is non-finite, so every sample meets a mass that is
    not finite at its first site: status 1, every bit 0, logq NaN; the gradient call finds no sample that counts (E_0[0, 0] is
    not finite and positive): status 2 and logq NaN for every sample, those whose psi avoids the entry included."""
    n, D, B = 12, 3, 65
    bad = make_cores(n, D).clone()
    bad[7, 0, 0, 0, part] = value
    c = bad.to(dev())
    ep = torch.tensor([EPOCH], dtype=torch.int64, device=dev())
    logZ = backend.cmps_environments(c, B)
    idx, logq, status = backend.cmps_sample(c, B, SEED, ep)
    assert not math.isfinite(float(logZ.item()))
    assert int(status.item()) == 1 and bool((idx == 0).all()) and bool(torch.isnan(logq).all())
    # samples on both sides of the entry: z_8 = 0 reads it, z_8 = 1 does not
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 2, size=(B, n))
    bits[0, 7], bits[1, 7] = 0, 1
    w = torch.from_numpy(rng.standard_normal(B)).to(dev())
    grad, lq, st = backend.cmps_score_vjp(c, torch.from_numpy(cx.idx_of_bits(bits)).to(dev()), w)
    assert int(st.item()) == 2 and bool(torch.isnan(lq).all())
    assert tuple(grad.shape) == (n, 2, D, D, 2)
    # the same calls on the sound cores afterwards: nothing of the bad run is left in the workspace
    good = make_cores(n, D).to(dev())
    assert math.isfinite(float(backend.cmps_environments(good, B).item()))
    idx, logq, status = backend.cmps_sample(good, B, SEED, ep)
    assert int(status.item()) == 0 and bool(torch.isfinite(logq).all())
    assert np.array_equal(idx.cpu().numpy(), sampled(n, D, 257)["idx"][:B])


def test_refused_sizes_leave_everything_untouched():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    UNSUPPORTED = _ext._ENUMS["BORNVI_ERR_UNSUPPORTED"]
    size = lib.bornvi_cmps_workspace_bytes
    for n, D, B in ((0, 4, 8), (64, 4, 8), (8, 0, 8), (8, 17, 8), (8, 4, 0), (8, 4, (1 << 24) + 1)):
        assert size(h.h, n, D, B) == 0
    # the workspace does not grow with B beyond 256 tiles of 64 samples
    assert size(h.h, 63, 16, 1 << 24) == size(h.h, 63, 16, 256 * 64) > size(h.h, 63, 16, 255 * 64)
    n, D, B = 8, 4, 8
    need = size(h.h, n, D, B)
    canary = lambda count, dtype: torch.full((count,), 77, dtype=dtype, device=dev())
    ws, cores = canary(need, torch.uint8), make_cores(n, D).to(dev())
    idx, logq, grad, st, lz = canary(B, torch.int64), canary(B, torch.float64), canary(cores.numel(), torch.float64), canary(1, torch.int32), canary(1, torch.float64)
    w, ep = torch.ones(B, dtype=torch.float64, device=dev()), torch.zeros(1, dtype=torch.int64, device=dev())
    P = lambda t: t.data_ptr()
    for nn, DD, BB, bytes_ in ((0, D, B, need), (64, D, B, need), (n, 0, B, need), (n, 17, B, need), (n, D, 0, need), (n, D, (1 << 24) + 1, need),
                               (n, D, B, need - 1), (n, D, B, 0)):
        assert lib.bornvi_cmps_environments(h.h, nn, DD, BB, P(cores), P(lz), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_cmps_sample(h.h, nn, DD, BB, P(cores), 1, P(ep), P(idx), P(logq), P(st), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_cmps_score_vjp(h.h, nn, DD, BB, P(cores), P(idx), P(w), P(logq), P(grad), P(st), P(ws), bytes_, None) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (ws, idx, logq, grad, st, lz):
        assert bool((t == 77).all())


def test_capture_and_replay():
    """One graph of environments + sample + score_vjp; epoch_dev changes between the replays; equal to the eager calls."""
    n, D, B = 12, 5, 257
    c = make_cores(n, D, seed=3).to(dev())
    ep = torch.zeros(1, dtype=torch.int64, device=dev())
    w = torch.from_numpy(np.random.default_rng(1).standard_normal(B)).to(dev())
    eager = {}
    for e in (0, 1, 2):
        ep.fill_(e)
        backend.cmps_environments(c, B)
        idx, logq, _ = backend.cmps_sample(c, B, SEED, ep)
        grad, _, _ = backend.cmps_score_vjp(c, idx, w)
        eager[e] = (idx.clone(), logq.clone(), grad.clone())
    idx = torch.empty(B, dtype=torch.int64, device=dev())
    logq = torch.empty(B, dtype=torch.float64, device=dev())
    lq2 = torch.empty(B, dtype=torch.float64, device=dev())
    grad = torch.empty_like(c)
    st1 = torch.empty(1, dtype=torch.int32, device=dev())
    st2 = torch.empty(1, dtype=torch.int32, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        backend.cmps_environments(c, B)                         # the side stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.cmps_environments(c, B)
        backend.cmps_sample(c, B, SEED, ep, out_idx=idx, out_logq=logq, status=st1)
        backend.cmps_score_vjp(c, idx, w, out=grad, out_logq=lq2, status=st2)
    for e in (2, 0, 1):
        ep.fill_(e)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, eager[e][0]) and torch.equal(logq, eager[e][1]) and torch.equal(grad, eager[e][2])
        assert int(st1.item()) == 0 and int(st2.item()) == 0


# ---- zero imaginary parts: the real family ---------------------------------------------------------------------------------
def real_c_env(j, D):
    return float(j * (3 * D + 1))


def real_logq_bound(n, D, kappa_b, kappa_Z, logq, logZ):
    lpsi2 = np.where(np.isfinite(logq), logq + logZ, 0.0)
    return 2 * (n * D + 2) * kappa_b + real_c_env(n, D) * kappa_Z + 8 * (np.abs(lpsi2) + abs(logZ) + 4)


def real_c_score(n, D, B, kappa_max, kappa_Z):
    G, tiles = geometry(B)
    sample = (n - 1) * D + (n * D + 2) * kappa_max + 3 + 64 + tiles + G
    envt = real_c_env(n - 1, D) + 2 * D + real_c_env(n, D) * kappa_Z + 6 + tiles + (-(-G // 256)) + 9 + 4
    return 1.0 + max(sample, envt)


@pytest.mark.parametrize("n,D,B", [(12, 8, 257), (63, 4, 4099)])
def test_zero_imaginary_parts_are_the_real_family(n, D, B):
    """The real calls' bounds are those of test_gpu_mps_sampled_kernel.py (restated above), added to this file's."""
    gen = torch.Generator().manual_seed(5000 * n + D)
    real = ((torch.eye(D, dtype=torch.float64) + 0.3 * torch.randn(n, 2, D, D, dtype=torch.float64, generator=gen)) / math.sqrt(2.0)).contiguous()
    cores = torch.stack((real, torch.zeros_like(real)), dim=-1).contiguous()
    # the seed is chosen on the CPU: the float64 mirror has no draw within 1e-10 of its uniform
    seed = next(s for s in range(SEED, SEED + 8) if sm.sample(real.numpy(), s, EPOCH, B, dtype=np.float64, margin=1e-10)["undecided"] == 0)
    assert seed == SEED
    cr, cc = real.to(dev()), cores.to(dev())
    ep = torch.tensor([EPOCH], dtype=torch.int64, device=dev())
    w = torch.from_numpy(np.random.default_rng([n, D, B]).standard_normal(B)).to(dev())
    lZr = backend.mps_environments(cr, B)
    ir, lqr, sr = backend.mps_sample(cr, B, seed, ep)
    gr, lqr2, sr2 = backend.mps_score_vjp(cr, ir, w)
    lZc = backend.cmps_environments(cc, B)
    ic, lqc, sc = backend.cmps_sample(cc, B, seed, ep)
    gc, lqc2, sc2 = backend.cmps_score_vjp(cc, ir, w)              # the real call's samples: the same sums
    torch.cuda.synchronize()
    assert int(sr.item()) == int(sc.item()) == 0 and int(sr2.item()) == int(sc2.item()) == 0
    ir_, ic_ = ir.cpu().numpy(), ic.cpu().numpy()
    differ = np.nonzero(ir_ != ic_)[0]
    if len(differ):      # excused only where the float64 mirror's conditional at the first differing site is within 1e-10 of the uniform
        assert len(differ) <= B // 1000
        bits = sm.bits_of_idx(ir_[differ], n)
        first = np.argmax(bits != sm.bits_of_idx(ic_[differ], n), axis=1)
        p1 = hp.to_f64(sm.conditionals(real.numpy(), bits, dtype=np.float64)["p1"])[np.arange(len(differ)), first]
        U = sm.uniforms(seed, EPOCH, differ, n)[np.arange(len(differ)), first]
        assert np.all((np.abs(U - (1 - p1)) <= 1e-10) | (np.abs(U - p1) <= 1e-10))     # (mps_sampled_mirror.sample's two tests)
    same = ir_ == ic_
    bits = sm.bits_of_idx(ir_, n)
    env = sm.environments(real.numpy())
    ref = sm.score_gradient(real.numpy(), bits, w.cpu().numpy(), env)
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(ref["kappa"])
    logZ = float(np.log(env["Z"]))
    # with zero imaginary parts the majorant is |cores|: the complex bounds take the same kappas
    assert abs(float(lZr.item()) - float(lZc.item())) <= EPS * ((real_c_env(n, D) + c_env(n, D)) * kZ + 16 * (abs(logZ) + 4))
    both = real_logq_bound(n, D, kb, kZ, hp.to_f64(ref["logq"]), logZ) + logq_bound(n, D, kb, kZ, hp.to_f64(ref["logq"]), logZ)
    assert np.all(np.abs(lqr.cpu().numpy() - lqc.cpu().numpy())[same] <= EPS * both[same])
    assert np.all(np.abs(lqr2.cpu().numpy() - lqc2.cpu().numpy()) <= EPS * both)
    g = gc.cpu().numpy()
    assert np.all(g[..., 1] == 0.0)                                    # the imaginary half: exactly 0.0 everywhere
    C = real_c_score(n, D, B, float(kb.max()), kZ) + c_score(n, D, B, float(kb.max()), kZ)
    err = np.abs(g[..., 0] - gr.cpu().numpy())
    ratio = err / (EPS * hp.to_f64(ref["grad_abs"]) + 1e-300)
    print(f"n={n} D={D} B={B}: {len(differ)} samples differ; worst |re grad - real grad| ratio {ratio.max():.2f}, C = {C:.0f}")
    assert np.all(err <= EPS * C * hp.to_f64(ref["grad_abs"]))


# ---- an independent oracle ---------------------------------------------------------------------------------------------------
def test_statevector_round_trip_and_normalisation():
    from tensornetworks_amd import ComplexSampledMPSBornMachine
    n, D = 8, 16
    rng = np.random.default_rng(88)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    psi /= np.linalg.norm(psi)
    bm, _ = ComplexSampledMPSBornMachine.from_statevector(torch.as_tensor(psi), D)
    bm = bm.to(dev())
    idx = torch.arange(1 << n, dtype=torch.int64, device=dev())
    logq = bm.log_prob(idx).cpu().numpy()
    cores = bm.cores.detach().cpu().numpy()
    env = cx.environments(cores)
    cond = cx.conditionals(cores, cx.all_bits(n), env)
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(cond["psi_abs"] / np.abs(cond["psi"]))
    want = np.log(np.abs(psi) ** 2)
    # the cores carry the SVDs' own error: 1e-13 on an amplitude (test_cmps_host.py), 2e-13 / |psi| on log|psi|^2, and as much on log Z
    bound = EPS * logq_bound(n, D, kb, kZ, want, float(np.log(env["Z"]))) + 2e-13 / np.abs(psi) + 2e-13
    print(f"statevector n={n}: worst |log_prob - log|psi|^2| / bound = {np.max(np.abs(logq - want) / bound):.3f}")
    assert np.all(np.abs(logq - want) <= bound)
    p = bm.probabilities64().cpu().numpy()
    assert np.all(np.abs(p - np.exp(logq)) <= 4 * EPS * p)          # exp of the same logq, the device's exp against NumPy's
    # sum_z exp(logq) = 1 at n = 12, D = 3
    n, D = 12, 3
    torch.manual_seed(5)
    bm = ComplexSampledMPSBornMachine(n, bond_dim=D, init_method="random").to(dev())
    q = bm.probabilities64().cpu().numpy()
    cores = bm.cores.detach().cpu().numpy()
    env = cx.environments(cores)
    cond = cx.conditionals(cores, cx.all_bits(n), env)
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(cond["psi_abs"] / np.abs(cond["psi"]))
    lb = logq_bound(n, D, kb, kZ, hp.to_f64(cond["logq"]), float(np.log(env["Z"])))
    # exp carries logq's absolute error as a relative one (+ 2 for exp); the 2^n-term sum in float64 adds n + 1 units of the total
    bound = float((q * EPS * (lb + 2)).sum()) + EPS * (n + 1)
    print(f"sum of q at n={n} D={D}: |sum - 1| = {abs(q.sum() - 1):.2e}, bound {bound:.2e}")
    assert abs(float(q.sum()) - 1.0) <= bound
    assert tuple(bm.get_probabilities().shape) == (1, 1 << n)
