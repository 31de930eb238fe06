"""bornvi_mps_environments / _sample / _score_vjp and bornvi_bn_logjoint_samples against the extended-precision mirror
(mps_sampled_mirror.py), per entry the hp_reference.ratio way, and their contract: draws that do not depend on the batch,
exact power-of-two rescaling, exact zeros, the status word, bitwise reproducible, refused sizes, capturable.

Shapes: n in {1, 2, 3, 12, 33, 63} (one site with both boundaries, an index past 32 bits, the top of the range), D in
{1, 2, 3, 5, 16, 17, 32} (the odd pad and every DP template edge), B in {1, 63, 64, 65, 257, 4099} (a wave, a tile, the
finishing of several workgroups), not their cross product; every case has at most 2^18 draws.

Error bounds, derived from the kernels' operation chains (units of EPS64 = 2^-52, every rounding counted as a whole unit;
the power-of-two rescalings add none):
  E_k, L_k after j steps: a step is a D-term fma chain (T_s) and a 2 D-term one:  C_ENV(j) = j (3 D + 1) against the
    absolute-value environment;  kappa_Z = Z_abs / Z.
  psi of a sample: n D-term chains: C_PSI = n D + 2 against psi_abs;  kappa_b = psi_abs / |psi|.
  logq = 2 log|l_n[0]| - log E^_0[0,0] + (2 el - eE[0]) ln 2:  2 C_PSI kappa_b + C_ENV(n) kappa_Z and the assembly: two
    logs, one product with ln 2 and three additions, each at most a unit of the largest partial result, which
    |log psi^2| + |log Z| + 4 bounds:  ASSEMBLE = 8 (|log psi^2| + |log Z| + 4).
  grad against grad_abs, C_SCORE = 1 + the larger of
    the sample term: l_{k-1} and r_k ((n - 1) D together), 1 / psi_b (C_PSI kappa_max), the quotient, the two products and
      the sum over samples: 64 terms in the matrix core per tile, the workgroup's tiles and the G partials in order:
      (n - 1) D + C_PSI kappa_max + 3 + 64 + tiles per workgroup + G;
    the environment term: L_{k-1} and E_k (C_ENV(n - 1) together), the two D-term chains, 1 / Z (C_ENV(n) kappa_Z), sum w
      (6 butterfly levels, the tiles, the G totals: 6 + tiles + ceil(G / 256) + 9) and four more operations.
The constants are not fitted: each test prints the worst ratio beside its C."""
import functools
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_mirror as mm
import mps_sampled_mirror as sm
from tensornetworks_amd import backend
from tensornetworks_amd.backend import mps_environments, mps_sample, mps_score_vjp, bn_logjoint_samples  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
SEED = 20240
# (n, D, B): every n, D and B of the lists above at least once
CASES = [(1, 1, 1), (1, 3, 63), (2, 2, 64), (3, 5, 65), (3, 17, 1), (12, 3, 257), (12, 16, 64), (12, 17, 65), (33, 2, 257),
         (33, 32, 64), (63, 4, 4099), (63, 16, 63), (63, 1, 65), (2, 32, 257)]
LANES, MAX_WG = 64, 256


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def make_cores(n, D, seed=0, spread=0.3):
    gen = torch.Generator().manual_seed(7000 * n + 13 * D + seed)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    return ((eye + spread * torch.randn(n, 2, D, D, dtype=torch.float64, generator=gen)) / math.sqrt(2.0)).contiguous()


def c_env(j, D):
    return float(j * (3 * D + 1))


def geometry(B):
    tiles = -(-B // LANES)
    G = min(tiles, MAX_WG)
    return G, -(-tiles // G)


def logq_bound(n, D, kappa_b, kappa_Z, logq, logZ):
    lpsi2 = np.where(np.isfinite(logq), logq + logZ, 0.0)
    return 2 * (n * D + 2) * kappa_b + c_env(n, D) * kappa_Z + 8 * (np.abs(lpsi2) + abs(logZ) + 4)


def c_score(n, D, B, kappa_max, kappa_Z):
    G, tiles = geometry(B)
    sample = (n - 1) * D + (n * D + 2) * kappa_max + 3 + 64 + tiles + G
    envt = c_env(n - 1, D) + 2 * D + c_env(n, D) * kappa_Z + 6 + tiles + (-(-G // 256)) + 9 + 4
    return 1.0 + max(sample, envt)


def workspace_view(n, D, B):
    """(E^ [n + 1, D, D], eE [n + 1], L^, eL) read back from the cached workspace (the layout of kernels_mps_sample.hip)."""
    d = dev()
    key = backend._ws_key(d, f"mps_sampled_{n}_{D}_{B}")
    buf = backend._workspaces[key]
    base = (-buf.data_ptr()) % 256
    up = lambda b: (b + 255) & ~255
    raw = buf.cpu().numpy()[base:]
    o = 256
    ne = (n + 1) * D * D
    E = raw[o:o + 8 * ne].view(np.float64).reshape(n + 1, D, D).copy(); o += up(8 * ne)
    L = raw[o:o + 8 * ne].view(np.float64).reshape(n + 1, D, D).copy(); o += up(8 * ne)
    eE = raw[o:o + 4 * (n + 1)].view(np.int32).copy(); o += up(4 * (n + 1))
    eL = raw[o:o + 4 * (n + 1)].view(np.int32).copy()
    return E, eE, L, eL


@functools.lru_cache(maxsize=None)
def sampled(n, D, B):
    """One run of environments + sample of a case and the mirror's evaluation on the GPU's own prefixes, shared by the tests."""
    cores = make_cores(n, D)
    c = cores.to(dev())
    ep = torch.tensor([3], dtype=torch.int64, device=dev())
    logZ = backend.mps_environments(c, B)
    idx, logq, status = backend.mps_sample(c, B, SEED, ep)
    torch.cuda.synchronize()
    envs = workspace_view(n, D, B)
    env = sm.environments(cores.numpy())
    bits = sm.bits_of_idx(idx.cpu().numpy(), n)
    cond = sm.conditionals(cores.numpy(), bits, env)
    return dict(cores=cores, logZ=float(logZ.item()), idx=idx.cpu().numpy(), logq=logq.cpu().numpy(), status=int(status.item()),
                envs=envs, env=env, bits=bits, cond=cond)


@pytest.mark.parametrize("n,D,B", CASES)
def test_environments_and_log_z(n, D, B):
    r = sampled(n, D, B)
    Eh, eE, Lh, eL = r["envs"]
    env = r["env"]
    worst = 0.0
    for k in range(n + 1):
        got_E = Eh[k].astype(sm.LD) * sm.LD(2.0) ** int(eE[k])
        got_L = Lh[k].astype(sm.LD) * sm.LD(2.0) ** int(eL[k])
        for got, ref, ab, C in ((got_E, env["E"][k], env["E_abs"][k], c_env(n - k, D)), (got_L, env["L"][k], env["L_abs"][k], c_env(k, D))):
            err = np.abs(got - ref)
            den = ab * sm.LD(EPS)
            if C == 0:
                assert np.all(err == 0)
                continue
            ratio = float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), np.where(err == 0, 0, np.inf)))) / C
            worst = max(worst, ratio)
        # power-of-two rescaling: the largest magnitude of a stored matrix lies in [1, 2)
        assert 1.0 <= np.abs(Eh[k]).max() < 2.0 and 1.0 <= np.abs(Lh[k]).max() < 2.0
    kZ = float(env["Z_abs"] / env["Z"])
    logZ_ref = float(np.log(env["Z"]))
    bound = EPS * (c_env(n, D) * kZ + 8 * (abs(logZ_ref) + 4))
    print(f"n={n} D={D}: worst environment ratio / C_ENV = {worst:.3f}; |logZ err| / bound = {abs(r['logZ'] - logZ_ref) / bound:.3f}")
    assert worst <= 1.0
    assert abs(r["logZ"] - logZ_ref) <= bound
    if n <= 12:
        _, _, _, Z = backend.mps_probs(r["cores"].to(dev()), want_q32=False)
        # exp(logZ) carries logZ's absolute error as a relative one (+ 2 for exp); Z of mps_probs errs by (2 C_PSI + 1) kappa + T_Z
        # (tests/test_gpu_mps_kernel.py; T_Z <= 29 for n <= 12)
        assert abs(math.exp(r["logZ"]) / float(Z.item()) - 1.0) <= bound + EPS * (2 + (2 * (n * D + 2) + 1) * kZ + 29)


@pytest.mark.parametrize("n,D,B", CASES)
def test_sampler_bits_and_logq(n, D, B):
    r = sampled(n, D, B)
    assert r["status"] == 0
    U = sm.uniforms(SEED, 3, np.arange(B), n)
    p1 = hp.to_f64(r["cond"]["p1"])
    # undecided: U within 2^-40 of p1 or of the decision boundary m_0 / (m_0 + m_1) = 1 - p1 (z_k = 1 iff U >= 1 - p1)
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
    ratio = np.abs(hp.to_f64(r["logq"].astype(sm.LD) - ref)) / (EPS * bound)
    print(f"n={n} D={D} B={B}: worst logq ratio = {ratio.max():.3f} (bound in units of eps: up to {bound.max():.0f})")
    assert ratio.max() <= 1.0
    if n <= 12:
        _, q64, _, _ = backend.mps_probs(r["cores"].to(dev()), want_q32=False)
        q = q64.cpu().numpy()[r["idx"]]
        # q of mps_probs, relative to itself (tests/test_gpu_mps_kernel.py: q_bound): (2 C_PSI + 1)(kappa_b + kappa_Z) + 2 + T_Z,
        # T_Z <= 29 for n <= 12, and the log's own rounding
        kq = (2 * (n * D + 2) + 1) * (kb + kZ) + 2 + 29 + 2 * np.abs(r["logq"])
        assert np.all(np.abs(r["logq"] - np.log(q)) <= EPS * (bound + kq))


def test_draws_do_not_depend_on_the_batch():
    n, D = 63, 4
    big = sampled(n, D, 4099)
    c = big["cores"].to(dev())
    ep = torch.tensor([3], dtype=torch.int64, device=dev())
    backend.mps_environments(c, 64)
    idx, logq, _ = backend.mps_sample(c, 64, SEED, ep)
    assert np.array_equal(idx.cpu().numpy(), big["idx"][:64]) and np.array_equal(logq.cpu().numpy(), big["logq"][:64])
    idx2, _, _ = backend.mps_sample(c, 64, SEED, ep)
    assert torch.equal(idx, idx2)                                   # two calls are bitwise equal
    other_epoch, _, _ = backend.mps_sample(c, 64, SEED, torch.tensor([4], dtype=torch.int64, device=dev()))
    other_seed, _, _ = backend.mps_sample(c, 64, SEED + 1, ep)
    assert not torch.equal(idx, other_epoch) and not torch.equal(idx, other_seed)


def test_power_of_two_scaling_and_status():
    """n = 63, D = 4: cores times 2^12 (2^-12) multiply psi^2 by 2^(+-1512): beyond float64 without the rescaling.  idx stays
    bitwise the same, logq within the bound.  A zero core: status != 0, idx 0, nothing non-finite outside logq."""
    n, D, B = 63, 4, 4099
    r = sampled(n, D, B)
    ep = torch.tensor([3], dtype=torch.int64, device=dev())
    env = r["env"]
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(r["cond"]["psi_abs"] / np.abs(r["cond"]["psi"]))
    for p in (12, -12):
        c = (r["cores"] * 2.0 ** p).to(dev())
        logZ = backend.mps_environments(c, B)
        idx, logq, status = backend.mps_sample(c, B, SEED, ep)
        assert int(status.item()) == 0 and np.array_equal(idx.cpu().numpy(), r["idx"])
        shift = 2 * n * p * math.log(2.0)
        assert abs(float(logZ.item()) - (float(np.log(env["Z"])) + shift)) <= EPS * (c_env(n, D) * kZ + 8 * (abs(shift) + abs(r["logZ"]) + 4))
        bound = logq_bound(n, D, kb, kZ, hp.to_f64(r["cond"]["logq"]), float(np.log(env["Z"])) + shift) + 16 * abs(shift)
        assert np.all(np.abs(hp.to_f64(logq.cpu().numpy().astype(sm.LD) - r["cond"]["logq"])) <= EPS * bound)
        grad, lq, st = backend.mps_score_vjp(c, idx, torch.ones(B, dtype=torch.float64, device=dev()) / B)
        assert int(st.item()) == 0 and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(lq).all())
    z = r["cores"].clone()
    z[40] = 0.0
    c = z.to(dev())
    logZ = backend.mps_environments(c, B)
    idx, logq, status = backend.mps_sample(c, B, SEED, ep)
    assert int(status.item()) != 0 and bool((idx == 0).all()) and float(logZ.item()) == -math.inf
    grad, lq, st = backend.mps_score_vjp(c, idx, torch.zeros(B, dtype=torch.float64, device=dev()))
    assert int(st.item()) != 0


SCORE_CASES = [(1, 1, 1), (1, 3, 63), (2, 2, 64), (3, 5, 65), (3, 17, 257), (12, 3, 4099), (12, 16, 257), (12, 32, 65), (33, 2, 257),
               (33, 17, 64), (63, 4, 257), (63, 16, 65), (63, 32, 1), (2, 5, 16500)]


def score_inputs(n, D, B):
    rng = np.random.default_rng([n, D, B, 5])
    bits = rng.integers(0, 2, size=(B, n))
    bits[0] = 0
    bits[-1] = 1
    if B > 8:
        bits[3] = bits[5] = bits[B // 2]           # repeated samples
    w = rng.standard_normal(B)
    return bits, w


@pytest.mark.parametrize("n,D,B", SCORE_CASES)
def test_score_vjp_against_the_mirror(n, D, B):
    cores = make_cores(n, D, seed=1)
    bits, w = score_inputs(n, D, B)
    idx = torch.from_numpy(sm.idx_of_bits(bits)).to(dev())
    wt = torch.from_numpy(w).to(dev())
    c = cores.to(dev())
    backend.mps_environments(c, B)
    grad, logq, status = backend.mps_score_vjp(c, idx, wt)
    grad2, logq2, _ = backend.mps_score_vjp(c, idx, wt)
    torch.cuda.synchronize()
    assert torch.equal(grad, grad2) and torch.equal(logq, logq2)                # bitwise reproducible
    assert int(status.item()) == 0
    env = sm.environments(cores.numpy())
    ref = sm.score_gradient(cores.numpy(), bits, w, env)
    kZ = float(env["Z_abs"] / env["Z"])
    kmax = float(ref["kappa"].max())
    C = c_score(n, D, B, kmax, kZ)
    g = grad.cpu().numpy()
    r, at = hp.worst(hp.ratio(g, ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    print(f"n={n} D={D} B={B}: worst grad ratio {r:.2f} at {at}, C_SCORE = {C:.0f} (kappa_max {kmax:.2f}, kappa_Z {kZ:.2f})")
    assert r <= C
    if D > 1:
        assert np.all(g[0][:, 1:, :] == 0.0) and np.all(g[n - 1][:, :, 1:] == 0.0)
    bound = logq_bound(n, D, hp.to_f64(ref["kappa"]), kZ, hp.to_f64(ref["logq"]), float(np.log(env["Z"])))
    assert np.all(np.abs(hp.to_f64(logq.cpu().numpy().astype(sm.LD) - ref["logq"])) <= EPS * bound)


def test_score_vjp_zero_amplitude():
    """A sample with psi = 0: logq -inf, no contribution to the sample term, status 2."""
    n, D = 4, 2
    cores = make_cores(n, D, seed=2)
    cores[1, 1] = 0.0                                   # every z with z_2 = 1 has psi = 0
    bits = np.array([[0, 0, 1, 0], [0, 1, 0, 1], [1, 0, 0, 1]])
    w = np.array([0.5, -2.0, 1.5])
    c = cores.to(dev())
    backend.mps_environments(c, 3)
    grad, logq, status = backend.mps_score_vjp(c, torch.from_numpy(sm.idx_of_bits(bits)).to(dev()), torch.from_numpy(w).to(dev()))
    assert int(status.item()) == 2 and float(logq[1].item()) == -math.inf and bool(torch.isfinite(logq[[0, 2]]).all())
    env = sm.environments(cores.numpy())
    ref = sm.score_gradient(cores.numpy(), bits, w, env)
    C = c_score(n, D, 3, float(ref["kappa"][[0, 2]].max()), float(env["Z_abs"] / env["Z"]))
    r, at = hp.worst(hp.ratio(grad.cpu().numpy(), ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    assert r <= C, (r, at)


@pytest.mark.parametrize("n,D", [(3, 3), (3, 16), (10, 3), (10, 16)])
def test_score_vjp_ties_to_the_enumerated_vjp(n, D):
    """score_vjp(idx = every outcome, w = q g) is mps_vjp(g): sum_z q_z g_z grad log q_z = grad sum_z q_z g_z, within the sum
    of the two derived bounds (w itself carries q's relative error C_Q)."""
    from test_gpu_mps_kernel import constants as mps_constants, make_inputs
    cores, g = make_inputs(n, D)
    c = cores.to(dev())
    N = 1 << n
    _, q64, _, _ = backend.mps_probs(c, want_q32=False)
    want = backend.mps_vjp(c, g.to(dev())).cpu().numpy()
    w = (q64 * g.to(dev())).contiguous()
    backend.mps_environments(c, N)
    got, _, status = backend.mps_score_vjp(c, torch.arange(N, dtype=torch.int64, device=dev()), w)
    assert int(status.item()) == 0
    ref = mm.reference(cores.numpy(), g.numpy())
    env = sm.environments(cores.numpy())
    sref = sm.score_gradient(cores.numpy(), mm.bits_of(n), w.cpu().numpy(), env)
    kappa = float(ref["Z_abs"] / ref["Z"])
    Cm = mps_constants(n, D, kappa)
    c_q = 2 * Cm["psi"] + 3 + (2 * Cm["psi"] + 1) * kappa + Cm["t_z"]
    Cs = c_score(n, D, N, float(sref["kappa"].max()), float(env["Z_abs"] / env["Z"])) + c_q
    bound = Cs * hp.to_f64(sref["grad_abs"]) + Cm["grad"] * hp.to_f64(ref["grad_abs"])
    err = np.abs(got.cpu().numpy() - want)
    print(f"n={n} D={D}: worst |score_vjp - mps_vjp| / bound = {np.max(err / (EPS * bound + 1e-300)):.3f}")
    assert np.all(err <= EPS * bound)


def _host_terms(packed, bits, p_floor=1e-30):
    """sum over the nodes of |log factor|: the scale of the rounding of a V-term sum of logs."""
    role, npar, par, off, cpt = (packed[k] for k in ("role", "n_parents", "parents", "cpt_off", "cpt"))
    V = len(role)
    vals = np.zeros((bits.shape[0], V), np.int64)
    for v in range(V):
        vals[:, v] = bits[:, role[v]] if role[v] >= 0 else (1 if role[v] == -2 else 0)
    tot = np.zeros(bits.shape[0])
    for v in range(V):
        cfg = np.zeros(bits.shape[0], np.int64)
        for p in range(npar[v]):
            cfg = cfg * 2 + vals[:, par[v, p]]
        tot += np.abs(np.log(np.maximum(cpt[off[v] + 2 * cfg + vals[:, v]], p_floor)))
    return V, tot


def _logjoint_case(bn, lat, x, bits, against_table):
    """Device log joint of `bits` against float64 host sums: a log is taken to within 2 units of its own size on either side
    and the V-term sum adds one per addition: (V + 4) eps sum |log factor|.  Against log(pxz) of bornvi_score_from_cpts, whose
    product of V factors carries V units: + (V + 2) eps."""
    from tensornetworks_amd.bayesian_network import pack_network
    n = len(lat)
    packed = pack_network(bn, lat, x)
    keep, desc = backend.bn_descriptor(packed, dev())
    idx = torch.from_numpy(sm.idx_of_bits(bits)).to(dev())
    got = backend.bn_logjoint_samples(desc, n, idx).cpu().numpy()
    V, tot = _host_terms(packed, bits)
    want = sm.log_joint(packed, bits)
    assert np.all(np.abs(got - want) <= EPS * (V + 4) * tot)
    if against_table:
        _, pxz = backend.score_from_packed(packed, n, dev())
        tab = np.log(pxz.cpu().numpy()[idx.cpu().numpy()])
        assert np.all(np.abs(got - tab) <= EPS * ((V + 4) * tot + V + 2))


def test_log_joint_of_samples():
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network, pack_network
    from tensornetworks_amd._ext import BornviError
    sp = get_sprinkler_network(False)
    for wv in (0, 1):
        _logjoint_case(sp, ['C', 'S', 'R'], {'W': wv}, mm.bits_of(3), True)
    bn, lat, obs, x = synthetic_network(12, 0)
    _logjoint_case(bn, lat, x, mm.bits_of(12), True)
    bn, lat, obs, x = synthetic_network(40, 0)
    rng = np.random.default_rng(40)
    bits = rng.integers(0, 2, size=(1000, 40))
    bits[0] = 0
    bits[1] = 1
    _logjoint_case(bn, lat, x, bits, False)
    keep, desc = backend.bn_descriptor(pack_network(sp, ['C', 'S'], {'W': 1}), dev())       # R is summed out
    with pytest.raises(BornviError, match="summed-out"):
        backend.bn_logjoint_samples(desc, 2, torch.zeros(4, dtype=torch.int64, device=dev()))


def test_refused_sizes():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    assert lib.bornvi_mps_sample_workspace_bytes(h.h, 64, 4, 8) == 0 and lib.bornvi_mps_sample_workspace_bytes(h.h, 8, 33, 8) == 0
    assert lib.bornvi_mps_sample_workspace_bytes(h.h, 8, 4, 0) == 0 and lib.bornvi_mps_sample_workspace_bytes(h.h, 8, 4, (1 << 24) + 1) == 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev())
    rc = lib.bornvi_mps_environments(h.h, 64, 4, 8, buf.data_ptr(), None, buf.data_ptr(), buf.numel(), None)
    assert rc == -4
    # the workspace does not grow with B beyond 256 tiles of 64 samples
    assert lib.bornvi_mps_sample_workspace_bytes(h.h, 63, 16, 1 << 24) == lib.bornvi_mps_sample_workspace_bytes(h.h, 63, 16, 256 * 64)


def test_capture_and_replay():
    """One graph of environments + sample + score_vjp; epoch_dev changes between the replays; equal to the eager calls."""
    n, D, B = 12, 5, 257
    c = make_cores(n, D, seed=3).to(dev())
    ep = torch.zeros(1, dtype=torch.int64, device=dev())
    w = torch.from_numpy(np.random.default_rng(1).standard_normal(B)).to(dev())
    eager = {}
    for e in (0, 1, 2):
        ep.fill_(e)
        backend.mps_environments(c, B)
        idx, logq, _ = backend.mps_sample(c, B, SEED, ep)
        grad, _, _ = backend.mps_score_vjp(c, idx, w)
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
        backend.mps_environments(c, B)                         # the side stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.mps_environments(c, B)
        backend.mps_sample(c, B, SEED, ep, out_idx=idx, out_logq=logq, status=st1)
        backend.mps_score_vjp(c, idx, w, out=grad, out_logq=lq2, status=st2)
    for e in (2, 0, 1):
        ep.fill_(e)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, eager[e][0]) and torch.equal(logq, eager[e][1]) and torch.equal(grad, eager[e][2])
        assert int(st1.item()) == 0 and int(st2.item()) == 0
