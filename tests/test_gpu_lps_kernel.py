"""bornvi_lps_environments / _sample / _score_vjp (locally purified cores, kernels_lps.hip) against the extended-precision
mirror (lps_mirror.py), per entry the hp_reference.ratio way, and their contract: draws replayed from aux, the NULL aux and the
NULL gradient, the sampler's frequencies, the real family at m = 1, bitwise reproducible, independent of the batch, capturable,
exact power-of-two rescaling, the status word, refused sizes.

Shapes (n, m, D, B): (1, 1, 1, 64) the smallest; (3, 2, 2, 65) a second sampler tile with one sample; (5, 3, 3, 257) odd D and m,
padding in both; (12, 2, 8, 257) mid size; (6, 4, 16, 130) both maxima; (63, 2, 4, 4099) the largest n, both aux words;
(63, 1, 2, 64 G_max + 65), G_max = 1024 workgroups at D <= 8: the score kernel's tiles (16 samples) wrap past the grid.

Error bounds, derived from the kernels' operation chains (units of EPS64 = 2^-52, every rounding counted as a whole unit; the
power-of-two rescalings add none), against the majorants of lps_mirror.py (the same recursions over |cores|):
  E_k, L_k after j steps: per step a D-term chain (T_j = A_j X), a 2 m D-term chain (j outer, d inner) and the store:
    C_ENV(j) = j ((2 m + 1) D + 1);  kappa_Z = Z_abs / Z.
  A density after j steps: per step the product rho A_mu (D non-zero terms of the 16: the zero padding adds exact zeros) and
    the sum over mu of A_mu^T Y (m D terms), both on the matrix cores, whose order of summation inside a K-step of 4 is not
    stated: every term is counted twice (once for the sum of products, once for the accumulation):  C_T(j) = 2 j D (m + 1).
    The kernel runs X -> sum_mu A^T X^T A on the stored tile; X^T differs from X by earlier roundings only, which this count
    already carries (the recursion is linear in X): no term is added for it, and nothing is symmetrised.  kappa_b = T_abs / T.
  logq = log rho^_n[0,0] - log E^_0[0,0] + (e_rho - eE[0]) ln 2:  C_T(n) kappa_b + C_ENV(n) kappa_Z and the assembly: two logs,
    one product with ln 2 and three additions, each at most a unit of the largest partial result:  8 (|log T| + |log Z| + 4).
  grad against grad_abs, C_SCORE = 1 + the larger of
    the sample term: rho_{k-1} and R_k (C_T(n - 1) together), c = 2 w / T (C_T(n) kappa_max, the quotient and the product with
      rho: 3), W = A R_k (2 D), and the sum over samples: a wave's long-K product over its 4 samples of a tile, 4 D terms
      (2 . 4 D), then per tile the 4 waves' tiles added one after the other into the workgroup's partial (4 additions a
      tile of the workgroup), and the G partials in order:  C_T(n - 1) + C_T(n) kappa_max + 3 + 2 D + 8 D + 4 tiles + G;
    the environment term: L_{k-1} and E_k (C_ENV(n - 1) together), the two D-term chains (2 D), 1 / Z (C_ENV(n) kappa_Z),
      sum w (16 additions per tile, 6 butterfly levels, ceil(G / 256) and 3 more) and four more operations.
  The gradient's bound goes through hp.measured_constant: max(16, 8 x what the float64 mirror shows on the same samples), never
  above C_SCORE.  Nothing is fitted to the device: each test prints the worst ratio beside its C."""
import functools
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import lps_mirror as lp
import mps_sampled_mirror as sm
from lps_mirror import c_env, c_score, geometry, logq_bound          # the counts derived above, as functions
from tensornetworks_amd import backend

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
SEED = 20250
EPOCH = 3
G_MAX = lp.MAX_WG_SMALL
CASES = [(1, 1, 1, 64), (3, 2, 2, 65), (5, 3, 3, 257), (12, 2, 8, 257), (6, 4, 16, 130), (63, 2, 4, 4099), (63, 1, 2, 64 * G_MAX + 65)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def make_cores(n, m, D, seed=0):
    return torch.from_numpy(lp.random_cores(n, m, D, 9000 * n + 170 * m + 17 * D + seed)).contiguous()


def epoch_tensor(e=EPOCH):
    return torch.tensor([e], dtype=torch.int64, device=dev())


def workspace_view(n, m, D, B):
    """(E^ [n + 1, D, D], eE [n + 1], L^, eL) read back from the cached workspace (the layout of kernels_lps.hip)."""
    d = dev()
    buf = backend._workspaces[backend._ws_key(d, f"lps_{n}_{m}_{D}_{B}")]
    base = (-buf.data_ptr()) % 256
    up = lambda b: (b + 255) & ~255
    ne = (n + 1) * D * D
    raw = buf[base:base + 256 + 2 * up(8 * ne) + 2 * up(4 * (n + 1))].cpu().numpy()
    o = 256
    out = []
    for _ in range(2):
        out.append(raw[o:o + 8 * ne].view(np.float64).reshape(n + 1, D, D).copy())
        o += up(8 * ne)
    eE = raw[o:o + 4 * (n + 1)].view(np.int32).copy(); o += up(4 * (n + 1))
    eL = raw[o:o + 4 * (n + 1)].view(np.int32).copy()
    return out[0], eE, out[1], eL


@functools.lru_cache(maxsize=None)
def sampled(n, m, D, B):
    """One run of environments + sample + score_vjp of a case, shared by the tests (the reference is computed once)."""
    cores = make_cores(n, m, D)
    c = cores.to(dev())
    w = np.random.default_rng([n, m, D, B, 5]).standard_normal(B)
    wt = torch.from_numpy(w).to(dev())
    logZ = backend.lps_environments(c, B)
    idx, aux, status = backend.lps_sample(c, B, SEED, epoch_tensor(), want_aux=True)
    grad, logq, st2 = backend.lps_score_vjp(c, idx, wt)
    torch.cuda.synchronize()
    envs = workspace_view(n, m, D, B)
    env = lp.environments(cores.numpy())
    idx_h = idx.cpu().numpy()
    return dict(cores=cores, c=c, w=w, wt=wt, logZ=float(logZ.item()), idx=idx_h, idx_dev=idx, aux=aux.cpu().numpy(), status=int(status.item()),
                grad=grad.cpu().numpy(), grad_dev=grad, logq=logq.cpu().numpy(), logq_dev=logq, status_score=int(st2.item()), envs=envs, env=env,
                bits=lp.bits_of_idx(idx_h, n))


@pytest.mark.parametrize("n,m,D,B", CASES)
def test_environments_and_log_z(n, m, D, B):
    r = sampled(n, m, D, B)
    Eh, eE, Lh, eL = r["envs"]
    env = r["env"]
    worst = 0.0
    for k in range(n + 1):
        for mat, ex, ref, ab, C in ((Eh[k], eE[k], env["E"][k], env["E_abs"][k], c_env(n - k, m, D)),
                                    (Lh[k], eL[k], env["L"][k], env["L_abs"][k], c_env(k, m, D))):
            assert 1.0 <= np.abs(mat).max() < 2.0          # the power-of-two rescaling: the largest magnitude lies in [1, 2)
            err = np.abs(mat.astype(lp.LD) * lp.LD(2.0) ** int(ex) - ref)
            if C == 0:
                assert np.all(err == 0)
                continue
            den = ab * lp.LD(EPS)
            ratio = float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), np.where(err == 0, 0, np.inf)))) / C
            worst = max(worst, ratio)
    kZ = float(env["Z_abs"] / env["Z"])
    logZ_ref = float(np.log(env["Z"]))
    bound = EPS * (c_env(n, m, D) * kZ + 8 * (abs(logZ_ref) + 4))
    print(f"n={n} m={m} D={D}: worst environment ratio / C_ENV = {worst:.3f}; |logZ err| / bound = {abs(r['logZ'] - logZ_ref) / bound:.3f}")
    assert worst <= 1.0
    assert abs(r["logZ"] - logZ_ref) <= bound


@pytest.mark.parametrize("n,m,D,B", CASES)
def test_draws_against_the_mirror(n, m, D, B):
    """Every drawn (z_k, mu_k) equals the mirror's decision on the GPU's own prefix, read from aux."""
    r = sampled(n, m, D, B)
    assert r["status"] == 0
    mus = lp.mus_of_aux(r["aux"], n)
    assert mus.max() <= m - 1 and (n > 32 or not r["aux"][:, 1].any())
    assert np.array_equal(lp.aux_of_mus(mus), r["aux"])                    # no bit outside the sites' fields
    masses = lp.masses_on_prefix(r["cores"].numpy(), r["bits"], mus, r["env"])
    U = lp.uniforms(SEED, EPOCH, np.arange(B), n)
    undecided = 0
    for k in range(n):
        z, mu, und = lp.decide(masses[k], U[:, k])
        undecided += und
        assert np.array_equal(z, r["bits"][:, k]) and np.array_equal(mu, mus[:, k]), k
    assert undecided == 0
    if m > 1:
        assert mus.any()
    assert np.all(r["idx"] >= 0) and (n == 63 or np.all(r["idx"] < (1 << n)))


@pytest.mark.parametrize("n,m,D,B", CASES)
def test_logq_and_gradient_against_the_mirror(n, m, D, B):
    r = sampled(n, m, D, B)
    cores, bits, w, env = r["cores"].numpy(), r["bits"], r["w"], r["env"]
    assert r["status_score"] == 0 and r["grad"].shape == (n, 2, m, D, D)
    ref = lp.score_gradient(cores, bits, w, env)
    f64 = lp.score_gradient(cores, bits, w, dtype=np.float64)
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(ref["kappa"])
    bound = logq_bound(n, m, D, kb, kZ, hp.to_f64(ref["logq"]), float(np.log(env["Z"])))
    lr = np.abs(hp.to_f64(r["logq"].astype(lp.LD) - ref["logq"])) / (EPS * bound)
    oracle, _ = hp.worst(hp.ratio(f64["grad"], ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    derived = c_score(n, m, D, B, float(kb.max()), kZ)
    C = hp.measured_constant(oracle, derived)
    g = r["grad"]
    gr, at = hp.worst(hp.ratio(g, ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    print(f"n={n} m={m} D={D} B={B}: worst logq ratio {lr.max():.3f} (bound up to {bound.max():.0f} eps); worst grad ratio {gr:.2f} at {at}, "
          f"C = {C:.0f} (float64 mirror {oracle:.2f}, derived {derived:.0f}, kappa_max {kb.max():.2f}, kappa_Z {kZ:.2f})")
    assert lr.max() <= 1.0
    assert C <= derived and gr <= C
    if D > 1:      # entries of the first and last core that do not enter psi: exactly 0.0
        assert np.all(g[0][:, :, 1:] == 0.0) and np.all(g[n - 1][:, :, :, 1:] == 0.0)


@pytest.mark.parametrize("n,m,D,B", CASES[:6])
def test_null_aux_null_gradient_and_repeats(n, m, D, B):
    """aux = NULL gives the same idx; a NULL grad_cores the same logq bits; two calls are bitwise equal."""
    r = sampled(n, m, D, B)
    c = r["c"]
    backend.lps_environments(c, B)
    idx, aux, st = backend.lps_sample(c, B, SEED, epoch_tensor())
    assert aux is None and int(st.item()) == 0 and np.array_equal(idx.cpu().numpy(), r["idx"])
    idx2, aux2, _ = backend.lps_sample(c, B, SEED, epoch_tensor(), want_aux=True)
    assert torch.equal(idx, idx2) and np.array_equal(aux2.cpu().numpy(), r["aux"])
    none, logq, st = backend.lps_score_vjp(c, idx, out=False)
    assert none is None and int(st.item()) == 0 and torch.equal(logq, r["logq_dev"])
    grad, logq2, _ = backend.lps_score_vjp(c, idx, r["wt"])
    assert torch.equal(grad, r["grad_dev"]) and torch.equal(logq2, r["logq_dev"])
    other_epoch, _, _ = backend.lps_sample(c, B, SEED, epoch_tensor(EPOCH + 1))
    other_seed, _, _ = backend.lps_sample(c, B, SEED + 1, epoch_tensor())
    if n * B >= 64:
        assert not torch.equal(idx, other_epoch) and not torch.equal(idx, other_seed)


def test_sample_b_does_not_depend_on_the_batch():
    n, m, D = 63, 2, 4
    big = sampled(n, m, D, 4099)
    c = big["c"]
    for B in (1, 17, 64, 130):
        backend.lps_environments(c, B)
        idx, aux, _ = backend.lps_sample(c, B, SEED, epoch_tensor(), want_aux=True)
        _, logq, _ = backend.lps_score_vjp(c, idx, out=False)
        assert np.array_equal(idx.cpu().numpy(), big["idx"][:B]) and np.array_equal(aux.cpu().numpy(), big["aux"][:B])
        assert np.array_equal(logq.cpu().numpy(), big["logq"][:B])


def test_sampler_frequencies():
    """(4, 2, 3, 2^16): the frequencies of the 16 outcomes within 5 standard errors of the exact q; the seed is the one with
    which test_lps_host.py::test_mirror_sampler_frequencies shows that the mirror's own sampler satisfies this."""
    n, m, D, B = 4, 2, 3, 1 << 16
    cores = lp.random_cores(n, m, D, 21)
    c = torch.from_numpy(cores).to(dev())
    backend.lps_environments(c, B)
    idx, _, st = backend.lps_sample(c, B, lp.FREQ_SEED, epoch_tensor(0))
    assert int(st.item()) == 0
    _, q = lp.brute_force(cores)
    q = hp.to_f64(q)
    freq = np.bincount(idx.cpu().numpy(), minlength=16) / B
    zs = np.abs(freq - q) / np.sqrt(q * (1 - q) / B)
    print(f"sampler frequencies: worst |freq - q| / standard error = {zs.max():.2f}")
    assert zs.max() <= 5.0
    # and log_prob over all 16 states is that q
    _, logq, _ = backend.lps_score_vjp(c[:, :, :, :, :].contiguous(), torch.arange(16, dtype=torch.int64, device=dev()).repeat(B // 16), out=False)
    assert np.all(np.abs(np.exp(logq[:16].cpu().numpy()) - q) <= 1e-13)


# ---- m = 1: the real family -------------------------------------------------------------------------------------------------
def real_c_env(j, D):
    return float(j * (3 * D + 1))


def real_logq_bound(n, D, kappa_b, kappa_Z, logq, logZ):
    lpsi2 = np.where(np.isfinite(logq), logq + logZ, 0.0)
    return 2 * (n * D + 2) * kappa_b + real_c_env(n, D) * kappa_Z + 8 * (np.abs(lpsi2) + abs(logZ) + 4)


def real_c_score(n, D, B, kappa_max, kappa_Z):
    tiles = -(-B // 64)
    G = min(tiles, 256)
    tiles = -(-tiles // G)
    sample = (n - 1) * D + (n * D + 2) * kappa_max + 3 + 64 + tiles + G
    envt = real_c_env(n - 1, D) + 2 * D + real_c_env(n, D) * kappa_Z + 6 + tiles + (-(-G // 256)) + 9 + 4
    return 1.0 + max(sample, envt)


@pytest.mark.parametrize("n,D,B", [(12, 8, 257), (63, 4, 4099)])
def test_m_equal_one_is_the_real_family(n, D, B):
    """No index differs from bornvi_mps_sample's on the same cores (the environments and the sampler's chains are the same
    bits); logq and the gradient agree with bornvi_mps_score_vjp within the sum of the two bounds (the real calls' bounds are
    those of test_gpu_mps_sampled_kernel.py, restated above)."""
    real = make_cores(n, 1, D, seed=1)[:, :, 0].contiguous()
    cr, cp = real.to(dev()), real[:, :, None].contiguous().to(dev())
    ep = epoch_tensor()
    w = torch.from_numpy(np.random.default_rng([n, D, B]).standard_normal(B)).to(dev())
    lZr = backend.mps_environments(cr, B)
    ir, lqr, sr = backend.mps_sample(cr, B, SEED, ep)
    gr, lqr2, sr2 = backend.mps_score_vjp(cr, ir, w)
    lZp = backend.lps_environments(cp, B)
    ip, _, sp = backend.lps_sample(cp, B, SEED, ep)
    gp, lqp, sp2 = backend.lps_score_vjp(cp, ir, w)
    torch.cuda.synchronize()
    assert int(sr.item()) == int(sp.item()) == 0 and int(sr2.item()) == int(sp2.item()) == 0
    assert float(lZr.item()) == float(lZp.item())                          # the same chains: the same bits
    assert torch.equal(ir, ip)
    bits = sm.bits_of_idx(ir.cpu().numpy(), n)
    env = sm.environments(real.numpy())
    ref = sm.score_gradient(real.numpy(), bits, w.cpu().numpy(), env)
    refp = lp.score_gradient(real[:, :, None].numpy(), bits, w.cpu().numpy())
    kZ = float(env["Z_abs"] / env["Z"])
    kb, kp = hp.to_f64(ref["kappa"]), hp.to_f64(refp["kappa"])
    logZ = float(np.log(env["Z"]))
    both = real_logq_bound(n, D, kb, kZ, hp.to_f64(ref["logq"]), logZ) + logq_bound(n, 1, D, kp, kZ, hp.to_f64(ref["logq"]), logZ)
    assert np.all(np.abs(lqr2.cpu().numpy() - lqp.cpu().numpy()) <= EPS * both)
    assert np.all(np.abs(lqr.cpu().numpy() - lqp.cpu().numpy()) <= EPS * both)
    err = np.abs(gp.cpu().numpy()[:, :, 0] - gr.cpu().numpy())
    bound = EPS * (real_c_score(n, D, B, float(kb.max()), kZ) * hp.to_f64(ref["grad_abs"])
                   + c_score(n, 1, D, B, float(kp.max()), kZ) * hp.to_f64(refp["grad_abs"][:, :, 0]))
    print(f"n={n} D={D} B={B}: worst |purified grad - real grad| / bound = {np.max(err / np.where(bound > 0, bound, 1)):.3f}")
    assert np.all(err <= bound)


# ---- contract -------------------------------------------------------------------------------------------------------------------
def test_power_of_two_scaling_changes_no_index():
    """n = 63, D = 4, m = 2: cores times 2^12 (2^-12) multiply T by 2^(+-1512): beyond float64 without the rescaling.  idx and
    aux stay bitwise the same, logq within the bound, the gradient finite."""
    n, m, D, B = 63, 2, 4, 4099
    r = sampled(n, m, D, B)
    env = r["env"]
    kZ = float(env["Z_abs"] / env["Z"])
    ref = lp.logq_of(r["cores"].numpy(), r["bits"], env)
    for p in (12, -12):
        c = (r["cores"] * 2.0 ** p).to(dev())
        logZ = backend.lps_environments(c, B)
        idx, aux, status = backend.lps_sample(c, B, SEED, epoch_tensor(), want_aux=True)
        assert int(status.item()) == 0 and np.array_equal(idx.cpu().numpy(), r["idx"]) and np.array_equal(aux.cpu().numpy(), r["aux"])
        shift = 2 * n * p * math.log(2.0)
        assert abs(float(logZ.item()) - (float(np.log(env["Z"])) + shift)) <= EPS * (c_env(n, m, D) * kZ + 8 * (abs(shift) + abs(r["logZ"]) + 4))
        grad, lq, st = backend.lps_score_vjp(c, idx, torch.ones(B, dtype=torch.float64, device=dev()) / B)
        bound = logq_bound(n, m, D, hp.to_f64(ref["kappa"]), kZ, hp.to_f64(ref["logq"]), float(np.log(env["Z"])) + shift) + 16 * abs(shift)
        assert np.all(np.abs(hp.to_f64(lq.cpu().numpy().astype(lp.LD) - ref["logq"])) <= EPS * bound)
        assert int(st.item()) == 0 and bool(torch.isfinite(grad).all())


def test_zero_mass_and_status():
    """A zero site: status 1 from the sampler (idx and aux 0), log Z -inf, status 2 from the score call.  A sample with T = 0:
    logq -inf, no contribution to the sample term, status 2."""
    n, m, D, B = 12, 2, 3, 65
    z = make_cores(n, m, D).clone()
    z[7] = 0.0
    c = z.to(dev())
    logZ = backend.lps_environments(c, B)
    idx, aux, status = backend.lps_sample(c, B, SEED, epoch_tensor(), want_aux=True)
    assert int(status.item()) == 1 and bool((idx == 0).all()) and bool((aux == 0).all()) and float(logZ.item()) == -math.inf
    _, lq, st = backend.lps_score_vjp(c, idx, torch.zeros(B, dtype=torch.float64, device=dev()))
    assert int(st.item()) == 2
    n, m, D = 4, 2, 2
    cores = make_cores(n, m, D, seed=2)
    cores[1, 1] = 0.0                                   # every z with z_2 = 1 has T = 0
    bits = np.array([[0, 0, 1, 0], [0, 1, 0, 1], [1, 0, 0, 1]])
    w = np.array([0.5, -2.0, 1.5])
    c = cores.to(dev())
    backend.lps_environments(c, 3)
    grad, logq, status = backend.lps_score_vjp(c, torch.from_numpy(lp.idx_of_bits(bits)).to(dev()), torch.from_numpy(w).to(dev()))
    assert int(status.item()) == 2 and float(logq[1].item()) == -math.inf and bool(torch.isfinite(logq[[0, 2]]).all())
    env = lp.environments(cores.numpy())
    ref = lp.score_gradient(cores.numpy(), bits, w, env)
    C = c_score(n, m, D, 3, float(ref["kappa"][[0, 2]].max()), float(env["Z_abs"] / env["Z"]))
    r, at = hp.worst(hp.ratio(grad.cpu().numpy(), ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    assert r <= C, (r, at)


@pytest.mark.parametrize("value", [math.inf, math.nan], ids=["inf", "nan"])
def test_non_finite_core_entry(value):
    """The real contract for a non-finite number (an input case), n = 12, m = 2, D = 3, one Inf or NaN in A_8[0, 1][0, 0]: log Z
    is not finite; every environment left of the site is non-finite, so every sample meets a mass that is not finite at its
    first site: status 1, every bit and mu 0; the score call finds no sample that counts (E_0[0, 0] is not finite and
    positive): status 2 and no finite logq, the samples whose amplitudes avoid the entry included.  The calls return."""
    n, m, D, B = 12, 2, 3, 65
    bad = make_cores(n, m, D).clone()
    bad[7, 0, 1, 0, 0] = value
    c = bad.to(dev())
    logZ = backend.lps_environments(c, B)
    idx, aux, status = backend.lps_sample(c, B, SEED, epoch_tensor(), want_aux=True)
    assert not math.isfinite(float(logZ.item()))
    assert int(status.item()) == 1 and bool((idx == 0).all()) and bool((aux == 0).all())
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 2, size=(B, n))
    bits[0, 7], bits[1, 7] = 0, 1                        # z_8 = 0 reads the entry, z_8 = 1 does not
    w = torch.from_numpy(rng.standard_normal(B)).to(dev())
    it = torch.from_numpy(lp.idx_of_bits(bits)).to(dev())
    grad, lq, st = backend.lps_score_vjp(c, it, w)
    assert int(st.item()) == 2 and not bool(torch.isfinite(lq).any())
    assert tuple(grad.shape) == (n, 2, m, D, D)
    _, lq0, st0 = backend.lps_score_vjp(c, it, out=False)
    assert int(st0.item()) == 2 and not bool(torch.isfinite(lq0).any())
    # the same calls on the sound cores afterwards: nothing of the bad run is left in the workspace
    good = make_cores(n, m, D).to(dev())
    assert math.isfinite(float(backend.lps_environments(good, B).item()))
    idx, _, status = backend.lps_sample(good, B, SEED, epoch_tensor())
    _, lq, st = backend.lps_score_vjp(good, idx, out=False)
    assert int(status.item()) == 0 and int(st.item()) == 0 and bool(torch.isfinite(lq).all())
    backend.lps_environments(good, 257)
    ref, _, _ = backend.lps_sample(good, 257, SEED, epoch_tensor())
    assert torch.equal(idx, ref[:B])


def test_refused_sizes_leave_everything_untouched():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    UNSUPPORTED = _ext._ENUMS["BORNVI_ERR_UNSUPPORTED"]
    size = lib.bornvi_lps_workspace_bytes
    for n, m, D, B in ((0, 2, 4, 8), (64, 2, 4, 8), (8, 0, 4, 8), (8, 5, 4, 8), (8, 2, 0, 8), (8, 2, 17, 8), (8, 2, 4, 0), (8, 2, 4, (1 << 24) + 1)):
        assert size(h.h, n, m, D, B) == 0
    # the workspace does not grow with B beyond G_max tiles of 16 samples, and the largest cases stay near 1 GiB
    assert size(h.h, 63, 4, 16, 1 << 24) == size(h.h, 63, 4, 16, lp.MAX_WG_LARGE * 16) > size(h.h, 63, 4, 16, lp.MAX_WG_LARGE * 16 - 16)
    assert size(h.h, 63, 4, 8, 1 << 24) == size(h.h, 63, 4, 8, lp.MAX_WG_SMALL * 16) > size(h.h, 63, 4, 8, lp.MAX_WG_SMALL * 16 - 16)
    assert max(size(h.h, 63, 4, 16, 1 << 24), size(h.h, 63, 4, 8, 1 << 24)) <= (1 << 30)
    n, m, D, B = 8, 2, 4, 8
    need = size(h.h, n, m, D, B)
    canary = lambda count, dtype: torch.full((count,), 77, dtype=dtype, device=dev())
    ws, cores = canary(need, torch.uint8), make_cores(n, m, D).to(dev())
    idx, aux, logq, grad = canary(B, torch.int64), canary(2 * B, torch.int64), canary(B, torch.float64), canary(cores.numel(), torch.float64)
    st, lz = canary(1, torch.int32), canary(1, torch.float64)
    w, ep = torch.ones(B, dtype=torch.float64, device=dev()), torch.zeros(1, dtype=torch.int64, device=dev())
    P = lambda t: t.data_ptr()
    for nn, mm, DD, BB, bytes_ in ((0, m, D, B, need), (64, m, D, B, need), (n, 0, D, B, need), (n, 5, D, B, need), (n, m, 0, B, need),
                                   (n, m, 17, B, need), (n, m, D, 0, need), (n, m, D, (1 << 24) + 1, need), (n, m, D, B, need - 1), (n, m, D, B, 0)):
        assert lib.bornvi_lps_environments(h.h, nn, mm, DD, BB, P(cores), P(lz), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_lps_sample(h.h, nn, mm, DD, BB, P(cores), 1, P(ep), P(idx), P(aux), P(st), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_lps_score_vjp(h.h, nn, mm, DD, BB, P(cores), P(idx), P(w), P(logq), P(grad), P(st), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_lps_score_vjp(h.h, nn, mm, DD, BB, P(cores), P(idx), None, P(logq), None, P(st), P(ws), bytes_, None) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (ws, idx, aux, logq, grad, st, lz):
        assert bool((t == 77).all())


def test_capture_and_replay():
    """The three calls captured into one graph (a single chain, no branches) and replayed once give the eager bits."""
    n, m, D, B = 12, 3, 5, 257
    c = make_cores(n, m, D, seed=3).to(dev())
    ep = epoch_tensor(1)
    w = torch.from_numpy(np.random.default_rng(1).standard_normal(B)).to(dev())
    backend.lps_environments(c, B)
    idx0, aux0, _ = backend.lps_sample(c, B, SEED, ep, want_aux=True)
    grad0, logq0, _ = backend.lps_score_vjp(c, idx0, w)
    eager = (idx0.clone(), aux0.clone(), grad0.clone(), logq0.clone())
    idx = torch.empty(B, dtype=torch.int64, device=dev())
    aux = torch.empty(B, 2, dtype=torch.int64, device=dev())
    logq = torch.empty(B, dtype=torch.float64, device=dev())
    grad = torch.empty_like(c)
    st1 = torch.empty(1, dtype=torch.int32, device=dev())
    st2 = torch.empty(1, dtype=torch.int32, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        backend.lps_environments(c, B)                         # the side stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.lps_environments(c, B)
        backend.lps_sample(c, B, SEED, ep, out_idx=idx, out_aux=aux, status=st1)
        backend.lps_score_vjp(c, idx, w, out=grad, out_logq=logq, status=st2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager[0]) and torch.equal(aux, eager[1]) and torch.equal(grad, eager[2]) and torch.equal(logq, eager[3])
    assert int(st1.item()) == 0 and int(st2.item()) == 0
