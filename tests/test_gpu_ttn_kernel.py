"""bornvi_ttn_environments / _sample / _score_vjp (tree tensor network, kernels_ttn.hip) against the extended-precision mirror
(ttn_mirror.py), per entry the hp_reference.ratio way, and their contract: draws on the GPU's own prefix, the sampler's logq
equal to the score call's bit for bit, the NULL gradient, bitwise reproducible, independent of the batch, capturable, exact
power-of-two rescaling, the status word, refused sizes, the sampler's frequencies.

Shapes (n, D, B): (1, 2, 64) L = 2, one padding position; (2, 2, 65); (3, 2, 65) a bottom node with one padding child;
(5, 3, 257) odd D, zero-padded to the D = 4 instance, and an all-padding bottom node; (8, 4, 257) a full tree; (13, 8, 130) the
largest D, the density stack in the workspace; (33, 4, 257) L = 64 with whole all-padding subtrees; (63, 2, 4099); (63, 8, 257).

Error bounds, derived from the kernels' operation chains (units of EPS64 = 2^-52, every rounding counted as a whole unit; the
power-of-two rescalings add none), against the majorants of ttn_mirror.py (the same recursions over |cores|).  t is a node's
height above the positions (bottom nodes 1, the root h), d its depth (the root 0); a position's vector and density are exact.
  x_v: per node the chain M = T x_l over a (D terms) and the chain M x_r over b (D terms), and the errors of both children, which
    add because x_v is bilinear in them:  C_X(t) = 2 D + 2 C_X(t - 1) = 2 D (2^t - 1);  kappa_b = psi_abs / |psi|.
  U_v: per node the chains A (D terms), W (D terms) and U (D^2 terms), and both children's errors:  C_U(t) = (D^2 + 2 D)(2^t - 1);
    kappa_Z = Z_abs / Z.
  V_v: per step down the chain Y over p (D terms), whose operands carry V's error and that of R = T U_sibling (a D-term chain and
    C_U of the sibling's height), and the D^2-term chain:  C_V(d) = sum_{k < d} (2 D + D^2 + C_U(h - k - 1)).
  y_v: per step down the chain N over p (D terms) and the chain with the sibling's x (D terms and C_X of the sibling's height):
    C_Y(d) = sum_{k < d} (2 D + C_X(h - k - 1)).
  logq = 2 log|x^_1[0]| - log U^_1[0, 0] + (2 ex_1 - eU_1) ln 2:  2 C_X(h) kappa_b + C_U(h) kappa_Z and the assembly: two logs,
    one product with ln 2 and three additions, each at most a unit of the largest partial result:  8 (|log psi^2| + |log Z| + 4).
  grad against grad_abs, C_SCORE = 1 + the larger, over the depths d, of
    the sample term: c = 2 w / psi (C_X(h) kappa_max, the quotient and the product with y: 2), y_v (C_Y(d)), the product
      x_l[a] x_r[b] (1 and twice C_X(h - d - 1)), the long-K product on the matrix cores over the workgroup's 64 tiles samples,
      whose order inside a K-step of 4 is not stated: every term counted twice (2 . 64 tiles), and the G partials in order;
    the environment term: V_v (C_V(d)), the D-term chain over p', W_v (2 D and twice C_U(h - d - 1)), 1 / Z (1 and
      C_U(h) kappa_Z), sum w (an addition per tile, 6 butterfly levels, ceil(G / 256) per thread, 6 levels and 3 wave totals),
      the product and the difference.
  The gradient's bound goes through hp.measured_constant: max(16, 8 x what the float64 mirror shows on the same samples), never
  above C_SCORE.  Nothing is fitted to the device: each test prints the worst ratio beside its C."""
import functools
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import ttn_mirror as tt
from ttn_mirror import c_score, c_u, c_v, logq_bound          # the counts derived above, as functions
from tensornetworks_amd import backend

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
SEED = 20250          # chosen on the CPU: the mirror's own sampler has no undecided draw at any case (asserted below on the GPU's prefix)
EPOCH = 3
CASES = [(1, 2, 64), (2, 2, 65), (3, 2, 65), (5, 3, 257), (8, 4, 257), (13, 8, 130), (33, 4, 257), (63, 2, 4099), (63, 8, 257)]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def make_cores(n, D, seed=0):
    """The uniform state + noise of a size that keeps the majorants near the values (kappa_Z, kappa_b of order 10 at every case: a
    bound in units of the majorant then says something about the value): the noise of the L - 1 nodes adds up in Z like
    (L - 1) (spread D)^2, so spread = 2 / (D sqrt L), and 0.3 at most."""
    _, L = tt.tree_shape(n)
    return torch.from_numpy(tt.random_cores(n, D, 9000 * n + 17 * D + seed, spread=min(0.3, 2.0 / (D * math.sqrt(L))))).contiguous()


def epoch_tensor(e=EPOCH):
    return torch.tensor([e], dtype=torch.int64, device=dev())


def workspace_view(n, D, B):
    """(U^ [2 L, D, D], V^ [2 L, D, D], eU [2 L], eV [2 L]) read back from the cached workspace (the layout of kernels_ttn.hip)."""
    d = dev()
    _, L = tt.tree_shape(n)
    buf = backend._workspaces[backend._ws_key(d, f"ttn_{n}_{D}_{B}")]
    base = (-buf.data_ptr()) % 256
    up = lambda b: (b + 255) & ~255
    ne = 2 * L * D * D
    raw = buf[base:base + 256 + 2 * up(8 * ne) + 2 * up(4 * 2 * L)].cpu().numpy()
    o = 256
    out = []
    for _ in range(2):
        out.append(raw[o:o + 8 * ne].view(np.float64).reshape(2 * L, D, D).copy())
        o += up(8 * ne)
    eU = raw[o:o + 8 * L].view(np.int32).copy(); o += up(8 * L)
    eV = raw[o:o + 8 * L].view(np.int32).copy()
    return out[0], out[1], eU, eV


@functools.lru_cache(maxsize=None)
def sampled(n, D, B):
    """One run of environments + sample + score_vjp of a case, shared by the tests (the reference is computed once)."""
    cores = make_cores(n, D)
    c = cores.to(dev())
    w = np.random.default_rng([n, D, B, 5]).standard_normal(B)
    wt = torch.from_numpy(w).to(dev())
    logZ = backend.ttn_environments(c, n, B)
    idx, logq_s, status = backend.ttn_sample(c, n, B, SEED, epoch_tensor())
    grad, logq, st2 = backend.ttn_score_vjp(c, n, idx, wt)
    torch.cuda.synchronize()
    envs = workspace_view(n, D, B)
    env = tt.environments(cores.numpy(), n)
    idx_h = idx.cpu().numpy()
    return dict(cores=cores, c=c, w=w, wt=wt, logZ=float(logZ.item()), idx=idx_h, idx_dev=idx, status=int(status.item()),
                logq_sampler=logq_s, grad=grad.cpu().numpy(), grad_dev=grad, logq=logq.cpu().numpy(), logq_dev=logq,
                status_score=int(st2.item()), envs=envs, env=env, bits=tt.bits_of_idx(idx_h, n))


def _worst_ratio(mat, ex, ref, ab):
    err = np.abs(mat.astype(tt.LD) * tt.LD(2.0) ** int(ex) - ref)
    den = ab * tt.LD(EPS)
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), np.where(err == 0, 0, np.inf))))


@pytest.mark.parametrize("n,D,B", CASES)
def test_environments_and_log_z(n, D, B):
    r = sampled(n, D, B)
    Uh, Vh, eU, eV = r["envs"]
    env = r["env"]
    h, L = tt.tree_shape(n)
    worst = 0.0
    for v in range(1, L):
        d = v.bit_length() - 1
        for mat, ex, ref, ab, C in ((Uh[v], eU[v], env["U"][v], env["U_abs"][v], c_u(h - d, D)),
                                    (Vh[v], eV[v], env["V"][v], env["V_abs"][v], c_v(d, h, D))):
            assert 1.0 <= np.abs(mat).max() < 2.0          # the power-of-two rescaling: the largest magnitude lies in [1, 2)
            if C == 0:
                assert _worst_ratio(mat, ex, ref, ab) == 0.0
                continue
            worst = max(worst, _worst_ratio(mat, ex, ref, ab) / C)
    kZ = float(env["Z_abs"] / env["Z"])
    logZ_ref = float(np.log(env["Z"]))
    bound = EPS * (c_u(h, D) * kZ + 8 * (abs(logZ_ref) + 4))
    print(f"n={n} D={D}: worst environment ratio / C = {worst:.3f}; |logZ err| / bound = {abs(r['logZ'] - logZ_ref) / bound:.3f}")
    assert worst <= 1.0
    assert abs(r["logZ"] - logZ_ref) <= bound


@pytest.mark.parametrize("n,D,B", CASES)
def test_draws_against_the_mirror(n, D, B):
    """Every drawn bit equals the mirror's decision on the GPU's own prefix; no draw lies within 2^-40 of its threshold."""
    r = sampled(n, D, B)
    assert r["status"] == 0
    masses = tt.masses_on_prefix(r["cores"].numpy(), n, r["bits"], r["env"])
    U = tt.uniforms(SEED, EPOCH, np.arange(B), n)
    undecided = 0
    for j in range(n):
        z, _, und = tt.decide(masses[j][:, :, None], U[:, j])
        undecided += und
        assert np.array_equal(z, r["bits"][:, j]), j
    assert undecided == 0
    assert np.all(r["idx"] >= 0) and (n == 63 or np.all(r["idx"] < (1 << n)))
    if n * B >= 64:
        assert 0 < r["bits"].sum() < r["bits"].size
    # the sampler's logq is the score call's, bit for bit: they share the device function for x_v
    assert torch.equal(r["logq_sampler"], r["logq_dev"])


@pytest.mark.parametrize("n,D,B", CASES)
def test_logq_and_gradient_against_the_mirror(n, D, B):
    r = sampled(n, D, B)
    cores, bits, w, env = r["cores"].numpy(), r["bits"], r["w"], r["env"]
    _, L = tt.tree_shape(n)
    assert r["status_score"] == 0 and r["grad"].shape == (L - 1, D, D, D)
    ref = tt.score_gradient(cores, n, bits, w, env)
    f64 = tt.score_gradient(cores, n, bits, w, dtype=np.float64)
    kZ = float(env["Z_abs"] / env["Z"])
    kb = hp.to_f64(ref["kappa"])
    bound = logq_bound(n, D, kb, kZ, hp.to_f64(ref["logq"]), float(np.log(env["Z"])))
    lr = np.abs(hp.to_f64(r["logq"].astype(tt.LD) - ref["logq"])) / (EPS * bound)
    oracle, _ = hp.worst(hp.ratio(f64["grad"], ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    derived = c_score(n, D, B, float(kb.max()), kZ)
    C = hp.measured_constant(oracle, derived)
    g = r["grad"]
    gr, at = hp.worst(hp.ratio(g, ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    print(f"n={n} D={D} B={B}: worst logq ratio {lr.max():.3f} (bound up to {bound.max():.0f} eps); worst grad ratio {gr:.2f} at {at}, "
          f"C = {C:.0f} (float64 mirror {oracle:.2f}, derived {derived:.0f}, kappa_max {kb.max():.2f}, kappa_Z {kZ:.2f})")
    assert lr.max() <= 1.0
    assert C <= derived and gr <= C
    live = tt.live_mask(n, D)
    assert np.all(g[~live] == 0.0) and not np.signbit(g[~live]).any()          # dead entries: exactly +0.0


@pytest.mark.parametrize("n,D,B", CASES)
def test_null_gradient_and_repeats(n, D, B):
    """A NULL grad_cores gives the same logq bits; two calls are bitwise equal; dead cores entries are never read."""
    r = sampled(n, D, B)
    c = r["c"]
    backend.ttn_environments(c, n, B)
    idx, logq_s, st = backend.ttn_sample(c, n, B, SEED, epoch_tensor())
    assert int(st.item()) == 0 and np.array_equal(idx.cpu().numpy(), r["idx"]) and torch.equal(logq_s, r["logq_dev"])
    none, logq, st = backend.ttn_score_vjp(c, n, idx, out=False)
    assert none is None and int(st.item()) == 0 and torch.equal(logq, r["logq_dev"])
    grad, logq2, _ = backend.ttn_score_vjp(c, n, idx, r["wt"])
    assert torch.equal(grad, r["grad_dev"]) and torch.equal(logq2, r["logq_dev"])
    other_epoch, _, _ = backend.ttn_sample(c, n, B, SEED, epoch_tensor(EPOCH + 1))
    other_seed, _, _ = backend.ttn_sample(c, n, B, SEED + 1, epoch_tensor())
    if n * B >= 64:
        assert not torch.equal(idx, other_epoch) and not torch.equal(idx, other_seed)
    noisy = torch.where(torch.from_numpy(tt.live_mask(n, D)), r["cores"], torch.full_like(r["cores"], math.nan)).to(dev())
    logZ = backend.ttn_environments(noisy, n, B)
    idx3, logq3, st3 = backend.ttn_sample(noisy, n, B, SEED, epoch_tensor())
    grad3, _, st4 = backend.ttn_score_vjp(noisy, n, idx3, r["wt"])
    assert float(logZ.item()) == r["logZ"] and torch.equal(idx3, idx) and torch.equal(logq3, r["logq_dev"]) and torch.equal(grad3, r["grad_dev"])
    assert int(st3.item()) == 0 and int(st4.item()) == 0


def test_sample_b_does_not_depend_on_the_batch():
    n, D = 63, 2
    big = sampled(n, D, 4099)
    c = big["c"]
    for B in (1, 17, 64, 130):
        backend.ttn_environments(c, n, B)
        idx, logq, _ = backend.ttn_sample(c, n, B, SEED, epoch_tensor())
        _, logq2, _ = backend.ttn_score_vjp(c, n, idx, out=False)
        assert np.array_equal(idx.cpu().numpy(), big["idx"][:B])
        assert np.array_equal(logq.cpu().numpy(), big["logq"][:B]) and torch.equal(logq, logq2)
    n, D = 13, 8
    small = sampled(n, D, 130)
    B = 64 * 3 + 5
    backend.ttn_environments(small["c"], n, B)
    idx, logq, _ = backend.ttn_sample(small["c"], n, B, SEED, epoch_tensor())
    assert np.array_equal(idx.cpu().numpy()[:130], small["idx"]) and np.array_equal(logq.cpu().numpy()[:130], small["logq"])


def test_sampler_frequencies():
    """(5, 3, 2^16): the frequencies of the 32 outcomes within 4 standard errors of the exact q; the seed is the one with which
    test_ttn_host.py::test_mirror_sampler_frequencies_and_no_undecided_draw shows the mirror's own sampler under 3."""
    n, D, B = 5, 3, 1 << 16
    cores = tt.random_cores(n, D, 21)
    c = torch.from_numpy(cores).to(dev())
    backend.ttn_environments(c, n, B)
    idx, logq, st = backend.ttn_sample(c, n, B, tt.FREQ_SEED, epoch_tensor(0))
    assert int(st.item()) == 0
    _, q = tt.brute_force(cores, n)
    q = hp.to_f64(q)
    freq = np.bincount(idx.cpu().numpy(), minlength=32) / B
    zs = np.abs(freq - q) / np.sqrt(q * (1 - q) / B)
    print(f"sampler frequencies: worst |freq - q| / standard error = {zs.max():.2f}")
    assert zs.max() <= 4.0
    assert np.all(np.abs(np.exp(logq.cpu().numpy()) - q[idx.cpu().numpy()]) <= 1e-13)


@pytest.mark.parametrize("n,D,B", [(63, 2, 4099), (13, 8, 130)])
def test_power_of_two_scaling_changes_no_index(n, D, B):
    """Every live core entry times 2^12 or 2^-12: the same indices, log Z and logq shifted by what the mirror says."""
    r = sampled(n, D, B)
    _, L = tt.tree_shape(n)
    for p in (12, -12):
        c = (r["cores"] * 2.0 ** p).to(dev())
        logZ = backend.ttn_environments(c, n, B)
        idx, logq, status = backend.ttn_sample(c, n, B, SEED, epoch_tensor())
        assert int(status.item()) == 0 and np.array_equal(idx.cpu().numpy(), r["idx"])
        shift = 2 * (L - 1) * p * math.log(2.0)          # psi is of degree L - 1 in the cores, Z of degree 2 (L - 1)
        assert abs(float(logZ.item()) - (r["logZ"] + shift)) <= 64 * EPS * (abs(shift) + abs(r["logZ"]) + 4)
        assert np.abs(logq.cpu().numpy() - r["logq"]).max() <= 64 * EPS * (abs(shift) + np.abs(r["logq"]).max() + 4)
        grad, _, st = backend.ttn_score_vjp(c, n, idx, r["wt"])
        assert int(st.item()) == 0 and bool(torch.isfinite(grad).all())


def test_zero_mass_and_status():
    """All-zero cores: status 1 from the sampler (idx 0, logq NaN), log Z -inf, status 2 from the score call.  A sample with
    psi = 0: logq -inf, no contribution to the sample term, status 2."""
    n, D, B = 12, 3, 65
    c = torch.zeros_like(make_cores(n, D)).to(dev())
    logZ = backend.ttn_environments(c, n, B)
    idx, logq, status = backend.ttn_sample(c, n, B, SEED, epoch_tensor())
    assert int(status.item()) == 1 and bool((idx == 0).all()) and bool(torch.isnan(logq).all()) and float(logZ.item()) == -math.inf
    _, lq, st = backend.ttn_score_vjp(c, n, idx, torch.zeros(B, dtype=torch.float64, device=dev()))
    assert int(st.item()) == 2
    n, D = 4, 2
    cores = make_cores(n, D, seed=2)
    cores[1, :, 1, :] = 0.0                             # node 2 (positions 0, 1): every z with z_1 = 1 has psi = 0
    bits = np.array([[0, 0, 1, 0], [1, 1, 0, 1], [0, 1, 0, 1]])
    w = np.array([0.5, -2.0, 1.5])
    c = cores.to(dev())
    backend.ttn_environments(c, n, 3)
    grad, logq, status = backend.ttn_score_vjp(c, n, torch.from_numpy(tt.idx_of_bits(bits)).to(dev()), torch.from_numpy(w).to(dev()))
    assert int(status.item()) == 2 and float(logq[1].item()) == -math.inf and bool(torch.isfinite(logq[[0, 2]]).all())
    env = tt.environments(cores.numpy(), n)
    ref = tt.score_gradient(cores.numpy(), n, bits, w, env)
    C = c_score(n, D, 3, float(ref["kappa"][[0, 2]].max()), float(env["Z_abs"] / env["Z"]))
    r, at = hp.worst(hp.ratio(grad.cpu().numpy(), ref["grad"], ref["grad_abs"], X=hp._LongDouble))
    assert r <= C, (r, at)


@pytest.mark.parametrize("value", [math.inf, math.nan], ids=["inf", "nan"])
def test_non_finite_core_entry(value):
    """One Inf or NaN in a live entry of a bottom node at n = 12, D = 3: log Z is not finite, every sample meets a mass that is not
    finite at its first position (U of the node is in every density): status 1, every bit 0, logq NaN; the score call finds no
    sample that counts (Z is not finite and positive): status 2.  The calls return, and nothing is left in the workspace."""
    n, D, B = 12, 3, 65
    bad = make_cores(n, D).clone()
    bad[11, 0, 0, 1] = value                             # node 12: positions 8, 9
    c = bad.to(dev())
    logZ = backend.ttn_environments(c, n, B)
    idx, logq, status = backend.ttn_sample(c, n, B, SEED, epoch_tensor())
    assert not math.isfinite(float(logZ.item()))
    assert int(status.item()) == 1 and bool((idx == 0).all()) and bool(torch.isnan(logq).all())
    rng = np.random.default_rng(12)
    it = torch.from_numpy(tt.idx_of_bits(rng.integers(0, 2, size=(B, n)))).to(dev())
    w = torch.from_numpy(rng.standard_normal(B)).to(dev())
    grad, lq, st = backend.ttn_score_vjp(c, n, it, w)
    assert int(st.item()) == 2 and not bool(torch.isfinite(lq).any()) and tuple(grad.shape) == (15, D, D, D)
    _, lq0, st0 = backend.ttn_score_vjp(c, n, it, out=False)
    assert int(st0.item()) == 2 and not bool(torch.isfinite(lq0).any())
    good = make_cores(n, D).to(dev())
    assert math.isfinite(float(backend.ttn_environments(good, n, B).item()))
    idx, _, status = backend.ttn_sample(good, n, B, SEED, epoch_tensor())
    _, lq, st = backend.ttn_score_vjp(good, n, idx, out=False)
    assert int(status.item()) == 0 and int(st.item()) == 0 and bool(torch.isfinite(lq).all())
    backend.ttn_environments(good, n, 257)
    ref, _, _ = backend.ttn_sample(good, n, 257, SEED, epoch_tensor())
    assert torch.equal(idx, ref[:B])


def test_refused_sizes_leave_everything_untouched():
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    UNSUPPORTED = _ext._ENUMS["BORNVI_ERR_UNSUPPORTED"]
    size = lib.bornvi_ttn_workspace_bytes
    for n, D, B in ((0, 4, 8), (64, 4, 8), (8, 1, 8), (8, 9, 8), (8, 4, 0), (8, 4, (1 << 24) + 1)):
        assert size(h.h, n, D, B) == 0
    # the workspace does not grow with B beyond MAX_WG tiles of 64 samples; the header states its size at (63, 8)
    top = size(h.h, 63, 8, 1 << 24)
    assert top == size(h.h, 63, 8, tt.MAX_WG * 64) > size(h.h, 63, 8, tt.MAX_WG * 64 - 64)
    assert 0.775 * (1 << 30) <= top <= 0.785 * (1 << 30)
    n, D, B = 8, 4, 8
    need = size(h.h, n, D, B)
    canary = lambda count, dtype: torch.full((count,), 77, dtype=dtype, device=dev())
    ws, cores = canary(need, torch.uint8), make_cores(n, D).to(dev())
    idx, logq, grad = canary(B, torch.int64), canary(B, torch.float64), canary(cores.numel(), torch.float64)
    st, lz = canary(1, torch.int32), canary(1, torch.float64)
    w, ep = torch.ones(B, dtype=torch.float64, device=dev()), torch.zeros(1, dtype=torch.int64, device=dev())
    P = lambda t: t.data_ptr()
    for nn, DD, BB, bytes_ in ((0, D, B, need), (64, D, B, need), (n, 1, B, need), (n, 9, B, need), (n, D, 0, need),
                               (n, D, (1 << 24) + 1, need), (n, D, B, need - 1), (n, D, B, 0)):
        assert lib.bornvi_ttn_environments(h.h, nn, DD, BB, P(cores), P(lz), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_ttn_sample(h.h, nn, DD, BB, P(cores), 1, P(ep), P(idx), P(logq), P(st), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_ttn_score_vjp(h.h, nn, DD, BB, P(cores), P(idx), P(w), P(logq), P(grad), P(st), P(ws), bytes_, None) == UNSUPPORTED
        assert lib.bornvi_ttn_score_vjp(h.h, nn, DD, BB, P(cores), P(idx), None, P(logq), None, P(st), P(ws), bytes_, None) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (ws, idx, logq, grad, st, lz):
        assert bool((t == 77).all())


def test_capture_and_replay():
    """The three calls captured into one graph (a single chain, no branches) and replayed once give the eager bits."""
    n, D, B = 12, 5, 257
    c = make_cores(n, D, seed=3).to(dev())
    ep = epoch_tensor(1)
    w = torch.from_numpy(np.random.default_rng(1).standard_normal(B)).to(dev())
    backend.ttn_environments(c, n, B)
    idx0, lq0, _ = backend.ttn_sample(c, n, B, SEED, ep)
    grad0, logq0, _ = backend.ttn_score_vjp(c, n, idx0, w)
    eager = (idx0.clone(), lq0.clone(), grad0.clone(), logq0.clone())
    idx = torch.empty(B, dtype=torch.int64, device=dev())
    lqs = torch.empty(B, dtype=torch.float64, device=dev())
    logq = torch.empty(B, dtype=torch.float64, device=dev())
    grad = torch.empty_like(c)
    st1 = torch.empty(1, dtype=torch.int32, device=dev())
    st2 = torch.empty(1, dtype=torch.int32, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        backend.ttn_environments(c, n, B)                      # the side stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.ttn_environments(c, n, B)
        backend.ttn_sample(c, n, B, SEED, ep, out_idx=idx, out_logq=lqs, status=st1)
        backend.ttn_score_vjp(c, n, idx, w, out=grad, out_logq=logq, status=st2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager[0]) and torch.equal(lqs, eager[1]) and torch.equal(grad, eager[2]) and torch.equal(logq, eager[3])
    assert int(st1.item()) == 0 and int(st2.item()) == 0
