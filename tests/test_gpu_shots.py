"""Finite-shot KSD training on the GPU: the sampler (bornvi_shots_histogram) against the NumPy mirror of its documented
draw function (tests/shots_mirror.py) bit for bit on dyadic rows, draw for draw against extended-precision inversion on
rows that are not dyadic (sparse and peaked, one dominant outcome, 30 orders of magnitude and unnormalised, a circuit's own
|psi|^2), its invariants and statistics, and the shots mode of QuantumBornMachine / KSDVariationalInference (eager, graph
replay, train(), two ranks).  Every seed is fixed: each statistical check is deterministic, with thresholds at about the
1e-6 level of its null distribution."""
import os

import numpy as np
import pytest
import torch
from scipy import stats

import shots_mirror as sm
from conftest import run_ranks
import shots_worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _dyadic(rng, N, zeros=0.3):
    """A row of multiples of 2^-k summing to exactly 1: every partial sum is exact in any order."""
    a = rng.integers(0, 64, N).astype(np.int64)
    a[rng.random(N) < zeros] = 0
    a[rng.integers(N)] += 1
    K = 1 << int(np.ceil(np.log2(a.sum())))
    a[np.nonzero(a)[0][-1]] += K - a.sum()
    return a / K


def _sample(probs, n, shots, seed, epoch, dev, **kw):
    from tensornetworks_amd import backend
    P = torch.as_tensor(np.ascontiguousarray(probs), dtype=torch.float64, device=dev).reshape(-1, 1 << n)
    ep = torch.tensor([epoch], dtype=torch.int64, device=dev)
    return backend.shots_histogram(P, n, shots, seed, ep, **kw).cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 8, 12, 14, 16])
def test_counts_equal_mirror_bitwise(dev, n):
    rng = np.random.default_rng(100 + n)
    B = 3
    probs = np.stack([_dyadic(rng, 1 << n) for _ in range(B)])
    for seed, epoch, S in ((1, 0, 1), (0xDEADBEEFCAFEF00D, 7, 1000), (12345, 1 << 33 | 5, 100000)):
        got = _sample(probs, n, S, seed, epoch, dev)
        want = sm.histogram(probs, S, seed, epoch)
        assert np.array_equal(got, want / S), (n, seed, epoch, S)
        assert (want.sum(axis=1) == S).all()


def test_counts_equal_mirror_strided_ids(dev):
    """Rows keyed like the (+p, -p) rows of a strided parameter shard without the base row."""
    n, S = 9, 20000
    rng = np.random.default_rng(1)
    probs = np.stack([_dyadic(rng, 1 << n) for _ in range(6)])
    got = _sample(probs, n, S, 77, 3, dev, include_base=False, p_begin=5, p_stride=3)
    want = sm.histogram(probs, S, 77, 3, include_base=False, p_begin=5, p_stride=3)
    assert np.array_equal(got, want / S)


def test_three_levels_equal_mirror(dev):
    """n = 25: blocks of blocks of blocks (2^25 -> 2^13 -> 2 masses)."""
    n, S = 25, 30000
    rng = np.random.default_rng(25)
    probs = _dyadic(rng, 1 << n, zeros=0.9)[None]
    got = _sample(probs, n, S, 5, 2, dev)
    want = sm.histogram(probs, S, 5, 2)
    assert np.array_equal(got, want / S)


def test_invariants(dev):
    from tensornetworks_amd import backend
    n, S = 13, 54321
    N = 1 << n
    rows = [np.eye(N)[0], np.eye(N)[N - 1], np.eye(N)[4097], np.zeros(N)]
    rng = np.random.default_rng(3)
    x = rng.random(N) ** 4
    x[rng.random(N) < 0.5] = 0.0
    rows.append(x / x.sum())                                   # not dyadic: only the invariants are pinned
    probs = torch.tensor(np.stack(rows), dtype=torch.float64, device=dev)
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    f = backend.shots_histogram(probs, n, S, 9, ep)
    c = (f * S).round().cpu().numpy().astype(np.int64)
    assert torch.equal(f, torch.as_tensor(c / S, device=dev))      # exact multiples of 1/S
    assert c[0, 0] == S and c[1, N - 1] == S and c[2, 4097] == S
    assert (c[3] == 0).all()                                       # a row of zeros yields zeros
    assert c[4].sum() == S and (c[4][rows[4] == 0] == 0).all()      # probability 0: never drawn
    again = backend.shots_histogram(probs, n, S, 9, ep)
    assert torch.equal(again, f)                                   # same (seed, epoch): same bits
    ep += 1
    assert not torch.equal(backend.shots_histogram(probs, n, S, 9, ep)[4], f[4])
    ep -= 1
    inplace = probs.clone()
    backend.shots_histogram(inplace, n, S, 9, ep, out=inplace)
    assert torch.equal(inplace, f)                                 # in place == out of place
    with pytest.raises(backend.BornviError):
        backend.shots_histogram(probs, n, 0, 9, ep)
    buf = torch.zeros((5 << n) + 8, dtype=torch.float64, device=dev)
    with pytest.raises(backend.BornviError):                      # partial overlap of out and probs is refused
        backend.shots_histogram(buf[: 5 << n].view(5, N), n, S, 9, ep, out=buf[8:].view(5, N))


def _hw_q(n, L, seed, dev):
    from tensornetworks_amd import backend
    g = np.random.default_rng(seed)
    P = backend.num_params("hardware_efficient", n, L)
    th = torch.tensor(g.uniform(-np.pi, np.pi, P), dtype=torch.float64, device=dev)
    return backend.circuit_probs("hardware_efficient", n, L, th.view(1, -1))[0]


def test_chi_square_goodness_of_fit(dev):
    from tensornetworks_amd import backend
    n, S = 10, 10 ** 6
    q = _hw_q(n, 3, 0, dev)
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    pvals = []
    for seed in (1, 2, 3):
        c = (backend.shots_histogram(q.view(1, -1), n, S, seed, ep)[0] * S).round().cpu().numpy()
        e = q.cpu().numpy() * S
        big = e >= 5
        obs = np.append(c[big], c[~big].sum())
        exp = np.append(e[big], e[~big].sum())
        keep = exp > 0
        pvals.append(stats.chisquare(obs[keep], exp[keep] * obs[keep].sum() / exp[keep].sum()).pvalue)
    assert min(pvals) > 1e-6, pvals


def test_mean_histogram_converges_to_q(dev):
    from tensornetworks_amd import backend
    n, S, E = 6, 1000, 2000
    q = _hw_q(n, 2, 1, dev)
    ep = torch.zeros(1, dtype=torch.int64, device=dev)
    acc = torch.zeros(1 << n, dtype=torch.float64, device=dev)
    rows = q.view(1, -1).repeat(8, 1).contiguous()                # 8 independent circuit ids per epoch
    for _ in range(E):
        acc += backend.shots_histogram(rows, n, S, 4, ep).sum(0)
        ep += 1
    mean = (acc / (8 * E)).cpu().numpy()
    qq = q.cpu().numpy()
    se = np.sqrt(qq * (1 - qq) / (8 * E * S))
    z = np.abs(mean - qq)[qq > 0] / se[qq > 0]
    assert z.max() < 6.0, z.max()                                  # 64 bins, family-wise ~1e-6


# ---- rows that are not dyadic: every draw against exact inversion -----------------------------------------------------------
# sm.histogram_exact forms masses and cdfs in extended precision and counts the draws whose u lies within 2^-40 of a boundary
# (about 100 times what the kernels' order of summation can move one: tests/test_shots_host.py derives it).  With no such
# draw, the kernel's counts must equal the reference's exactly.  The synthetic inputs are the ones that host module has
# already shown to be free of undecided draws.
CASES = {c[0]: c for c in sm.synthetic_cases()}


def _equals_exact(probs, n, S, seed, epoch, dev, **ids):
    """Asserts freq == exact counts / S for one call; returns the number of draws compared."""
    got = _sample(probs, n, S, seed, epoch, dev, **ids)
    want, undecided = sm.histogram_exact(probs, S, seed, epoch, **ids)
    assert undecided == 0
    assert np.array_equal(got, want / S)
    c = np.rint(got * S).astype(np.int64)
    has_mass = (np.asarray(probs) > 0).any(axis=1)
    assert (c.sum(axis=1) == np.where(has_mass, S, 0)).all()         # every row with a positive entry sums to S
    assert (c[np.asarray(probs) == 0] == 0).all()                    # probability 0: never drawn
    return int(c.sum())


@pytest.mark.parametrize("n,kind", [(n, k) for n in sm.REAL_N for k in "abcd" if k != "d" or n >= 3])
def test_real_rows_equal_exact_inversion(dev, n, kind):
    if kind == "d":                                                  # the device's own |psi|^2 of a hardware-efficient circuit,
        probs = _hw_q(n, 2, 40 + n, dev).cpu().numpy()[None]         # read back: the reference's input bit for bit
        assert abs(probs.sum() - 1.0) < 1e-12
    else:
        probs = sm.real_rows(kind, n)
    draws = sum(_equals_exact(probs, n, S, sm.REAL_SEED, sm.REAL_EPOCH, dev) for S in sm.REAL_SHOTS)
    print(f"n = {n}, kind ({kind}): undecided 0, {draws} draws compared")


def test_full_top_block_dyadic_equals_mirror(dev):
    """n = 24: the top level is exactly one full block of 4096 masses."""
    name, make, S, seed, epoch, ids = CASES["n24-dyadic"]
    probs = make()
    want = sm.histogram(probs, S, seed, epoch)
    assert np.array_equal(_sample(probs, 24, S, seed, epoch, dev), want / S) and want.sum() == S
    print(f"n = 24 dyadic: bitwise, {S} draws compared")


def test_full_top_block_sparse_equals_exact_inversion(dev):
    name, make, S, seed, epoch, ids = CASES["n24-sparse"]
    probs = make()
    assert (probs == 0).mean() > 0.98
    draws = _equals_exact(probs, 24, S, seed, epoch, dev)
    print(f"n = 24, 99 % zeros: undecided 0, {draws} draws compared")


def test_power_of_two_scaling_keeps_every_bit(dev):
    """Every add and the product u * total scale exactly by a power of two as long as nothing goes subnormal or overflows:
    a row times 2^-600 or 2^+600 gives the bits of the unscaled row's frequencies."""
    freqs, draws = [], 0
    for e in sm.SCALES:
        name, make, S, seed, epoch, ids = CASES[f"scale-2^{e:+.0f}"]
        probs = make()
        assert np.isfinite(probs).all() and probs[probs > 0].min() > 2.0 ** -400 * probs.sum() > 0
        assert probs[probs > 0].min() > 2.0 ** -1000 and probs.sum() < 2.0 ** 1000
        draws += _equals_exact(probs, 13, S, seed, epoch, dev)
        freqs.append(_sample(probs, 13, S, seed, epoch, dev))
    assert np.array_equal(freqs[0], freqs[1]) and np.array_equal(freqs[0], freqs[2])
    print(f"scaled rows: undecided 0, {draws} draws compared")


@pytest.mark.parametrize("kind", ["a", "c"])
def test_real_rows_strided_ids_equal_exact_inversion(dev, kind):
    name, make, S, seed, epoch, ids = CASES[f"strided-{kind}"]
    assert ids == dict(include_base=False, p_begin=5, p_stride=3)
    draws = _equals_exact(make(), 9, S, seed, epoch, dev, **ids)
    print(f"strided ids, kind ({kind}): undecided 0, {draws} draws compared")


def test_batch_equals_rows_sampled_one_call_each(dev):
    name, make, S, seed, epoch, ids = CASES["mixed-batch"]
    probs = make()
    n = 13
    draws = _equals_exact(probs, n, S, seed, epoch, dev)
    batch = _sample(probs, n, S, seed, epoch, dev)
    for r in range(len(probs)):
        if r == 0:
            alone = _sample(probs[:1], n, S, seed, epoch, dev)[0]
        else:                                                        # row r is shift (r - 1) & 1 of parameter (r - 1) >> 1:
            pair = np.stack([probs[0], probs[r]]) if (r - 1) & 1 else probs[r:r + 1]      # the - shift is a call's row 1
            alone = _sample(pair, n, S, seed, epoch, dev, include_base=False, p_begin=(r - 1) >> 1)[-1]
        assert np.array_equal(alone, batch[r]), r
    print(f"batch of {len(probs)}: undecided 0, {draws} draws compared")


def _vi(n, L, dev, shots=None, seed=0, ansatz="hardware_efficient", init="small_random", **kw):
    from tensornetworks_amd.bayesian_network import synthetic_network
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    bn, lat, obs, x = synthetic_network(n, seed=1)
    torch.manual_seed(seed)
    vi = KSDVariationalInference(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, qbm_ansatz_type=ansatz,
                                 qbm_init_method=init, pytorch_device=str(dev), qbm_shots=shots, **kw)
    vi._prepare_stein(x)
    return vi


def test_gradient_times_loss_is_unbiased(dev):
    """grad_p loss = 1/2 (q^+_p - q^-_p)^T K q^ with independent draws: its mean over 500 epochs at fixed theta matches the
    exact 1/2 (q+_p - q-_p)^T K q within 5 standard errors for every p."""
    n, L, E = 6, 2, 500
    exact = _vi(n, L, dev)
    loss0, grad0, _ = exact.ksd_and_grad()
    target = (grad0 * loss0).cpu().numpy()
    vi = _vi(n, L, dev, shots=2000, shot_seed=11)
    theta64 = vi.born_machine.theta.detach().to(dev, torch.float64)
    samples = torch.stack([(lambda r: r[1] * r[0])(vi.ksd_and_grad(theta64)) for _ in range(E)]).cpu().numpy()
    mean, se = samples.mean(0), samples.std(0, ddof=1) / np.sqrt(E)
    assert (se > 0).all()
    z = np.abs(mean - target) / se
    assert z.max() < 5.0, (z.max(), int(z.argmax()))


def test_basic_ansatz_at_zero_has_exact_loss(dev):
    """basic ansatz, theta = 0: identity gates, q = e_0 exactly, so its histogram is e_0 and the shots loss is the exact one."""
    exact = _vi(5, 2, dev, ansatz="basic", init="zero")
    loss0, _, q0 = exact.ksd_and_grad()
    qn = q0.cpu().numpy()
    assert qn[0] == 1.0 and (qn[1:] == 0).all()
    vi = _vi(5, 2, dev, shots=777, shot_seed=3, ansatz="basic", init="zero")
    loss, grad, q = vi.ksd_and_grad()
    assert torch.equal(q, q0)
    assert abs(loss.item() - loss0.item()) <= 1e-15
    assert vi.born_machine.get_probabilities().detach().cpu().numpy()[0] == 1.0


def test_born_machine_histograms(dev):
    """get_probabilities: a fresh histogram per call (mirror-exact for the base circuit id at the machine's epoch);
    backward: the shifted circuits' histograms at that epoch."""
    from tensornetworks_amd.quantum_born_machine import QuantumBornMachine
    from tensornetworks_amd import backend
    torch.manual_seed(0)
    qbm = QuantumBornMachine(4, 2, shots=5000, shot_seed=21).to(dev)
    assert qbm.dev.shots == 5000
    a = qbm.get_probabilities()
    b = qbm.get_probabilities()
    assert not torch.equal(a, b)
    for h in (a, b):
        hn = h.detach().cpu().numpy()
        c = np.rint(hn * 5000)
        assert np.array_equal(hn, c / 5000) and int(c.sum()) == 5000
    d = qbm.get_prob_dict()
    assert len(d) == 16 and abs(sum(d.values()) - 1.0) < 1e-12
    # backward with dL/dq = w equals 1/2 w.(q^+ - q^-) of the shifted histograms at the forward's epoch
    w = torch.linspace(-1, 1, 16, dtype=torch.float64, device=dev)
    qbm.theta.grad = None
    ep_before = int(qbm.shot_epoch(dev).item())
    (qbm.get_probabilities() * w).sum().backward()
    th64 = qbm.theta.detach().to(dev, torch.float64)
    P = th64.numel()
    sh = backend.paramshift_probs("hardware_efficient", 4, 2, th64, 0, P, include_base=False)
    ep = torch.tensor([ep_before], dtype=torch.int64, device=dev)
    backend.shots_histogram(sh, 4, 5000, 21, ep, include_base=False, out=sh)
    want = 0.5 * (sh[0::2] - sh[1::2]) @ w
    torch.testing.assert_close(qbm.theta.grad.to(torch.float64), want.to(qbm.theta.grad.device), rtol=1e-6, atol=1e-7)


def test_adjoint_with_shots_is_rejected(dev):
    vi = _vi(4, 1, dev, shots=100, shot_seed=1)
    vi.grad_engine = "adjoint"
    with pytest.raises(ValueError):
        vi.ksd_and_grad()


def test_graph_replay_equals_eager_sequence(dev):
    """lr = 0 keeps theta fixed: the graph-replayed steps draw at epochs 2, 3, ... exactly what eager ksd_and_grad calls
    draw at those epochs (the epoch counter is a device tensor advanced inside the captured step)."""
    n, L, K = 8, 2, 8
    eager = _vi(n, L, dev, shots=4096, shot_seed=99)
    want = [eager.ksd_and_grad()[0].item() for _ in range(K)]
    vi = _vi(n, L, dev, shots=4096, shot_seed=99)
    params, opt, sched = vi.make_optimizer(0.0, 100, True, "adam", (0.9, 0.999), capturable=True)
    rec = []
    step = vi.make_graphed_step(params, opt, sched, 10.0, warmup=2, record=rec)
    got = [r[0].item() for r in rec] + [step()[0].item() for _ in range(K - 2)]
    assert got == want
    assert len(set(got)) == K


def test_train_with_shots_tracks_exact_tvd(dev):
    """Sprinkler, n = 3, S = 10^4: train() and train(host_sync=False) run with shots; the final TVD (measured on the
    exact q) ends within 0.05 of exact-mode training from the same initialisation (measured on the MI355X with these
    seeds: 0.2084 against 0.1763, a difference of 0.032)."""
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    bn = get_sprinkler_network(False)
    lat, obs, x = ["C", "S", "R"], ["W"], {"W": 1}
    post, _ = bn.get_true_posterior(lat, x)
    finals = {}
    for shots, host_sync in ((None, True), (10 ** 4, True), (10 ** 4, False)):
        torch.manual_seed(0)
        vi = KSDVariationalInference(bn, lat, obs, qbm_num_latent_vars=3, qbm_ansatz_layers=4, pytorch_device=str(dev),
                                     qbm_shots=shots, shot_seed=2024)
        h = vi.train(x, num_epochs=300, lr_born_machine=0.005, verbose=False, true_posterior_for_tvd=post,
                     host_sync=host_sync)
        assert len(h["loss_ksd"]) == 300 and np.isfinite(h["loss_ksd"]).all() and np.isfinite(h["tvd"]).all()
        finals[(shots, host_sync)] = h["tvd"][-1]
        if shots:
            qe = vi.born_machine.exact_probabilities().cpu().numpy()
            tab = [post.get(z, 0.0) for z in vi.born_machine.all_outcomes_tuples]
            assert abs(h["tvd"][-1] - 0.5 * np.abs(np.asarray(tab) - qe).sum()) < 1e-6   # the TVD is of the exact q
    print("final TVDs", finals)
    for host_sync in (True, False):
        assert abs(finals[(10 ** 4, host_sync)] - finals[(None, True)]) < 0.05, finals
    # graph replay (no TVD: n <= 13, Adam): the same losses as the eager deferred loop
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        vi = KSDVariationalInference(bn, lat, obs, qbm_num_latent_vars=3, qbm_ansatz_layers=4, pytorch_device=str(dev),
                                     qbm_shots=10 ** 4, shot_seed=2024)
        runs.append(vi.train(x, num_epochs=40, lr_born_machine=0.005, verbose=False, host_sync=False)["loss_ksd"])
    assert runs[0] == runs[1] and len(set(runs[0])) > 30


def _errors(tmp_path):
    return "\n".join(open(tmp_path / f).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".err"))


def test_two_ranks_equal_solo(dev, tmp_path):
    """W = 2 (gloo, both ranks on cuda:0): every shifted row is keyed by its GLOBAL circuit id, so the sharded shots step
    gives the solo step's loss and gradient bit for bit (matrix-free contraction: not sharded, same summation)."""
    n, L = 6, 2
    codes = run_ranks(shots_worker.shots_rank, 2, (n, L, str(tmp_path)), timeout=600)
    assert codes == [0, 0], (codes, _errors(tmp_path))
    vi = _vi(n, L, dev, shots=3000, seed=7, shot_seed=123, gram_mode="kron")
    loss, grad, q = vi.ksd_and_grad()
    for r in range(2):
        o = np.load(tmp_path / f"rank{r}.npz")
        np.testing.assert_array_equal(o["loss"], loss.cpu().numpy())
        np.testing.assert_array_equal(o["grad"], grad.cpu().numpy())
        np.testing.assert_array_equal(o["q"], q.cpu().numpy())
