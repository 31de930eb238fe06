"""AmortisedMPSInference on the GPU: Sprinkler with the sites (C, S, R, W) and D = 4, so the family
contains p exactly.  One epoch of each objective against the mirror's epoch (the mirror sampler, mps_sampled_mirror's score
gradient, the mirror's log-marginal gradient) within the kernels' bounds; the two query lists of 'conditional'; a short run
against p and against the CPU mirror of the same epochs; runs that do not depend on read-outs; the read-outs' consistency.

Bounds of the epoch, in units of EPS64: the gradient is the score call's (C_SCORE grad_abs, test_gpu_mps_sampled_kernel.py) plus
the log-marginal call's (amortised_mirror.log_marginal_gradient's bound) plus one unit of their magnitudes for the sum of the
two; the loss is a mean of B log q (each logq_bound; B - 1 additions in whatever order: B units of the mean magnitude) plus
sum_j c_j logm_j (each logm_bound of test_gpu_mps_query_kernel.py, the product, and 2^c additions)."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import amortised_mirror as am
import hp_reference as hp
import mps_query_mirror as qm
import mps_sampled_mirror as sm
from tensornetworks_amd import backend
from tensornetworks_amd.amortised_vi_sampled import AmortisedMPSInference
from tensornetworks_amd.bayesian_network import get_sprinkler_network
from test_gpu_mps_query_kernel import logm_bound
from test_gpu_mps_sampled_kernel import c_score, logq_bound

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
SITES = ['C', 'S', 'R', 'W']
LAT, OBS = ['C', 'S', 'R'], ['W']
N, D = 4, 4
# The short run starts from init_method='random' under torch seed 11: a start that is far from p at EVERY evidence below (marginal
# TVD >= 0.14, |log q(x) - log p(x)| >= 0.24, KL 2.6), so that "closer than before" says something about the fit and not about a
# start that happens to sit on one of the targets; 8192 draws an epoch keep the fit's own sampling noise (largest at the rare
# evidence S = 1, W = 0, p(x) = 0.007) several times below those distances.
RUN = dict(num_samples=8192, epochs=60, lr=0.05, seed=3, init_method='random')
EVIDENCES = [{'W': w} for w in (0, 1)] + [{'S': s, 'W': w} for s in (0, 1) for w in (0, 1)]


def make(num_samples, seed=3, init_method='small_random', init_seed=11):
    torch.manual_seed(init_seed)                         # the cores' initialisation draws from torch's generator
    return AmortisedMPSInference(get_sprinkler_network(False), LAT, OBS,
                                 {'bond_dim': D, 'num_samples': num_samples, 'seed': seed, 'init_method': init_method}, device='cuda')


def cores_of(vi):
    return vi.born_machine.cores.detach().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def mirror_epoch(B):
    """The mirror's epoch 0 at the trainer's initial cores, shared by the tests and left unchanged."""
    vi = make(B)
    c = cores_of(vi)
    s = am.bn_sample(vi._packed, N, 3, 0, B)
    env = sm.environments(c)
    score = sm.score_gradient(c, s["bits"], np.full(B, -1.0 / B), env)
    counts = np.bincount(s["bits"][:, 3], minlength=2)
    evs = [{3: 0}, {3: 1}]
    enum = am.log_marginal_gradient(c, evs, counts / B)
    per = am.log_marginal_gradient(c, [{3: int(w)} for w in s["bits"][:, 3]], np.full(B, 1.0 / B))
    kZ = float(env["Z_abs"] / env["Z"])
    logZ = float(np.log(env["Z"]))
    lq_bound = logq_bound(N, D, hp.to_f64(score["kappa"]), kZ, hp.to_f64(score["logq"]), logZ)
    lm = [qm.log_marginal(c, ev, env) for ev in evs]
    return dict(c=c, s=s, env=env, score=score, counts=counts, enum=enum, per=per, kZ=kZ, lq_bound=lq_bound, lm=lm)


@pytest.mark.parametrize("objective", ["joint", "conditional"])
def test_one_epoch_against_the_mirror(objective):
    B = 1000
    M = mirror_epoch(B)
    vi = make(B)
    loss, grad, st = vi.loss_and_grad(0, objective)
    assert int(st.item()) == 0
    assert np.array_equal(vi.last_idx.cpu().numpy(), M["s"]["idx"].astype(np.int64))
    score = M["score"]
    cs = c_score(N, D, B, float(score["kappa"].max()), M["kZ"])
    ref_grad = score["grad"]
    bound = cs * score["grad_abs"]
    ref_loss = -score["logq"].mean()
    loss_bound = float(M["lq_bound"].mean()) + B * float(np.abs(hp.to_f64(score["logq"])).mean())
    if objective == "conditional":
        ref_grad = ref_grad + M["enum"]["grad"]
        bound = bound + M["enum"]["bound"] + np.abs(score["grad"]) + np.abs(M["enum"]["grad"])
        for cnt, r in zip(M["counts"], M["lm"]):
            ref_loss = ref_loss + (cnt / sm.LD(B)) * r["logm"]
            loss_bound += (cnt / B) * (logm_bound(N, D, r) + 4 * abs(float(r["logm"])))
        loss_bound += abs(float(ref_loss))
    r, at = hp.worst(hp.ratio(grad.cpu().numpy(), ref_grad, bound, X=hp._LongDouble))
    lerr = abs(float(hp.to_f64(sm.LD(loss.item()) - ref_loss)))
    print(f"{objective}: worst gradient error / bound = {r:.2e} at {at}; loss error / bound = {lerr / (EPS * loss_bound):.2e}")
    assert r <= 1.0 and lerr <= EPS * loss_bound


def test_conditional_query_lists_agree():
    """All 2^c evidences with count_j / B against one query per sample: the same gradient within the two bounds."""
    B = 1000
    M = mirror_epoch(B)
    vi = make(B)
    loss_e, grad_e, st_e = vi.loss_and_grad(0, 'conditional')
    mask, value, c = vi.evidence_queries(vi.last_idx)
    assert c.cpu().numpy().tolist() == (M["counts"] / B).tolist()                     # integer counts, one division
    loss_p, grad_p, st_p = vi.loss_and_grad(0, 'conditional', per_sample_queries=True)
    assert int(st_e.item()) == 0 and int(st_p.item()) == 0
    # the score term is the same call twice: what differs is the log-marginal term and its one addition
    lim = EPS * hp.to_f64(M["enum"]["bound"] + M["per"]["bound"] + 2 * (np.abs(M["score"]["grad"]) + np.abs(M["enum"]["grad"])))
    diff = np.abs(grad_e.cpu().numpy() - grad_p.cpu().numpy())
    assert np.all(diff <= lim), float((diff / np.where(lim > 0, lim, 1)).max())
    # the losses: the same B log q, then 2 products and a sum against a B-term sum of the same logm values: B + 8 units
    mag = float(np.abs(hp.to_f64(M["score"]["logq"])).mean()) + sum(abs(float(r["logm"])) for r in M["lm"])
    assert abs(loss_e.item() - loss_p.item()) <= EPS * (B + 8) * mag


def true_marginals(bn, x):
    free = [nm for nm in SITES if nm not in x]
    lat = [nm for nm in free]
    post, px = bn.get_true_posterior(lat, x)
    return {nm: sum(p for z, p in post.items() if z[i] == 1) for i, nm in enumerate(lat)}, px


def readout_errors(vi, bn):
    """Per evidence: (sum over the free sites of the TVD of the site's marginal, |log q(x) - log p(x)|)."""
    out = []
    for x in EVIDENCES:
        want, px = true_marginals(bn, x)
        got = vi.posterior_marginals(x)
        assert list(got) == [nm for nm in SITES if nm not in x]
        out.append((sum(abs(got[nm] - want[nm]) for nm in want), abs(vi.log_evidence(x) - math.log(px))))
    return out


@functools.lru_cache(maxsize=None)
def short_run():
    """The device run (with read-outs between the epochs), shared by the tests below."""
    bn = get_sprinkler_network(False)
    vi = make(RUN["num_samples"], RUN["seed"], RUN["init_method"])
    c0 = cores_of(vi)
    kl0 = vi.exact_forward_kl()
    before = readout_errors(vi, bn)
    seen = []

    def look(epoch, t):
        if epoch % 7 == 0:
            seen.append((t.posterior_marginals({'W': 1})['R'], t.log_evidence({'S': 0}), t.exact_forward_kl(),
                         int(t.posterior_sample({'W': 0}, 65)[0][0].item())))

    hist = vi.train(RUN["epochs"], RUN["lr"], objective='joint', verbose=False, epoch_callback=look)
    return dict(bn=bn, vi=vi, c0=c0, kl0=kl0, before=before, hist=hist, seen=seen)


def test_short_run_fits_the_network():
    R = short_run()
    vi, bn = R["vi"], R["bn"]
    assert all(s == 0 for s in R["hist"]["status"]) and len(R["seen"]) == len(range(0, RUN["epochs"], 7))
    kl = vi.exact_forward_kl()
    after = readout_errors(vi, bn)
    print(f"KL(p || q): {R['kl0']:.6f} -> {kl:.6f}")
    assert kl < R["kl0"]
    for x, (tv0, le0), (tv1, le1) in zip(EVIDENCES, R["before"], after):
        print(f"  {x}: marginal TVD {tv0:.4f} -> {tv1:.4f}, |log q(x) - log p(x)| {le0:.4f} -> {le1:.4f}")
        assert tv1 < tv0 and le1 < le0, x
    # the CPU mirror of the same epochs: the device's final KL is at most twice the mirror's (the reordered float sums
    # through Adam over the epochs)
    p = am.site_joint(bn, SITES)
    assert abs(am.forward_kl(R["c0"], p) - R["kl0"]) <= 1e-12
    rep = am.replay(R["c0"], vi._packed, N, [3], RUN["num_samples"], RUN["seed"], RUN["epochs"], RUN["lr"], "joint")
    kl_mirror = am.forward_kl(rep["cores"], p)
    print(f"final KL: device {kl:.9f}, CPU mirror {kl_mirror:.9f}")
    assert kl <= 2 * kl_mirror


def test_runs_do_not_depend_on_readouts_and_repeat():
    R = short_run()
    vi = make(RUN["num_samples"], RUN["seed"], RUN["init_method"])
    assert np.array_equal(cores_of(vi), R["c0"])
    hist = vi.train(RUN["epochs"], RUN["lr"], objective='joint', verbose=False)          # no read-out in between
    assert np.array_equal(cores_of(vi), cores_of(R["vi"]))
    assert hist == R["hist"]


def test_readouts_are_consistent():
    vi = short_run()["vi"]
    bm = vi.born_machine
    for x in EVIDENCES:
        ev = {SITES.index(k): v for k, v in x.items()}
        base = bm.log_marginal(ev)
        got = vi.posterior_marginals(x)
        for nm, val in got.items():
            one = bm.log_marginal({**ev, SITES.index(nm): 1})
            assert val == float(torch.exp(one - base).item()), (x, nm)                   # a query's bits do not depend on Q
        assert vi.log_evidence(x) == float(base.item())
    # q(z | x) of every completion sums to one, and is log q(x, z) - log q(x)
    x = {'W': 1}
    z = np.array(list(itertools.product((0, 1), repeat=3)))
    lp = vi.posterior_log_prob(x, z).cpu().numpy()
    assert abs(np.exp(lp).sum() - 1.0) <= 1e-12
    marg = vi.posterior_marginals(x)
    for i, nm in enumerate(LAT):
        assert abs(np.exp(lp)[z[:, i] == 1].sum() - marg[nm]) <= 1e-12
    # samples carry x; with all but one site given, the free site's frequency matches its marginal within 5 sigma
    B = 65536
    x = {'C': 1, 'S': 0, 'W': 1}
    idx, logq, logm = vi.posterior_sample(x, B, seed=5, epoch=1)
    bits = sm.bits_of_idx(idx.cpu().numpy(), N)
    for nm, v in x.items():
        assert np.all(bits[:, SITES.index(nm)] == v)
    p1 = vi.posterior_marginals(x)['R']
    freq = bits[:, SITES.index('R')].mean()
    assert abs(freq - p1) <= 5 * math.sqrt(p1 * (1 - p1) / B), (freq, p1)
    assert abs(float(logm.item()) - vi.log_evidence(x)) == 0.0
    idx2, _, _ = vi.posterior_sample({'W': 0}, 257)
    assert np.all(sm.bits_of_idx(idx2.cpu().numpy(), N)[:, 3] == 0)
