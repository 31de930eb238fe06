"""bornvi_bn_score_samples and bornvi_stein_pairs_rowsum against the extended-precision mirror (ksd_sampled_mirror.py), per
entry, in units of EPS64 = 2^-52.  The constants come from the kernels' own operation chains (kernels_ksd_sampled.hip), not
from what the kernels give; the worst ratio error / bound is printed beside each.

Scores.  S[b, i] = 1 - prod over the k affected factors of a quotient of two floored factors: k quotients, k - 1 products and
one subtraction, 2 k roundings = k units of EPS64 on a quantity of size at most 1 + |ratio|; the bound the issue sets is
(2 k + 2) EPS64 (1 + |ratio|).  logp is bit-equal to bornvi_bn_logjoint_samples.

Row sums.  The kernel evaluates kappa in the Gram arrangement (mirror: gemm_form), whose absolute-term sum A is at most
AMPLIFICATION = 4 times the closed form's B~ for n l >= 1 (test_ksd_sampled_host.py).  One entry: c_entry(n) = (5 n + 18) / 2
units of A (mirror: c_entry lists the roundings), so C_entry = 4 c_entry(n) units of B~.  A row sum adds its entries in a
chain of 2 per tile of its column range, a 16-lane butterfly and the G partials: C_sum = c_sum(B) units of sum |kappa| <=
sum B~.  The total adds ceil(B / 256) row sums per thread, a 64-lane butterfly and four waves: c_total(B) more.
  |r_b - ref_b| <= EPS64 (C_entry + C_sum) sum_{b' != b} B~_bb',   |T - ref| <= EPS64 (C_entry + C_sum + C_total) sum_b sum_{b' != b} B~_bb'.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import hp_reference as hp
import ksd_sampled_mirror as km
from tensornetworks_amd import backend
from tensornetworks_amd.backend import bn_score_samples, stein_pairs_rowsum  # noqa: F401  (fails at import without the feature)

pytestmark = pytest.mark.gpu
EPS = hp.EPS64


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _network(name):
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
    if name == "sprinkler":
        return get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], {'W': 1}
    return synthetic_network(int(name), 0)


def _indices(rng, n, B):
    idx = rng.integers(0, 1 << n, B, dtype=np.int64) if n < 63 else rng.integers(0, 1 << 62, B, dtype=np.int64) * 2 + rng.integers(0, 2, B)
    idx[0] = 0
    if B > 1:
        idx[1] = (1 << n) - 1
    return idx


def _score_check(tag, packed, n, idx, p_floor=1e-30):
    keep, desc = backend.bn_descriptor(packed, dev())
    ti = torch.from_numpy(idx).to(dev())
    S, logp = backend.bn_score_samples(desc, n, ti, p_floor, want_logp=True)
    S2 = backend.bn_score_samples(desc, n, ti, p_floor)
    assert torch.equal(S, S2)
    assert torch.equal(logp, backend.bn_logjoint_samples(desc, n, ti, p_floor)), tag
    ref, R, k = km.scores(packed, idx, n, p_floor)
    got = S.cpu().numpy()
    assert got.shape == (len(idx), n) and np.all(np.isfinite(got)), tag
    ratio = hp.ratio(got, ref, (2 * k[None, :] + 2) * (1 + R))
    w = hp.worst(ratio)
    print(f"scores {tag} B={len(idx)}: worst error / bound = {w[0]:.3f} at {w[1]} (k <= {int(k.max())})")
    assert w[0] <= 1.0, (tag, w)
    return got, R, k


@pytest.mark.parametrize("name", ["sprinkler", "1", "2", "12", "33", "63"])
def test_scores_against_the_mirror(name):
    from tensornetworks_amd.bayesian_network import pack_network
    bn, lat, obs, x = _network(name)
    n = len(lat)
    packed = pack_network(bn, lat, x)
    rng = np.random.default_rng(100 + n)
    for B in (1, 63, 64, 65, 257):
        _score_check(name, packed, n, _indices(rng, n, B))


def test_scores_with_a_zero_cpt_entry():
    """A CPT entry of exactly 0 (its complement 1): every factor is floored, so every score is finite and within the bound."""
    from tensornetworks_amd.bayesian_network import pack_network
    bn, lat, obs, x = _network("12")
    packed = {k: np.array(v, copy=True) for k, v in pack_network(bn, lat, x).items()}
    off = int(packed["cpt_off"][5])
    packed["cpt"][off], packed["cpt"][off + 1] = 0.0, 1.0
    got, R, _ = _score_check("zero entry", packed, 12, _indices(np.random.default_rng(7), 12, 257))
    assert hp.to_f64(R).max() > 1e20          # (the floored factor was met: a ratio of about 1 / p_floor)


@pytest.mark.parametrize("name", ["sprinkler", "1", "2", "4", "5"])
def test_scores_agree_with_the_table_kernel(name):
    """Every outcome of a small network, where no p(x, z) is below 1e-12: the rows equal backend.score_from_packed's, each to
    the sum of the two kernels' bounds (hp.score_constants for the table's)."""
    from tensornetworks_amd.bayesian_network import pack_network
    bn, lat, obs, x = _network(name)
    n = len(lat)
    packed = pack_network(bn, lat, x)
    idx = np.arange(1 << n, dtype=np.int64)
    got, R, k = _score_check(name + " (all outcomes)", packed, n, idx)
    S_tab, pxz = backend.score_from_packed(packed, n, dev())
    assert float(pxz.min()) >= 1e-12
    bound = EPS * ((2 * k[None, :] + 2) + hp.score_constants(packed)[1]) * hp.to_f64(1 + R)
    assert np.all(np.abs(got - S_tab.cpu().numpy()) <= bound)


def test_scores_refuse_a_summed_out_node():
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    from tensornetworks_amd._ext import BornviError
    keep, desc = backend.bn_descriptor(pack_network(get_sprinkler_network(False), ['C', 'S'], {'W': 1}), dev())   # R is summed out
    with pytest.raises(BornviError, match="summed-out"):
        backend.bn_score_samples(desc, 2, torch.zeros(4, dtype=torch.int64, device=dev()))


# ------------------------------------------------------------------------------------------------- row sums
def _network_scores(n, idx):
    from tensornetworks_amd.bayesian_network import pack_network
    bn, lat, obs, x = _network("sprinkler" if n == 3 else str(n))
    keep, desc = backend.bn_descriptor(pack_network(bn, lat, x), dev())
    return backend.bn_score_samples(desc, n, torch.from_numpy(idx).to(dev())).cpu().numpy()


def _mixed_scores(rng, B, n):
    return rng.standard_normal((B, n)) * rng.choice([0.01, 1.0, 30.0], size=(B, 1))


def _rowsum_check(tag, n, B, ls, idx, S):
    ti, tS = torch.from_numpy(idx).to(dev()), torch.from_numpy(np.ascontiguousarray(S)).to(dev())
    r, T = backend.stein_pairs_rowsum(ti, tS, n, ls)
    r2, T2 = backend.stein_pairs_rowsum(ti, tS, n, ls)
    assert torch.equal(r, r2) and torch.equal(T, T2), tag                  # two calls are bitwise equal
    K, Bt = km.kappa(idx, S, n, ls)
    ref_r, ref_T = km.rowsums(K)
    bnd_r, bnd_T = km.rowsums(Bt)
    Ce, Cs, Ct = km.AMPLIFICATION * km.c_entry(n), km.c_sum(B), km.c_total(B)
    wr = hp.worst(hp.ratio(r.cpu().numpy(), ref_r, (Ce + Cs) * bnd_r))
    wt = hp.worst(hp.ratio(T.cpu().numpy(), np.atleast_1d(ref_T), (Ce + Cs + Ct) * np.atleast_1d(bnd_T)))
    print(f"row sums {tag} n={n} B={B} l={ls:.4g}: worst error / bound = {wr[0]:.4f} (rows), {wt[0]:.4f} (total); C = {Ce + Cs:.0f}")
    assert wr[0] <= 1.0 and wt[0] <= 1.0, (tag, wr, wt)
    return r.cpu().numpy(), float(T.item()), (K, Bt)


ROWSUM_CASES = [(1, 3, 1.0), (2, 200, 0.5), (3, 64, 1.0), (3, 65, 1.0), (12, 257, 0.25), (33, 129, 1.0), (63, 63, 1.0),
                (63, 513, 1.0 / 63), (3, 2081, 1.0)]


@pytest.mark.parametrize("n,B,ls", ROWSUM_CASES)
def test_row_sums_against_the_mirror(n, B, ls):
    """The issue's shapes, and B = 2081: past 2048 samples a column range has two tiles (asserted), so 2081 lies past the
    first column-range boundary (64 columns) of the geometry actually built, with a last tile of one column."""
    if B == 2081:
        assert backend.stein_pairs_geometry(B)[0] >= 2 and km.pairs_geometry(B) == backend.stein_pairs_geometry(B)
    rng = np.random.default_rng(1000 * n + B)
    idx = _indices(rng, n, B)
    _rowsum_check("network scores", n, B, ls, idx, _network_scores(n, idx))
    _rowsum_check("mixed magnitudes", n, B, ls, idx, _mixed_scores(rng, B, n))


def test_duplicates_all_equal():
    """All B = 65 samples the same state: r_b = (B - 1) k_p(z, z).  A kernel that drops pairs at Hamming distance 0 gives 0."""
    n, B = 12, 65
    rng = np.random.default_rng(5)
    idx = np.full(B, int(rng.integers(0, 1 << n)), dtype=np.int64)
    S = np.repeat(_mixed_scores(rng, 1, n), B, axis=0)
    r, T, (K, Bt) = _rowsum_check("duplicates", n, B, 1.0, idx, S)
    kzz = float(hp.to_f64(K[0, 0]))
    assert kzz != 0.0
    Ce, Cs = km.AMPLIFICATION * km.c_entry(n), km.c_sum(B)
    assert np.all(np.abs(r - (B - 1) * kzz) <= EPS * (Ce + Cs + 1) * (B - 1) * float(hp.to_f64(Bt[0, 0])))


def test_duplicates_against_the_dense_gram():
    """n = 2, B = 200: with c the sample counts per outcome and K = backend.stein_gram, T = c^T K c - sum_z c_z K_zz: the
    diagonal of K_p is in, once per ordered pair of distinct samples of the same state.  Bound: the row-sum kernel's, plus the
    dense Gram's own hp.gram_constant units per entry, plus the host's c^T K c in float64 (16 terms: 16 units)."""
    from tensornetworks_amd.bayesian_network import pack_network
    n, B, ls = 2, 200, 0.5
    bn, lat, obs, x = _network("2")
    packed = pack_network(bn, lat, x)
    S_tab, _ = backend.score_from_packed(packed, n, dev())
    Kd = backend.stein_gram(S_tab, n, ls).cpu().numpy()
    idx = _indices(np.random.default_rng(2200), n, B)
    S = S_tab.cpu().numpy()[idx]
    r, T, (K, Bt) = _rowsum_check("n = 2 table scores", n, B, ls, idx, S)
    c = np.bincount(idx, minlength=4).astype(np.float64)
    want = c @ Kd @ c - (c * np.diagonal(Kd)).sum()
    _, bnd_T = km.rowsums(Bt)
    C_all = km.AMPLIFICATION * km.c_entry(n) + km.c_sum(B) + km.c_total(B) + float(np.max(hp.gram_constant(n, 2))) + 16
    print(f"T = {T!r}, c^T K c - sum c_z K_zz = {want!r}, |difference| / bound = {abs(T - want) / (EPS * C_all * float(bnd_T)):.4f}")
    assert abs(T - want) <= EPS * C_all * float(bnd_T)
    by_distance = c @ Kd @ c - (c * c * np.diagonal(Kd)).sum()
    assert abs(T - by_distance) > 1e-6 * abs(want)           # (what a distance-0 mask would have given is far away)


# ------------------------------------------------------------------------------------------------- contract
def test_capture_and_replay():
    """Scores and row sums captured into one graph: the replay equals the eager calls bit for bit."""
    from tensornetworks_amd.bayesian_network import pack_network
    n, B, ls = 12, 257, 0.25
    bn, lat, obs, x = _network("12")
    keep, desc = backend.bn_descriptor(pack_network(bn, lat, x), dev())
    idx = torch.from_numpy(_indices(np.random.default_rng(3), n, B)).to(dev())
    S_e, lp_e = backend.bn_score_samples(desc, n, idx, want_logp=True)
    r_e, T_e = backend.stein_pairs_rowsum(idx, S_e, n, ls)
    S = torch.zeros(B, n, dtype=torch.float64, device=dev())
    r = torch.zeros(B, dtype=torch.float64, device=dev())
    T = torch.zeros(1, dtype=torch.float64, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        backend.stein_pairs_rowsum(idx, S_e, n, ls)               # the side stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        backend.bn_score_samples(desc, n, idx, out=S)
        backend.stein_pairs_rowsum(idx, S, n, ls, out=r, total=T)
    for _ in range(2):
        r.zero_()
        T.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(S, S_e) and torch.equal(r, r_e) and torch.equal(T, T_e)


def test_refused_sizes():
    """n = 64, B = 1, B = cap + 1 and n l < 1: BORNVI_ERR_UNSUPPORTED (-4) comes back and nothing is launched (the outputs
    keep their sentinels)."""
    from tensornetworks_amd import _ext
    h = _ext.handle_for(dev())
    lib = _ext.lib()
    cap = backend.STEIN_PAIRS_MAX_BATCH
    assert lib.bornvi_stein_pairs_workspace_bytes(h.h, 64, 8) == 0 and lib.bornvi_stein_pairs_workspace_bytes(h.h, 8, 1) == 0
    assert lib.bornvi_stein_pairs_workspace_bytes(h.h, 8, cap + 1) == 0 and lib.bornvi_stein_pairs_workspace_bytes(h.h, 63, cap) > 0
    idx = torch.zeros(8, dtype=torch.int64, device=dev())
    S = torch.zeros(8, 64, dtype=torch.float64, device=dev())
    r = torch.full((8,), 7.0, dtype=torch.float64, device=dev())
    T = torch.full((1,), 7.0, dtype=torch.float64, device=dev())
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    st = _ext.stream_ptr(dev())
    for n, B, ls in ((64, 8, 1.0), (8, 1, 1.0), (8, cap + 1, 1.0), (8, 8, 0.1), (8, 8, float("nan"))):
        rc = lib.bornvi_stein_pairs_rowsum(h.h, n, B, C.c_double(ls), idx.data_ptr(), S.data_ptr(), r.data_ptr(), T.data_ptr(),
                                           ws.data_ptr(), ws.numel(), st)
        assert rc == -4, (n, B, ls, rc)
    keep, desc = backend.bn_descriptor({"role": np.array([0], np.int32), "n_parents": np.array([0], np.int32),
                                        "parents": np.zeros((1, 8), np.int32), "cpt_off": np.array([0], np.int32),
                                        "cpt": np.array([0.5, 0.5])}, dev())
    for n, B in ((64, 8), (0, 8), (8, 0), (8, (1 << 24) + 1)):
        rc = lib.bornvi_bn_score_samples(h.h, C.byref(desc), n, B, idx.data_ptr(), C.c_double(1e-30), S.data_ptr(), None, st)
        assert rc == -4, (n, B, rc)
    torch.cuda.synchronize()
    assert torch.all(r == 7.0) and torch.all(T == 7.0) and torch.all(S == 0.0)
