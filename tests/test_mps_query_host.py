"""The sampled MPS Born machine's exact queries on the CPU: the mirror (mps_query_mirror.py) against brute-force sums over all
2^n states, the evidence packing and every host-side refusal, the trainers' name mapping.  No GPU needed."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_query_mirror as qm
import mps_sampled_mirror as sm
from tensornetworks_amd.born_machine_base import pack_evidence
from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine

# long double carries 64 bits where it exists; the sums have at most 2^8 terms of products of 8 D-term chains
TOL = 1e-15 if hp.HAVE_LONGDOUBLE else 1e-11


def cores_of(n, D, seed=0):
    rng = np.random.default_rng([n, D, seed])
    return (np.eye(D)[None, None] + 0.4 * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0)


def evidences(n, seed=0):
    rng = np.random.default_rng([n, seed, 77])
    full = {p: int(rng.integers(0, 2)) for p in range(n)}
    out = [{}, full, {0: 1}, {n - 1: 0}, {p: int(rng.integers(0, 2)) for p in range(0, n, 2)}]
    out.append({p: int(rng.integers(0, 2)) for p in range(n) if rng.random() < 0.5})
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("D", [1, 2, 3, 5])
def test_mirror_against_enumeration(n, D):
    cores = cores_of(n, D)
    br = qm.brute(cores)
    q, bits = br["q"], br["bits"]
    env = sm.environments(cores)
    for ev in evidences(n):
        ok = qm.consistent(bits, ev)
        want = q[ok].sum()
        got = np.exp(qm.log_marginal(cores, ev, env)["logm"])
        assert abs(got - want) <= TOL * want, (ev, got, want)
    assert qm.log_marginal(cores, {}, env)["logm"] == 0
    m = qm.marginals(cores, env)
    one = bits.astype(bool)
    for i in range(n):
        assert abs(m["m1"][i] - q[one[:, i]].sum()) <= TOL
        for j in range(n):
            assert abs(m["m2"][i, j] - q[one[:, i] & one[:, j]].sum()) <= TOL
    assert np.all(m["m1_abs"] >= np.abs(m["m1"])) and np.all(m["m2_abs"] >= np.abs(m["m2"]))
    # the clamped sampler's conditionals along every consistent state: p1 is q(z_k = 1 | evidence, the prefix) and the
    # conditional log q sums with the log marginal to log q
    for ev in evidences(n)[1:]:
        ok = qm.consistent(bits, ev)
        c = qm.conditionals_clamped(cores, ev, bits[ok])
        mass = q[ok].sum()
        assert np.all(np.abs(np.exp(c["logq"]) - q[ok] / mass) <= TOL * 8)
        zb = bits[ok]
        for k in range(n):
            if k in ev:
                assert np.all(np.isnan(c["p1"][:, k]))
                continue
            for row in range(min(len(zb), 16)):
                pre = ok & np.all(bits[:, :k] == zb[row, :k], axis=1)
                want = q[pre & (bits[:, k] == 1)].sum() / q[pre].sum()
                assert abs(c["p1"][row, k] - want) <= TOL * 8
    s = qm.sample_clamped(cores, evidences(n)[4], 5, 1, 32)
    assert np.all(qm.consistent(s["bits"], evidences(n)[4]))
    free = qm.sample_clamped(cores, {}, 5, 1, 32)
    plain = sm.sample(cores, 5, 1, 32)
    assert np.array_equal(free["idx"], plain["idx"]) and free["undecided"] == plain["undecided"]


def test_evidence_packing():
    n = 5
    m, v = pack_evidence({0: 1, 4: 0, 2: 1}, n)
    assert m.dtype == torch.int64 and m.tolist() == [0b10101] and v.tolist() == [0b10100]
    assert pack_evidence({}, n)[0].tolist() == [0]
    m, v = pack_evidence([{1: 1}, {}, {3: 0, 4: 1}], n)
    assert m.tolist() == [0b01000, 0, 0b00011] and v.tolist() == [0b01000, 0, 0b00001]
    m, v = pack_evidence(({np.int64(1): np.int64(1)},), n)              # a tuple of dicts, NumPy integers
    assert m.tolist() == [0b01000] and v.tolist() == [0b01000]
    # the top position of n = 63 is bit 62: inside int64
    m, v = pack_evidence({0: 1, 62: 1}, 63)
    assert m.tolist() == [(1 << 62) | 1] and v.tolist() == [(1 << 62) | 1]
    for ev in ({}, {0: 1, 3: 0}, {4: 1}):
        assert tuple(int(t) for t in pack_evidence(ev, n)) == qm.words(ev, n)
    # tensors pass through; on the CPU the bits at or above n are checked
    tm, tv = torch.tensor([3, 0], dtype=torch.int64), torch.tensor([1, 0], dtype=torch.int64)
    m, v = pack_evidence((tm, tv), n)
    assert torch.equal(m, tm) and torch.equal(v, tv)
    m, v = pack_evidence((torch.tensor(3), torch.tensor(2)), n)          # 0-dim: one query
    assert m.tolist() == [3] and v.tolist() == [2]
    with pytest.raises(ValueError, match="at or above"):
        pack_evidence((torch.tensor([1 << 5]), torch.tensor([0])), n)
    with pytest.raises(ValueError, match="at or above"):
        pack_evidence((torch.tensor([0]), torch.tensor([-1])), 63)
    with pytest.raises(ValueError, match="int64"):
        pack_evidence((torch.tensor([1], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)), n)
    with pytest.raises(ValueError, match="int64"):
        pack_evidence((torch.tensor([1, 2]), torch.tensor([0])), n)


def test_refusals_before_any_gpu_call():
    bm = SampledMPSBornMachine(6, bond_dim=2)
    for bad in ({6: 1}, {-1: 0}, {True: 1}, {"a": 1}, {1.0: 1}):
        with pytest.raises(ValueError, match="position"):
            bm.log_marginal(bad)
        with pytest.raises(ValueError, match="position"):
            bm.sample_given(bad, 4)
    for bad in (2, -1, True, 0.0, None):
        with pytest.raises(ValueError, match="must be 0 or 1"):
            bm.log_marginal({0: bad})
    with pytest.raises(ValueError, match="queries"):
        bm.log_marginal([])
    with pytest.raises(ValueError, match="queries"):
        bm.log_marginal([{}] * ((1 << 16) + 1))
    with pytest.raises(ValueError, match="queries"):
        bm.log_marginal((torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)))
    with pytest.raises(ValueError, match="dict"):
        bm.log_marginal([{0: 1}, 3])
    with pytest.raises(ValueError, match="evidence"):
        bm.log_marginal(7)
    for bad in (True, 4.0, "4", 0, -2, None):
        with pytest.raises(ValueError, match="num_samples"):
            bm.sample_given({0: 1}, bad)
    with pytest.raises(ValueError, match="one evidence"):
        bm.sample_given([{0: 1}, {1: 0}], 4)
    with pytest.raises(ValueError, match="seed"):
        bm.sample_given({0: 1}, 4, seed=1.5)
    with pytest.raises(ValueError, match="epoch"):
        bm.sample_given({0: 1}, 4, epoch=True)


def test_trainer_name_mapping():
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(8, 0)
    for cls in (SampledELBOVariationalInference, SampledKSDVariationalInference):
        vi = cls(bn, lat, obs, {'bond_dim': 2, 'num_samples': 8})
        assert vi._evidence_by_name({lat[0]: 1, lat[7]: 0}) == {0: 1, 7: 0}
        assert vi._evidence_by_name([{lat[3]: 1}, {}]) == [{3: 1}, {}]
        with pytest.raises(ValueError, match="observed"):
            vi.posterior_log_marginal({obs[0]: 1})
        with pytest.raises(ValueError, match="not a latent"):
            vi.posterior_log_marginal({"no such variable": 1})
        with pytest.raises(ValueError, match="not a latent"):
            vi.posterior_sample_given({"no such variable": 1}, 4)
        with pytest.raises(ValueError, match="must be 0 or 1"):
            vi.posterior_log_marginal([{lat[0]: 1}, {lat[1]: 2}])
        with pytest.raises(ValueError, match="num_samples"):
            vi.posterior_sample_given({lat[0]: 1}, True)
        with pytest.raises(ValueError, match="evidence"):
            vi.posterior_sample_given([{lat[0]: 1}], 4)
