"""The sample-space natural gradient on the host: the push-through identity in the mirrors (sample_gram_mirror.py against
sampled_fisher_mirror.py), the 'sample' keyword, the constructor and every refused shape, and the float64 replays of the two
Sprinkler traces against each other.  No GPU."""
import numpy as np
import pytest
import torch

import mps_sampled_mirror as sm
import sample_gram_mirror as gm
import sampled_fisher_mirror as fm
from tensornetworks_amd.natural_gradient import SampledFisherPreconditioner, SampleSpaceFisherPreconditioner
from test_sampled_natgrad_host import make_cores

EPOCHS, LR, B = 40, 0.05, 1024
TRACE = {"elbo": dict(seed=5, damping=1e-3), "ksd": dict(seed=6, damping=1e-1)}


@pytest.mark.parametrize("lam", [1e-1, 1e-3])
@pytest.mark.parametrize("n,D,Bs", [(3, 2, 16), (3, 2, 64), (4, 3, 32), (4, 3, 200)])
def test_the_dual_solve_is_the_primal_full_solve(n, D, Bs, lam):
    """delta = (O^T O / B + lam I)^-1 O^T w = O^T (O O^T / B + lam I)^-1 w in extended precision, B < P and B > P
    (P = 24, 72): 1.5e-14 at the worst of the eight cases, (3, 2, 64) at lam = 1e-3."""
    cores = make_cores(n, D, seed=3).numpy()
    rng = np.random.default_rng([n, D, Bs])
    bits = rng.integers(0, 2, size=(Bs, n))
    bits[1] = bits[0]                                                  # a repeated sample: T itself is singular
    w = rng.standard_normal(Bs)
    g = sm.score_gradient(cores, bits, w)["grad"]
    primal, pinfo = fm.precondition(cores, bits, g, lam, "full")
    dual, dinfo = gm.precondition(cores, bits, w, lam)
    assert pinfo.tolist() == [0] and dinfo.tolist() == [0]
    rel = float(np.abs(dual - primal).max() / np.abs(primal).max())
    print(f"n={n} D={D} B={Bs} lam={lam}: |dual - primal| / |primal| = {rel:.2e}")
    assert rel <= 1e-12
    G = gm.sample_gram(cores, bits)
    assert np.array_equal(G["T"], G["T"].T) and np.all(G["T_abs"] >= np.abs(G["T"]))
    assert np.array_equal(G["T"][0], G["T"][1])


def test_keyword_export_and_constructor():
    c = SampledFisherPreconditioner.coerce
    d = c('sample')
    assert isinstance(d, SampleSpaceFisherPreconditioner) and d.damping == 1e-3 and d.info is None
    own = SampleSpaceFisherPreconditioner(damping=0.5)
    assert c(own) is own and own.damping == 0.5
    assert isinstance(c('site'), SampledFisherPreconditioner) and isinstance(c(True), SampledFisherPreconditioner)
    from tensornetworks_amd import SampleSpaceFisherPreconditioner as exported
    import tensornetworks_amd
    assert exported is SampleSpaceFisherPreconditioner and "SampleSpaceFisherPreconditioner" in tensornetworks_amd.__all__
    for bad in (0, 0.0, -1e-3, float('nan'), float('inf'), True, '1e-3'):
        with pytest.raises(ValueError, match="damping"):
            SampleSpaceFisherPreconditioner(damping=bad)


def test_plan_refusals():
    p = SampleSpaceFisherPreconditioner()
    assert p.plan(40, 4, 1024) == (1024, 1, 40) and p.plan(63, 32, 1024) == (1024, 1, 63) and p.plan(1, 1, 2) == (2, 1, 1)
    for n, D, Bs in ((3, 2, 1), (0, 2, 64), (64, 2, 64), (3, 33, 64), (3, 0, 64)):
        with pytest.raises(ValueError):
            p.plan(n, D, Bs)
    with pytest.raises(ValueError, match="1025 samples; the device solve holds at most 1024"):
        p.plan(3, 2, 1025)


def test_trainer_refuses_too_many_samples_at_construction():
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
    bn = get_sprinkler_network(False)
    for cls in (SampledELBOVariationalInference, SampledKSDVariationalInference):
        with pytest.raises(ValueError, match="2048 samples; the device solve holds at most 1024"):
            cls(bn, ['C', 'S', 'R'], ['W'], {'bond_dim': 2, 'num_samples': 2048}, natural_gradient='sample')
        vi = cls(bn, ['C', 'S', 'R'], ['W'], {'bond_dim': 2, 'num_samples': 1024}, natural_gradient='sample')
        assert isinstance(vi.natural_gradient, SampleSpaceFisherPreconditioner)
    bn40, lat, obs, _ = synthetic_network(40, 0)                       # the shape blocks='full' refuses
    vi = SampledELBOVariationalInference(bn40, lat, obs, {'bond_dim': 4, 'num_samples': 1024}, natural_gradient='sample')
    assert vi.natural_gradient.plan(40, 4, 1024) == (1024, 1, 40)


@pytest.mark.parametrize("kind", ["elbo", "ksd"])
def test_float64_replays_agree(kind):
    """The Sprinkler traces of test_gpu_sampled_natgrad_trainer.py (n = 3, D = 2, B = 1024, 40 epochs, SGD, lr 0.05): the
    float64 replay with the sample-space solve against the float64 replay with blocks='full', within 1e-8 in the loss and the
    step norm (5.4e-13 for the ELBO trace at damping 1e-3, 3.5e-10 for the KSD trace at 1e-1); the same samples in every
    epoch and no failed solve."""
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, pack_network
    seed, lam = TRACE[kind]["seed"], TRACE[kind]["damping"]
    bn = get_sprinkler_network(False)
    lat, obs, x = ['C', 'S', 'R'], ['W'], {'W': 1}
    torch.manual_seed(11)
    cls = SampledELBOVariationalInference if kind == "elbo" else SampledKSDVariationalInference
    vi = cls(bn, lat, obs, {'bond_dim': 2, 'num_samples': B, 'seed': seed})
    cores0 = vi.born_machine.cores.detach().cpu().numpy().copy()
    packed = pack_network(bn, lat, x)
    dual = gm.replay(kind, cores0, packed, B, seed, EPOCHS, LR, lam)
    full = fm.replay(kind, cores0, packed, B, seed, EPOCHS, LR, lam, "full", momentum=0.0)
    dl = np.abs(np.array(dual["loss"]) - np.array(full["loss"])).max()
    dg = np.abs(np.array(dual["grad_norm"]) - np.array(full["grad_norm"])).max()
    print(f"{kind}: dual against 'full' replay: loss {dl:.2e}, step norm {dg:.2e}")
    assert dl <= 1e-8 and dg <= 1e-8
    assert dual["undecided"] == 0 and full["undecided"] == 0
    assert dual["natgrad_info"] == [0] * EPOCHS and full["natgrad_info"] == [0] * EPOCHS
    assert all(np.array_equal(a, b) for a, b in zip(dual["idx"], full["idx"]))
