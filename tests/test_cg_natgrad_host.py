"""The matrix-free CG natural gradient on the host: the mirrors (cg_natgrad_mirror.py) against autograd and against the
Cholesky solve of sampled_fisher_mirror.py, the 'cg' keyword, the constructor and every refused shape.  No GPU."""
import numpy as np
import pytest
import torch

import cg_natgrad_mirror as cm
import hp_reference as hp
import mps_sampled_mirror as sm
import sampled_fisher_mirror as fm
from tensornetworks_amd.backend import cg_finish, cg_init, cg_step, mps_score_jvp  # noqa: F401  (fails without the feature)
from tensornetworks_amd.natural_gradient import (CGFisherPreconditioner, SampledFisherPreconditioner,
                                                 SampleSpaceFisherPreconditioner)
from test_sampled_natgrad_host import make_cores

EPS = hp.EPS64


@pytest.mark.parametrize("n,D", [(3, 2), (5, 3)])
def test_the_mirror_jvp_is_the_directional_derivative_of_log_q(n, D):
    """<grad log q(z_b), v> by forward-over-reverse autograd on mps_sampled_mirror.logq_torch (float64) against the mirror's
    rows . v: within 1e-12 of the largest |t| (float64 autograd of a handful of D-term chains)."""
    cores = make_cores(n, D, seed=3)
    rng = np.random.default_rng([n, D, 1])
    bits = rng.integers(0, 2, size=(24, n))
    v = rng.standard_normal(tuple(cores.shape))
    _, t = torch.autograd.functional.jvp(lambda A: sm.logq_torch(A, bits), cores, torch.from_numpy(v))
    ref = cm.jvp(cores.numpy(), bits, v)
    err = np.abs(t.numpy() - hp.to_f64(ref["t"])).max() / np.abs(hp.to_f64(ref["t"])).max()
    print(f"n={n} D={D}: |autograd jvp - mirror| / max|t| = {err:.2e}")
    assert err <= 1e-12
    assert np.all(ref["t_abs"] >= np.abs(ref["t"]))
    # the gauge direction: q does not change under a common scale of the cores
    gauge = cm.jvp(cores.numpy(), bits, cores.numpy(), sr=ref["sr"])
    assert np.abs(hp.to_f64(gauge["t"])).max() <= 1e-15 * float(gauge["t_abs"].max())


@pytest.mark.parametrize("dtype", [np.float64, cm.LD])
def test_the_mirror_cg_reproduces_the_cholesky_solve(dtype):
    """n = 3, D = 2 (P = 24), B = 40, lam = 1e-2: K = P + 5 iterations at rel_tol = 0 against damped_solve on the full matrix,
    within 1e3 EPS amp, amp = (||F||_inf + lam) / lam (the chain tests' convention)."""
    n, D, Bs, lam = 3, 2, 40, 1e-2
    cores = make_cores(n, D, seed=3).numpy()
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, size=(Bs, n))
    g = rng.standard_normal(2 * n * D * D)
    X = fm.score_rows(cores, bits, dtype=dtype)["rows"].reshape(-1, Bs)
    F = fm.fisher(X.reshape(n, -1, Bs))["full"]
    ref = fm.damped_solve(F, g.astype(dtype), lam)
    P = g.size
    out = cm.cg(cm.matvec(X), g, lam, P + 5, 0.0, dtype)
    amp = (float(np.abs(F).sum(axis=1).max()) + lam) / lam
    err = float(np.abs(out["x"] - ref).max() / np.abs(ref).max())
    print(f"{np.dtype(dtype).name}: |cg - cholesky| / |ref| = {err:.2e} after {out['iters']} iterations, relres "
          f"{float(out['relres']):.2e}, bound {1e3 * EPS * amp:.2e}")
    assert out["info"] == 0 and err <= 1e3 * EPS * amp
    assert cm.residual(X, g, out["x"], lam) <= 1e3 * EPS * amp
    # the recurrence's own rules
    assert cm.cg(cm.matvec(X), np.zeros(P), lam, 3, 0.0, dtype)["iters"] == 0
    nan = g.copy()
    nan[5] = np.nan
    bad = cm.cg(cm.matvec(X), nan, lam, 3, 0.0, dtype)
    assert bad["info"] == 1 and bad["iters"] == 0 and np.array_equal(np.isnan(bad["x"]), np.isnan(nan))
    frozen = cm.cg(cm.matvec(X), g, lam, 60, 1e-8, dtype), cm.cg(cm.matvec(X), g, lam, 67, 1e-8, dtype)
    assert frozen[0]["done"] and frozen[0]["iters"] == frozen[1]["iters"] and np.array_equal(frozen[0]["x"], frozen[1]["x"])


def test_keyword_export_and_constructor():
    c = SampledFisherPreconditioner.coerce
    d = c('cg')
    assert isinstance(d, CGFisherPreconditioner) and d.damping == 1e-3 and d.info is None and d.iters is None
    assert d.max_iters == CGFisherPreconditioner.MAX_ITERS and d.rel_tol == CGFisherPreconditioner.REL_TOL
    own = CGFisherPreconditioner(damping=0.5, max_iters=7, rel_tol=0.0)
    assert c(own) is own and (own.damping, own.max_iters, own.rel_tol) == (0.5, 7, 0.0)
    assert isinstance(c('site'), SampledFisherPreconditioner) and isinstance(c('sample'), SampleSpaceFisherPreconditioner)
    with pytest.raises(ValueError, match="'cg'"):
        c('conjugate')
    from tensornetworks_amd import CGFisherPreconditioner as exported
    import tensornetworks_amd
    assert exported is CGFisherPreconditioner and "CGFisherPreconditioner" in tensornetworks_amd.__all__
    for bad in (0, 0.0, -1e-3, float('nan'), float('inf'), True, '1e-3'):
        with pytest.raises(ValueError, match="damping"):
            CGFisherPreconditioner(damping=bad)
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="max_iters"):
            CGFisherPreconditioner(max_iters=bad)
    for bad in (-1e-9, float('nan'), float('inf'), True, '0'):
        with pytest.raises(ValueError, match="rel_tol"):
            CGFisherPreconditioner(rel_tol=bad)


def test_plan_refusals():
    p = CGFisherPreconditioner()
    assert p.plan(40, 4, 4096) == (1280, 1, 40) and p.plan(63, 32, 1 << 24) == (129024, 1, 63) and p.plan(1, 1, 2) == (2, 1, 1)
    for n, D, Bs in ((64, 2, 64), (3, 33, 64), (3, 2, 1), (3, 2, (1 << 24) + 1), (0, 2, 64), (3, 0, 64)):
        with pytest.raises(ValueError):
            p.plan(n, D, Bs)


def test_trainer_plans_the_shape_the_other_full_matrix_steps_refuse():
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn40, lat, obs, _ = synthetic_network(40, 0)
    cfg = {'bond_dim': 4, 'num_samples': 4096}
    for cls in (SampledELBOVariationalInference, SampledKSDVariationalInference):
        vi = cls(bn40, lat, obs, cfg, natural_gradient='cg')
        assert isinstance(vi.natural_gradient, CGFisherPreconditioner)
        assert vi.natural_gradient.plan(40, 4, 4096) == (1280, 1, 40)
        for spec in ('full', 'sample'):
            with pytest.raises(ValueError):
                cls(bn40, lat, obs, cfg, natural_gradient=spec)
