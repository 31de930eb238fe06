"""The sampled natural gradient on the host: the identities the mirror (sampled_fisher_mirror.py) and the kernels rest on, the
`natural_gradient` keyword of the sampled trainers and every refused shape.  No GPU."""
import numpy as np
import pytest
import torch

import mps_sampled_mirror as sm
import sampled_fisher_mirror as fm
from tensornetworks_amd.natural_gradient import SAMPLED_ROWS_BUDGET, SampledFisherPreconditioner

SHAPES = [(3, 2), (4, 3)]
TOL = 1e-12


def make_cores(n, D, seed=0):
    gen = torch.Generator().manual_seed(100 * n + D + seed)
    eye = torch.eye(D, dtype=torch.float64).expand(n, 2, D, D)
    return ((eye + 0.3 * torch.randn(n, 2, D, D, dtype=torch.float64, generator=gen)) / np.sqrt(2.0)).contiguous()


@pytest.mark.parametrize("n,D", SHAPES)
def test_exact_fisher_is_the_autograd_fisher(n, D):
    """sum_z q_z o_z o_z^T = J^T diag(1 / q) J with J = dq / dcores = q dlog q / dcores by torch autograd of logq_torch."""
    cores = make_cores(n, D)
    F, sr = fm.exact_fisher(cores.numpy())
    bits = fm.all_bits(n)
    A = cores.clone().requires_grad_(True)
    lq = sm.logq_torch(A, bits)
    J = torch.stack([torch.autograd.grad(lq[z], A, retain_graph=True)[0].reshape(-1) for z in range(1 << n)])   # dlog q_z
    q = torch.exp(lq.detach())
    Fa = (J * q[:, None]).T @ J
    scale = float(np.abs(Fa.numpy()).max())
    assert np.abs(F.astype(np.float64) - Fa.numpy()).max() <= TOL * scale
    assert abs(float(sr["q"].sum()) - 1.0) <= TOL


@pytest.mark.parametrize("n,D", SHAPES)
def test_rows_are_centred_scale_free_and_zero_at_the_boundaries(n, D):
    cores = make_cores(n, D, seed=1)
    sr = fm.score_rows(cores.numpy(), fm.all_bits(n))
    rows = sr["rows"]                                                   # [n, R, 2^n]
    scale = float(np.abs(rows).max())
    assert np.abs((rows * sr["q"][None, None, :]).sum(axis=2)).max() <= TOL * scale        # sum_z q_z o_z = 0
    A = cores.numpy().reshape(n, 2 * D * D)
    assert np.abs(np.einsum('krz,kr->kz', rows, A.astype(rows.dtype))).max() <= TOL * scale  # <o_b[k], vec A_k> = 0
    r5 = rows.reshape(n, 2, D, D, -1)
    assert np.all(r5[0][:, 1:, :, :] == 0.0) and np.all(r5[n - 1][:, :, 1:, :] == 0.0)


@pytest.mark.parametrize("n,D", SHAPES)
def test_site_blocks_are_the_diagonal_blocks(n, D):
    cores = make_cores(n, D, seed=2)
    bits = np.random.default_rng(n + D).integers(0, 2, size=(37, n))
    F = fm.fisher(fm.score_rows(cores.numpy(), bits)["rows"])
    R = 2 * D * D
    for k in range(n):
        assert np.array_equal(F["site"][k], F["full"][k * R:(k + 1) * R, k * R:(k + 1) * R])
    assert np.array_equal(F["full"], F["full"].T) and np.all(np.diag(F["full"]) >= 0)
    # F is singular (rank 7 of 24 at n = 3, D = 2 for the exact matrix): the damping is what makes the solve succeed
    g = np.random.default_rng(1).standard_normal(cores.shape)
    delta, info = fm.precondition(cores.numpy(), bits, g, 1e-3, "site")
    assert np.all(info == 0) and np.all(np.isfinite(delta.astype(np.float64)))
    delta0, info0 = fm.precondition(cores.numpy(), bits, g, 0.0, "full")
    assert info0[0] == 1 and np.array_equal(delta0.astype(np.float64), g)      # the first core's zero rows: pivot 0


def test_exact_fisher_rank():
    F, _ = fm.exact_fisher(make_cores(3, 2).numpy())
    assert np.linalg.matrix_rank(F.astype(np.float64), tol=1e-10) == 7


def test_keyword_coercion():
    c = SampledFisherPreconditioner.coerce
    assert c(None) is None and c(False) is None
    d = c(True)
    assert isinstance(d, SampledFisherPreconditioner) and (d.damping, d.blocks, d.rows_budget_bytes) == (1e-3, 'site', SAMPLED_ROWS_BUDGET)
    assert c(0.25).damping == 0.25 and c(0.25).blocks == 'site' and c(0).damping == 0.0
    assert c('full').blocks == 'full' and c('site').blocks == 'site'
    own = SampledFisherPreconditioner(damping=2.0, blocks='full')
    assert c(own) is own
    for bad in ('quantum', 'diag', [1e-3], object()):
        with pytest.raises(ValueError):
            c(bad)
    from tensornetworks_amd import SampledFisherPreconditioner as exported, backend
    assert exported is SampledFisherPreconditioner and SAMPLED_ROWS_BUDGET <= backend.WORKSPACE_CAP


@pytest.mark.parametrize("kw", [dict(damping=-1e-3), dict(damping=float('nan')), dict(damping=float('inf')), dict(damping=True),
                                dict(damping='1e-3'), dict(blocks='diag'), dict(rows_budget_bytes=0), dict(rows_budget_bytes=1.5),
                                dict(rows_budget_bytes=True)])
def test_bad_constructor_arguments(kw):
    with pytest.raises(ValueError):
        SampledFisherPreconditioner(**kw)


def test_refused_shapes():
    site, full = SampledFisherPreconditioner(), SampledFisherPreconditioner(blocks='full')
    assert site.plan(63, 22, 4096) == (968, 63, min(63, SAMPLED_ROWS_BUDGET // (968 * 4096 * 8)))
    with pytest.raises(ValueError, match="D <= 22"):
        site.plan(3, 23, 64)
    assert full.plan(56, 3, 64) == (1008, 1, 56)
    with pytest.raises(ValueError, match="1026 parameters"):
        full.plan(57, 3, 64)                                           # P = 2 * 57 * 9 = 1026
    with pytest.raises(ValueError, match="1280 parameters"):
        full.plan(40, 4, 1024)
    small = SampledFisherPreconditioner(rows_budget_bytes=32 * 1024 * 8 - 1)
    with pytest.raises(ValueError, match="rows of one site"):
        small.plan(40, 4, 1024)                                        # one site: 32 rows x 1024 columns x 8 bytes
    assert SampledFisherPreconditioner(rows_budget_bytes=32 * 1024 * 8).plan(40, 4, 1024) == (32, 40, 1)
    assert SampledFisherPreconditioner(rows_budget_bytes=32 * 1024 * 8).plan(40, 4, 1000) == (32, 40, 1)   # ld = 1024
    with pytest.raises(ValueError, match="more than"):
        SampledFisherPreconditioner(blocks='full', rows_budget_bytes=32 * 1024 * 8).plan(2, 4, 1024)
    for n, B in ((64, 64), (0, 64), (3, 1), (3, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            site.plan(n, 2, B)


def test_trainers_without_the_keyword_build_nothing():
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
    bn = get_sprinkler_network(False)
    for cls in (SampledELBOVariationalInference, SampledKSDVariationalInference):
        for spec in (None, False):
            vi = cls(bn, ['C', 'S', 'R'], ['W'], {'bond_dim': 2, 'num_samples': 64}, natural_gradient=spec)
            assert vi.natural_gradient is None
        assert cls(bn, ['C', 'S', 'R'], ['W'], {'bond_dim': 2, 'num_samples': 64}).natural_gradient is None
        vi = cls(bn, ['C', 'S', 'R'], ['W'], {'bond_dim': 2, 'num_samples': 64}, natural_gradient=0.5)
        assert vi.natural_gradient.damping == 0.5 and vi.natural_gradient.info is None
    bn40, lat, obs, _ = synthetic_network(40, 0)
    with pytest.raises(ValueError, match="1280 parameters"):
        SampledELBOVariationalInference(bn40, lat, obs, {'bond_dim': 4, 'num_samples': 1024}, natural_gradient='full')
    with pytest.raises(ValueError, match="D <= 22"):
        SampledKSDVariationalInference(bn40, lat, obs, {'bond_dim': 23, 'num_samples': 1024}, natural_gradient=True)
