"""The sampled trainers' posterior queries on the MI355X: an 8-variable chain, D = 4, 60 reverse-KL epochs.  The marginals
against the enumerated q of the same machine, evidence by variable name, and a training run that the queries leave alone."""
import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_query_mirror as qm
import mps_sampled_mirror as sm
from test_gpu_mps_query_kernel import c_marg

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
N, D, B, EPOCHS, LR = 8, 4, 512, 60, 0.05


def make():
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import synthetic_network
    bn, lat, obs, x = synthetic_network(N, 0)
    torch.manual_seed(3)
    vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 7}, device='cuda')
    return vi, lat, x


def query_everything(vi, lat):
    vi.posterior_marginals()
    vi.born_machine.pair_marginals()
    vi.posterior_log_marginal([{lat[0]: 1}, {lat[2]: 0, lat[5]: 1}])
    vi.posterior_sample_given({lat[1]: 1}, 33)
    vi.born_machine.sample_given({}, 33, epoch=1)


def test_queries_of_a_trained_machine_and_an_undisturbed_run():
    plain, lat, x = make()
    h1 = [plain.train(x, EPOCHS // 2, LR, verbose=False), plain.train(x, EPOCHS // 2, LR, verbose=False)]
    vi, _, _ = make()
    query_everything(vi, lat)
    h2 = [vi.train(x, EPOCHS // 2, LR, verbose=False)]
    query_everything(vi, lat)
    h2.append(vi.train(x, EPOCHS // 2, LR, verbose=False))
    query_everything(vi, lat)
    # the history and the final cores are those of the run that never called a query, bit for bit
    assert h1 == h2
    assert torch.equal(plain.born_machine.cores.detach(), vi.born_machine.cores.detach())
    assert torch.equal(plain.last_idx, vi.last_idx)

    # posterior_marginals against the enumerated q of the same machine, within the kernel's bound (C_M against the sums of
    # magnitudes, test_gpu_mps_query_kernel.py) and q64's own (test_gpu_mps_kernel.py: (2 C_PSI + 1)(kappa_z + kappa_Z) + 2 + T_Z)
    cores = vi.born_machine.cores.detach().cpu().numpy()
    env = sm.environments(cores)
    kZ = float(env["Z_abs"] / env["Z"])
    ref = qm.marginals(cores, env)
    q = vi.born_machine.probabilities64().detach().cpu().numpy().astype(sm.LD)
    bits = sm.bits_of_idx(np.arange(1 << N), N)
    cond = sm.conditionals(cores, bits, env)
    with np.errstate(divide="ignore", invalid="ignore"):
        kz = np.where(cond["psi"] != 0, cond["psi_abs"] / np.abs(cond["psi"]), 0)
    werr = q * ((2 * (N * D + 2) + 1) * (kz + kZ) + 2 + 29)
    got = vi.posterior_marginals()
    assert list(got) == lat
    worst = 0.0
    for k, name in enumerate(lat):
        ok = bits[:, k] == 1
        lim = float(hp.to_f64(EPS * (c_marg(N, D, kZ) * ref["m1_abs"][k] + werr[ok].sum())))
        err = abs(float(hp.to_f64(sm.LD(got[name]) - q[ok].sum())))
        worst = max(worst, err / lim)
        assert err <= lim, name
    print(f"worst |posterior_marginals - enumerated| / bound = {worst:.3f}")

    # evidence by name
    ev = {lat[1]: 1, lat[6]: 0}
    idx, logq, logm = vi.posterior_sample_given(ev, 257, epoch=2)
    z = sm.bits_of_idx(idx.cpu().numpy(), N)
    assert np.all(z[:, 1] == 1) and np.all(z[:, 6] == 0) and bool(torch.isfinite(logq).all())
    lm = vi.posterior_log_marginal(ev)
    assert torch.equal(lm, logm)
    both = vi.posterior_log_marginal([ev, {}])
    assert torch.equal(both[:1], lm) and float(both[1].item()) == 0.0
    want = q[(bits[:, 1] == 1) & (bits[:, 6] == 0)].sum()
    assert abs(float(np.exp(sm.LD(float(lm.item()))) / want) - 1.0) <= 1e-12
    for t in (idx, logq, logm, lm):
        assert t.device.type == "cuda" and not t.requires_grad
