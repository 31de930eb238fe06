"""Every engine past n = 20, against exact references: the sparse circuit oracle (oracle/sparse_circuit.py), the C port
of the dense oracle, the Stein kernel's closed form and float64 autograd.

Above n = 20 the kernels change regime: the 8-amplitude kernel's 32-bit HBM byte offsets reach bit 30 at n = 27, its
compact tables grow to millions of words and a state has more tiles than the device has CUs; the 16-amplitude kernel
loses its fast tables above n = 25; n = 28 and 29 run 2^13-tile plans on the generic pass kernel.

Conventions of the circuit checks (check_sparse): the GPU result gathered at the oracle's support matches it to 1e-12
relative to its maximum, the rest of the 2^n entries are <= 1e-14 (no mass at a wrong index), and it sums to 1 within
1e-12.  Nothing of size 2^n is copied to the host at n >= 24.  Peak device memory per test stays under 48 GiB."""
import gc
import math

import numpy as np
import pytest
import torch

from oracle import circuit as oc, sparse_circuit as sc, stein as os_

pytestmark = pytest.mark.gpu

G_GENERIC = 6       # generic rotations per circuit: support <= 2^6 (2^9 with the parameter-shift picks and a shift)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def be(dev):
    from tensornetworks_amd import backend
    return backend


@pytest.fixture(autouse=True)
def _free_device_memory(be):
    yield
    be.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture
def r4(be, dev):
    """reg_wires = 4 (16 amplitudes per thread: circuit_pass_fast_kernel, generic kernel beyond its tables), restored after."""
    default_r = be.get_option(dev, "reg_wires")
    be.set_option(dev, "reg_wires", 4)
    yield be
    be.set_option(dev, "reg_wires", default_r)


def sparse_case(ansatz, n, L, seed, g=G_GENERIC):
    rng = np.random.default_rng(seed)
    th, generic = sc.sparse_theta(ansatz, n, L, rng, g=g)
    return th, generic, rng


def check_sparse(q, idx, p, what=""):
    """q: GPU float64 [2^n] (restored on return); (idx, p): the exact sparse probabilities."""
    total = float(q.sum())
    it = torch.as_tensor(idx, device=q.device)
    got = q[it]
    ref = torch.as_tensor(p, device=q.device)
    err = float((got - ref).abs().max())
    assert err <= 1e-12 * float(ref.max()), f"{what}: support mismatch {err:.3e} (max p {float(ref.max()):.3e})"
    q[it] = 0.0
    off = float(q.abs().max())
    q[it] = got
    assert off <= 1e-14, f"{what}: mass {off:.3e} off the support"
    assert abs(total - 1.0) <= 1e-12, f"{what}: sum {total!r}"


def circuit_case(be, dev, ansatz, n, L, seed):
    th, generic, _ = sparse_case(ansatz, n, L, seed)
    q = be.circuit_probs(ansatz, n, L, torch.as_tensor(th, device=dev).reshape(1, -1))[0]
    if L == 0 and ansatz != "basic":       # H on every wire: the uniform distribution, exactly 2^-n per outcome
        assert float((q - 2.0 ** -n).abs().max()) <= 1e-12 * 2.0 ** -n
        assert abs(float(q.sum()) - 1.0) <= 1e-12
        return
    idx, p = sc.probs_sparse(ansatz, n, L, th)
    assert idx.size <= 1 << len(generic)
    check_sparse(q, idx, p, f"{ansatz} n={n} L={L}")


# ---- circuits, default engine (8 amplitudes per thread; 2^13-tile generic plans at n = 28, 29) --------------------
CIRCUIT_CELLS = [(n, L) for n in (21, 22, 24, 26, 27) for L in (1, 2)] + [(27, 0), (28, 1), (28, 2), (29, 1), (29, 2)]


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L", CIRCUIT_CELLS)
def test_circuit_sparse_default_engine(be, dev, ansatz, n, L):
    circuit_case(be, dev, ansatz, n, L, seed=1000 * n + 10 * L + len(ansatz))


@pytest.mark.parametrize("ansatz,n", [(a, n) for a in oc.ANSATZ_TYPES for n in (21, 22)] + [("hardware_efficient", 24)])
def test_circuit_dense_theta_against_c_port(be, dev, ansatz, n):
    """Fully random angles (every amplitude non-zero) against the oracle's C port, at the bar of the n = 20 test."""
    from oracle import cpu_port as cp
    assert cp.available(), "oracle/_build/libcpu_port.so is missing: run build()"
    L = 1
    th = np.random.default_rng(n + len(ansatz)).uniform(-np.pi, np.pi, oc.num_params(ansatz, n, L))
    want = torch.as_tensor(cp.circuit_probs(ansatz, n, L, th)[0], device=dev)
    q = be.circuit_probs(ansatz, n, L, torch.as_tensor(th, device=dev).reshape(1, -1))[0]
    err = (q - want).abs() - 1e-9 * want.abs()
    assert float(err.max()) <= 1e-17
    assert abs(float(q.sum()) - 1.0) <= 1e-12


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L", [(21, 1), (24, 2), (25, 1), (26, 1)])
def test_circuit_sparse_reg_wires_4(r4, dev, ansatz, n, L):
    """16 amplitudes per thread: fast tables up to n = 25, the generic kernel at n = 26."""
    circuit_case(r4, dev, ansatz, n, L, seed=7000 + 1000 * n + 10 * L + len(ansatz))


def test_n30_is_refused_before_any_launch(be, dev):
    from tensornetworks_amd._ext import BornviError
    n = 30
    th = torch.zeros(oc.num_params("basic", n, 1), dtype=torch.float64, device=dev)
    one = torch.zeros(1, dtype=torch.float64, device=dev)
    calls = [lambda: be.circuit_probs("basic", n, 1, th.reshape(1, -1)),
             lambda: be.paramshift_probs("basic", n, 1, th, 0, 1),
             lambda: be.paramshift_grad("basic", n, 1, th, one, 0, 1),
             lambda: be.paramshift_dot_begin("basic", n, 1, th, 0, 1),
             lambda: be.adjoint_state("basic", n, 1, th),
             lambda: be.stein_matvec_kron(one, one, n)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    for f in calls:
        with pytest.raises(BornviError, match="out of range"):
            f()
    assert torch.cuda.memory_allocated(dev) == before


# ---- parameter shift ----------------------------------------------------------------------------------------------
def pick_params(ansatz, n, L, th, generic, rng, count):
    """An arithmetic progression of `count` parameters (p_begin, p_end, p_stride) through the first generic one; every
    other member that is an RX / RY is made generic too, the rest stay monomial (RZ always is)."""
    kinds = sc.param_kinds(ansatz, n, L)
    P = th.size
    stride = max(1, P // count - 1)
    p0 = generic[0] % stride
    ps = list(range(p0, P, stride))[:count]
    for p in ps[1::2]:
        if kinds[p][0] in ("RX", "RY") and p not in generic:
            th[p] = rng.uniform(0.0, 2.0 * np.pi)
            generic.append(p)
    assert any(p in generic for p in ps) and any(p not in generic for p in ps)
    return ps, p0, ps[-1] + 1, stride


def shift_reference(ansatz, n, L, th, ps, w):
    """1/2 sum_z w_z (q+ - q-) per parameter from the sparse oracle (w gathered at both supports); and its scale."""
    ref, scale, rows = [], [], []
    for (ip, qp), (im, qm) in sc.paramshift_sparse(ansatz, n, L, th, ps):
        wp = w[torch.as_tensor(ip, device=w.device)].cpu().numpy()
        wm = w[torch.as_tensor(im, device=w.device)].cpu().numpy()
        ref.append(0.5 * (wp @ qp - wm @ qm))
        scale.append(0.5 * (np.abs(wp) @ qp + np.abs(wm) @ qm))
        rows.append(((ip, qp), (im, qm)))
    return np.array(ref), np.array(scale), rows


def device_weights(dev, n, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(1 << n, generator=g, dtype=torch.float64, device=dev)


@pytest.mark.parametrize("n,count", [(22, 6), (26, 6), (27, 2)])
def test_paramshift_grad_sparse(be, dev, monkeypatch, n, count):
    ansatz, L = "hardware_efficient", 2
    th, generic, rng = sparse_case(ansatz, n, L, seed=50 + n)
    ps, p0, p1, stride = pick_params(ansatz, n, L, th, generic, rng, count)
    w = device_weights(dev, n, n)
    if n >= 27:
        # chunks of two circuits: the library's chunked batch at this size too
        h = be._ext.handle_for(dev)
        monkeypatch.setattr(be, "WORKSPACE_CAP", h.size("bornvi_circuit_workspace_bytes", be.ansatz_id(ansatz), n, L, 2))
    grad = be.paramshift_grad(ansatz, n, L, torch.as_tensor(th, device=dev), w, p0, p1, stride).cpu().numpy()
    ref, scale, _ = shift_reference(ansatz, n, L, th, ps, w)
    assert grad.shape == ref.shape
    assert np.all(np.abs(grad - ref) <= 1e-12 * scale), (grad, ref)


@pytest.mark.parametrize("n,count", [(22, 6), (27, 2)])
def test_paramshift_dot_sparse(be, dev, n, count):
    ansatz, L = "hardware_efficient", 2
    th, generic, rng = sparse_case(ansatz, n, L, seed=80 + n)
    ps, p0, p1, stride = pick_params(ansatz, n, L, th, generic, rng, count)
    assert be.paramshift_dot_supported(ansatz, n, L, dev, len(ps))
    w = device_weights(dev, n, 3 * n)
    q, token = be.paramshift_dot_begin(ansatz, n, L, torch.as_tensor(th, device=dev), p0, p1, stride)
    _, grad = be.paramshift_dot_finish(token, w)
    ref, scale, _ = shift_reference(ansatz, n, L, th, ps, w)
    assert np.all(np.abs(grad.cpu().numpy() - ref) <= 1e-12 * scale), (grad, ref)
    check_sparse(q, *sc.probs_sparse(ansatz, n, L, th), what=f"dot q n={n}")


def test_fused_dot_respects_the_workspace_cap(be, dev, monkeypatch):
    """A fused-dot workspace above WORKSPACE_CAP sends the trainer down the chunked path, with the same gradient."""
    from tensornetworks_amd.bayesian_network import synthetic_network
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    n, L = 14, 3
    bn, lat, obs, x = synthetic_network(n, seed=4)
    torch.manual_seed(0)
    vi = KSDVariationalInference(bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, pytorch_device=str(dev))
    vi._prepare_stein(x)
    vi.overlap_streams = False
    P = oc.num_params("hardware_efficient", n, L)
    begins = []
    real_begin = be.paramshift_dot_begin
    monkeypatch.setattr(be, "paramshift_dot_begin", lambda *a, **k: begins.append(1) or real_begin(*a, **k))
    assert be.paramshift_dot_supported("hardware_efficient", n, L, dev, P)
    l0, g0, q0 = vi.ksd_and_grad()
    assert len(begins) == 1                      # the fused path ran
    need = int(be._ext.lib().bornvi_paramshift_dot_workspace_bytes(be._ext.handle_for(dev).h, 0, n, L, P))
    monkeypatch.setattr(be, "WORKSPACE_CAP", need - 1)
    assert not be.paramshift_dot_supported("hardware_efficient", n, L, dev, P)
    l1, g1, q1 = vi.ksd_and_grad()
    assert len(begins) == 1                      # ... and now the chunked one
    torch.cuda.synchronize()
    assert float((q0 - q1).abs().max()) <= 1e-12 * float(q0.abs().max())
    scale = float(g0.abs().max())
    assert float((g0 - g1).abs().max()) <= 1e-12 * scale
    assert abs(float(l0) - float(l1)) <= 1e-12 * abs(float(l0))


# ---- adjoint engine -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ansatz,n", [("hardware_efficient", 24), ("basic", 24), ("hardware_efficient", 29)])
def test_adjoint_state_sparse(be, dev, ansatz, n):
    L = 2
    th, _, _ = sparse_case(ansatz, n, L, seed=300 + n)
    state, probs = be.adjoint_state(ansatz, n, L, torch.as_tensor(th, device=dev))
    idx, amp = sc.state_sparse(ansatz, n, L, th)
    got = state[torch.as_tensor(idx, device=dev)].cpu().numpy()
    assert np.abs(got - amp).max() <= 1e-12 * np.abs(amp).max()
    p = amp.real ** 2 + amp.imag ** 2
    check_sparse(probs, idx, p, f"adjoint probs n={n}")
    del probs
    be.release_workspaces()             # (n = 29: 32 GiB of workspace and 4 GiB of probabilities go before |state|^2)
    torch.cuda.empty_cache()
    check_sparse(state.abs().square_(), idx, p, f"adjoint |state|^2 n={n}")


def test_adjoint_vjp_sparse(be, dev):
    ansatz, n, L = "hardware_efficient", 24, 2
    th, generic, rng = sparse_case(ansatz, n, L, seed=400)
    ps, _, _, _ = pick_params(ansatz, n, L, th, generic, rng, 6)
    tht = torch.as_tensor(th, device=dev)
    state, _ = be.adjoint_state(ansatz, n, L, tht, want_probs=False)
    w = device_weights(dev, n, 401)
    grad = be.adjoint_vjp(ansatz, n, L, tht, state, w).cpu().numpy()
    ref, scale, _ = shift_reference(ansatz, n, L, th, ps, w)
    assert np.all(np.abs(grad[ps] - ref) <= 1e-12 * scale), (grad[ps], ref)


# ---- matrix-free Stein mat-vec ----------------------------------------------------------------------------------------
def kp_block(zi, zj, Si, Sj, n, length_scale=1.0):
    """k_p(z_i, z_j) for every pair of the index lists (closed form of oracle.stein.gram_closed_form)."""
    a = math.exp(-1.0 / (n * length_scale))
    x = zi[:, None] ^ zj[None, :]
    bits = ((x[:, :, None] >> (n - 1 - np.arange(n))[None, None, :]) & 1).astype(np.float64)
    c = np.where(bits > 0, 1.0 - 1.0 / a, 1.0 - a)
    T = Si[:, None, :] * Sj[None, :, :] - c * (Si[:, None, :] + Sj[None, :, :]) + 2.0 * c
    return (a ** bits.sum(-1)) * T.sum(-1)


def bits_of(z, n):
    return tuple(int(b) for b in format(int(z), f"0{n}b"))


@pytest.mark.parametrize("n", [21, 24])
def test_stein_matvec_kron_sparse_q(be, dev, n):
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    S = torch.randn((1 << n, n), generator=g, dtype=torch.float64, device=dev)
    th, _, rng = sparse_case("hardware_efficient", n, 2, seed=500 + n)
    idx, p = sc.probs_sparse("hardware_efficient", n, 2, th)
    q = torch.zeros(1 << n, dtype=torch.float64, device=dev)
    q[torch.as_tensor(idx, device=dev)] = torch.as_tensor(p, device=dev)
    ksd2, y = be.stein_matvec_kron(S, q, n)
    blocks = np.arange(0, 1 << n, 1 << 13, dtype=np.int64)
    blocks = blocks[np.linspace(0, blocks.size - 1, min(blocks.size, 512)).astype(np.int64)]
    rows = np.unique(np.concatenate([idx, blocks, blocks + (1 << 13) - 1, rng.integers(0, 1 << n, 4096 - 2 * blocks.size - idx.size)]))
    Sr = S[torch.as_tensor(rows, device=dev)].cpu().numpy()
    Ss = S[torch.as_tensor(idx, device=dev)].cpu().numpy()
    K = kp_block(rows, idx, Sr, Ss, n)
    # the closed form against the term-by-term restatement of the reference, on a few pairs
    for i, j in [(0, 0), (1, 3), (rows.size - 1, idx.size - 1), (rows.size // 2, idx.size // 2)]:
        kv = os_.stein_kernel_value(bits_of(rows[i], n), bits_of(idx[j], n), Sr[i], Ss[j], n)
        assert abs(K[i, j] - kv) <= 1e-12 * max(1.0, abs(kv))
    y_ref = K @ p
    y_scale = np.abs(K) @ p
    got = y[torch.as_tensor(rows, device=dev)].cpu().numpy()
    assert np.all(np.abs(got - y_ref) <= 1e-12 * y_scale), float((np.abs(got - y_ref) / y_scale).max())
    Kss = kp_block(idx, idx, Ss, Ss, n)
    k_ref = float(p @ Kss @ p)
    assert abs(float(ksd2) - k_ref) <= 1e-12 * float(p @ np.abs(Kss) @ p), (float(ksd2), k_ref)


# ---- score from CPTs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [22, 26])
def test_score_from_cpts(be, dev, n):
    """64-bit outcome index and the per-outcome CPT walk at sizes the goldens never reach."""
    from tensornetworks_amd.bayesian_network import synthetic_network, pack_network
    bn, lat, obs, x = synthetic_network(n, 0)
    S, pxz = be.score_from_packed(pack_network(bn, lat, x), n, dev)
    rng = np.random.default_rng(n)
    rows = np.unique(np.concatenate([[0, (1 << n) - 1], rng.integers(0, 1 << n, 510)]))
    rt = torch.as_tensor(rows, device=dev)
    Sg, pg = S[rt].cpu().numpy(), pxz[rt].cpu().numpy()
    for r, z in enumerate(rows):
        zb = bits_of(z, n)
        s_ref = os_.score_for_z(bn, x, zb, lat, obs)
        p_ref = os_.compute_prob_joint_xz(bn, x, zb, lat, obs)
        assert abs(pg[r] - p_ref) <= 1e-14 * p_ref, (z, pg[r], p_ref)
        assert np.all(np.abs(Sg[r] - s_ref) <= 1e-14 * np.maximum(1.0, np.abs(s_ref))), (z, Sg[r], s_ref)


# ---- classical table kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [24, 26])
@pytest.mark.parametrize("mode", [0, 1])
def test_born_table_large_n(be, dev, n, mode):
    """One row of 2^n against float64 CPU autograd (test_gpu_classical.reference_terms), at that file's tolerances."""
    from test_gpu_classical import reference_terms
    gen = torch.Generator().manual_seed(n + 100 * mode)
    w = (torch.randn(1, 1 << n, generator=gen) * 2.0).to(dev)
    y = torch.randn(1, 1 << n, generator=gen, dtype=torch.float64).to(dev)
    ksd2 = torch.tensor([2.5], dtype=torch.float64, device=dev)
    lam = 0.013
    q32, q64, H = be.born_table_probs(w, mode)
    assert torch.equal(q64, q32.double())
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    g = be.born_table_vjp(w, q64, mode, y=y, ksd2=ksd2, entropy_weight=lam, loss_out=loss)
    q_ref, H_ref, g_ref, loss_ref = (t.to(dev) for t in reference_terms(w, mode, y, ksd2, lam))
    torch.testing.assert_close(q32.double(), q_ref, rtol=2e-7, atol=1e-12)
    torch.testing.assert_close(H.double(), H_ref, rtol=2e-6, atol=1e-6)
    torch.testing.assert_close(loss, loss_ref, rtol=1e-15, atol=0)
    scale = g_ref.abs().amax(dim=-1, keepdim=True).clamp(min=lam)
    assert float(((g.double() - g_ref).abs() / scale).max()) < 1e-5


# ---- sampler ----------------------------------------------------------------------------------------------------------
def test_shots_histogram_sparse_q_n26(be, dev):
    n, shots = 26, 1 << 20
    th, _, _ = sparse_case("basic", n, 2, seed=600)
    idx, p = sc.probs_sparse("basic", n, 2, th)
    q = torch.zeros(1, 1 << n, dtype=torch.float64, device=dev)
    it = torch.as_tensor(idx, device=dev)
    q[0, it] = torch.as_tensor(p, device=dev)
    epoch = torch.zeros(1, dtype=torch.int64, device=dev)
    f = be.shots_histogram(q, n, shots, 1234, epoch)[0]
    counts = f * shots
    assert float((counts - counts.round()).abs().max()) <= 1e-6
    on = counts[it].cpu().numpy()
    assert int(round(on.sum())) == shots
    counts[it] = 0.0
    assert float(counts.abs().max()) == 0.0
    # the sampled frequencies follow p (a loose 6-sigma bound per outcome)
    sigma = np.sqrt(p * (1 - p) / shots)
    assert np.all(np.abs(on / shots - p) <= 6 * sigma + 1e-12)
