"""bornvi_paramshift_states: the phase-coherent statevectors of the base and the pi-shifted circuits out of the batched
engine, against oracle.circuit.simulate (n <= 10) and bornvi_adjoint_state (above), for every ansatz, under both values of
reg_wires, at n = 1, 2, 3, at the sizes where the planner's describe calls report the first multi-pass plan of either
pass kernel, and with small tiles that force several passes at a size the oracle covers.

Tolerance: 64 eps (number of gates) per amplitude, absolute, eps = 2^-52 (|amplitude| <= 1: a gate's 2 x 2 complex product
errs by a few eps of the pair's magnitude, and the errors of successive gates add).  A flat absolute tolerance: amplitudes
far below it are not checked here; the per-entry bound (envelope and 2-norm arms) is test_gpu_circuit_precision.py's."""
import numpy as np
import pytest
import torch

from oracle import circuit as oc

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(params=[3, 4], ids=["r3", "r4"])
def be(dev, request):
    from tensornetworks_amd import backend
    default_r = backend.get_option(dev, "reg_wires")
    backend.set_option(dev, "reg_wires", request.param)
    yield backend
    backend.set_option(dev, "tile_bits", 13)
    backend.set_option(dev, "reg_wires", default_r)


def first_multi_pass_sizes(L=2):
    """Smallest n whose default plan has more than one pass, per pass kernel (8 and 16 amplitudes per thread), and the size
    below it (the largest one-pass plan), read off the planner (no GPU needed)."""
    from tensornetworks_amd import _ext
    sizes = set()
    for flag in (_ext.R3, 0):
        for n in range(1, 20):
            if int(_ext.plan_words(_ext.ANSATZ_IDS["hardware_efficient"], n, L, flag)[3]) > 1:
                sizes.update((n - 1, n))
                break
    return sorted(sizes)


def tol(ansatz, n, L):
    return 64 * EPS * len(oc.gate_list(ansatz, n, L))


def reference_rows(be, dev, ansatz, n, L, theta, params, include_base):
    rows = []
    for p in ([None] if include_base else []) + list(params):
        t = theta.copy()
        if p is not None:
            t[p] += np.pi
        if n <= 10:
            rows.append(oc.simulate(oc.gate_list(ansatz, n, L), n, t))
        else:
            rows.append(be.adjoint_state(ansatz, n, L, torch.from_numpy(t).to(dev), want_probs=False)[0].cpu().numpy())
    return np.array(rows)


def check(be, dev, ansatz, n, L, p_begin=0, p_end=None, include_base=True, seed=0):
    P = oc.num_params(ansatz, n, L)
    p_end = P if p_end is None else p_end
    theta = np.random.default_rng([n, L, seed]).uniform(-np.pi, np.pi, P)
    th = torch.from_numpy(theta).to(dev)
    before = be.paramshift_probs(ansatz, n, L, th, 0, min(P, 3), include_base=True).clone()
    got = be.paramshift_states(ansatz, n, L, th, p_begin, p_end, include_base=include_base)
    assert got.shape == ((1 if include_base else 0) + p_end - p_begin, 1 << n) and got.dtype == torch.complex128
    ref = reference_rows(be, dev, ansatz, n, L, theta, range(p_begin, p_end), include_base)
    err = float(np.abs(got.cpu().numpy() - ref).max()) if ref.size else 0.0
    print(f"{ansatz} n={n} L={L} [{p_begin}, {p_end}) base={include_base}: max |row - ref| {err:.3e} (tolerance {tol(ansatz, n, L):.3e})")
    assert err <= tol(ansatz, n, L)
    # |row|^2 is bornvi_circuit_probs at the same parameters
    thetas = np.tile(theta, (got.shape[0], 1))
    for r, p in enumerate(range(p_begin, p_end)):
        thetas[r + (1 if include_base else 0), p] += np.pi
    if got.shape[0]:
        q = be.circuit_probs(ansatz, n, L, torch.from_numpy(thetas).to(dev))
        assert float(((got.real ** 2 + got.imag ** 2) - q).abs().max()) <= tol(ansatz, n, L)
    # and the probability engine is left as it was: the same rows, bit for bit
    assert torch.equal(before, be.paramshift_probs(ansatz, n, L, th, 0, min(P, 3), include_base=True))
    return got


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L", [(1, 1), (2, 2), (3, 4), (5, 3), (10, 2)])
def test_small_states_match_the_oracle(be, dev, ansatz, n, L):
    check(be, dev, ansatz, n, L)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb", [(6, 3, 4), (9, 2, 6), (10, 2, 7)])
def test_several_passes_match_the_oracle(be, dev, ansatz, n, L, kb):
    be.set_option(dev, "tile_bits", kb)
    check(be, dev, ansatz, n, L)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
def test_first_multi_pass_sizes_match_the_adjoint_engine(be, dev, ansatz):
    sizes = first_multi_pass_sizes()
    assert sizes and max(sizes) >= 14, sizes
    for n in sizes:
        P = oc.num_params(ansatz, n, 2)
        check(be, dev, ansatz, n, 2, p_begin=P - 5, p_end=P - 1)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
def test_sub_range_and_base_row(be, dev, ansatz):
    n, L = 5, 2
    full = check(be, dev, ansatz, n, L)
    part = check(be, dev, ansatz, n, L, p_begin=3, p_end=9, include_base=False)
    assert torch.equal(part, full[4:10])
    with_base = check(be, dev, ansatz, n, L, p_begin=3, p_end=9, include_base=True)
    assert torch.equal(with_base[0], full[0]) and torch.equal(with_base[1:], part)
    only_base = be.paramshift_states(ansatz, n, L, torch.zeros(oc.num_params(ansatz, n, L), dtype=torch.float64, device=dev), 2, 2)
    assert only_base.shape == (1, 32)
    with pytest.raises(be.BornviError):
        be.paramshift_states(ansatz, n, L, torch.zeros(oc.num_params(ansatz, n, L), dtype=torch.float64, device=dev), 0, 10 ** 6)


def test_chunked_workspace_gives_the_same_rows(be, dev, monkeypatch):
    n, L, ansatz = 9, 2, "hardware_efficient"
    be.set_option(dev, "tile_bits", 6)
    P = oc.num_params(ansatz, n, L)
    th = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, P)).to(dev)
    full = be.paramshift_states(ansatz, n, L, th, 0, P)
    monkeypatch.setattr(be, "WORKSPACE_CAP", 7 * (2 * 16 << n) + 60000)          # room for about six circuits
    be.release_workspaces()
    assert torch.equal(full, be.paramshift_states(ansatz, n, L, th, 0, P))
    be.release_workspaces()


def test_capture_and_replay(be, dev):
    n, L, ansatz = 6, 2, "all_to_all"
    P = oc.num_params(ansatz, n, L)
    th = torch.from_numpy(np.random.default_rng(8).uniform(-1, 1, P)).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = be.paramshift_states(ansatz, n, L, th, 0, P)           # plan and the side stream's workspace exist
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    eager = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        be.paramshift_states(ansatz, n, L, th, 0, P, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, eager)
