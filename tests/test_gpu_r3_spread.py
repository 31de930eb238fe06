"""circuit_pass_r3_kernel<false, true> spreads the next tile's eight loads over the first LDS stages of a trip: the stages
are peeled out of the run-time stage loop (none, one or two of them, by the pass's stage count; the last stage of a pass is
never peeled) and the loads go out in one, two or three groups between them.  The launcher sends a pass there when it has
more than three slots to load and a stage to peel; every other pass, and the fused dot, runs the instantiation with the
single burst.  These tests walk every such shape through the
C ABI against the NumPy oracle (tolerance of test_gpu_r3.py::test_r3_probs_match_oracle) and the fused dot against the
un-fused gradient (1e-12, as test_fused_dot_equals_stored_probabilities), with persistent grids that run several trips
with a partial last one, and grids of exactly one trip.  The plan words are read here and the coverage is asserted, so a
planner change cannot empty a case silently."""
import functools

import numpy as np
import pytest
import torch

from oracle import circuit as oc

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-14

# (ansatz, n, L, tile_bits) with the read map on; stage counts and CH_DIRECT per pass as test_the_cases_cover_every_shape reads them:
CASES = [("all_to_all", 12, 2, 9),            # stages 3 4 1; zero slots in pass 1; last pass: one stage, straight from HBM, drain
         ("all_to_all", 13, 2, 9),            # stages 3 5 2; last pass: two stages, no peel
         ("hardware_efficient", 13, 3, 11),   # stages 6 6 3; pass 1 direct on both sides, zero slots; last pass by fill and drain
         ("hardware_efficient", 14, 3, 11),   # stages 6 6 4; last pass: direct first stage, two peeled, one in the loop, drain
         ("hardware_efficient", 12, 4, 9),    # stages 5 5 4 2 3; a two-stage pass direct on both sides
         ("basic", 14, 3, 11)]                # stages 7 5 3; last pass: direct first stage, ONE peeled stage, drain
DOT_CASES = [("all_to_all", 14, 3, 11),       # last pass: a single stage
             ("hardware_efficient", 14, 3, 11)]   # last pass: four stages
CH_NSTAGES, CH_DIRECT, CH_ZINFO = 0, 5, 6     # plan.hpp: CompactHeader


def pass_shapes(ansatz, n, L, kb):
    """[(stages, direct first stage, direct last stage, slots not loaded)] per pass, as the kernel derives them."""
    from tensornetworks_amd import _ext
    Cw, offs = _ext.plan_compact_words(_ext.ANSATZ_IDS[ansatz], n, L, kb | 0x100)
    assert Cw is not None, (ansatz, n, L, kb)
    out = []
    for i, o in enumerate(offs):
        ns, d = int(Cw[o + CH_NSTAGES]), int(Cw[o + CH_DIRECT])
        din = bool(d & 1) and i > 0 and ns > 0
        out.append((ns, din, bool(d & 2) and ns > 1, (int(Cw[o + CH_ZINFO]) & 0xff) if din else 0))
    return out


def peeled(ns, din):
    """Stages peeled in a pass that loads every slot, from its stage count and direct first stage alone.  This restates
    `spare` / `npeel` of circuit_pass_r3_kernel (kernels_circuit8.hip, "the next tile's eight loads are spread ..."): if that
    rule changes, change this with it -- the assertions below say which shapes the cases reach, the parity tests do not use it."""
    return max(0, min(2, ns - (1 if din else 0) - 1))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture()
def be(dev):
    from tensornetworks_amd import backend
    # (in this order on the way back: setting tile_bits also sets tile_bits_multi)
    keep = {k: backend.get_option(dev, k) for k in ("tile_bits", "tile_bits_multi", "fast_workgroups_per_cu", "reg_wires", "read_map",
                                                    "zero_support", "direct_stages")}
    backend.set_option(dev, "reg_wires", 3)
    backend.set_option(dev, "read_map", 1)
    yield backend
    for k, v in keep.items():
        backend.set_option(dev, k, v)


@pytest.fixture(scope="module")
def cus(dev):
    """Workgroups of the persistent grid with one workgroup per CU."""
    n = torch.cuda.get_device_properties(dev).multi_processor_count
    assert n % 16 == 0, n       # (a multiple of the 4, 8 or 16 tiles per circuit of the cases)
    return n


@functools.lru_cache(maxsize=None)
def two_rows(ansatz, n, L):
    """Two parameter vectors and the oracle's rows for them (computed once, read-only)."""
    th = np.random.default_rng(31 * n + L).uniform(-np.pi, np.pi, (2, oc.num_params(ansatz, n, L)))
    ref = np.stack([oc.probs(ansatz, n, L, th[0]), oc.probs(ansatz, n, L, th[1])])
    th.setflags(write=False)
    ref.setflags(write=False)
    return th, ref


def test_the_cases_cover_every_shape():
    shapes = [s for c in CASES for s in pass_shapes(*c)]
    counts = {ns for ns, _, _, _ in shapes}
    assert {1, 2, 3} <= counts and max(counts) >= 4, counts
    loading = [(ns, din) for c in CASES for ns, din, _, _ in pass_shapes(*c)[1:]]      # (with zero_support = 0 every slot is loaded)
    assert {peeled(ns, din) for ns, din in loading} == {0, 1, 2}                      # one, two and three load groups
    assert any(ns - (1 if din else 0) - peeled(ns, din) > 1 for ns, din in loading)   # peeled stages and a stage loop behind them
    assert any(dout for _, _, dout, _ in shapes) and any(not dout for _, _, dout, _ in shapes)     # direct last stage and drain
    assert any(din for _, din, _, _ in shapes) and any(not din and i for c in CASES for i, (_, din, _, _) in enumerate(pass_shapes(*c)))
    for c in CASES[:1] + CASES[2:3]:          # a pass that leaves slots out needs three passes
        sh = pass_shapes(*c)
        assert len(sh) >= 3 and sh[1][3] not in (0, 0xff) and peeled(sh[1][0], sh[1][1]) == 2, sh     # (three groups with zero_support = 0)
    for c in CASES:                           # whole waves, and a persistent grid of 256 is a multiple of the tiles per circuit
        assert c[3] >= 9 and 2 <= c[1] - c[3] <= 4
    assert pass_shapes(*DOT_CASES[0])[-1][0] == 1 and pass_shapes(*DOT_CASES[1])[-1][0] >= 4


@pytest.mark.parametrize("zero_support", [1, 0])
@pytest.mark.parametrize("trips", ["partial_last_trip", "one_trip"])
@pytest.mark.parametrize("ansatz,n,L,kb", CASES)
def test_spread_loads_match_oracle(be, dev, cus, ansatz, n, L, kb, trips, zero_support):
    """One persistent workgroup per CU (256 on an MI355X) for 100 circuits of 4, 8 or 16 tiles: 1.56, 3.125 or 6.25 trips (the
    last one partial: has_next turns false in different trips of different workgroups), and for exactly as many tiles as
    workgroups: one trip (has_next is false in the first real trip).  Every row must be the oracle's row of its parameters, with the zero slots left out and with every
    slot loaded; twice the same bits."""
    batch = 100 if trips == "partial_last_trip" else cus >> (n - kb)
    tiles = batch << (n - kb)
    assert (tiles > cus and tiles % cus != 0) if trips == "partial_last_trip" else tiles == cus
    be.set_option(dev, "tile_bits", kb)
    be.set_option(dev, "fast_workgroups_per_cu", 1)
    be.set_option(dev, "zero_support", zero_support)
    th2, ref = two_rows(ansatz, n, L)
    pick = np.random.default_rng(batch).integers(0, 2, batch)
    t = torch.as_tensor(th2[pick], dtype=torch.float64, device=dev).contiguous()
    q = be.circuit_probs(ansatz, n, L, t).cpu().numpy()
    q2 = be.circuit_probs(ansatz, n, L, t).cpu().numpy()
    np.testing.assert_allclose(q, ref[pick], rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(q, q2)


@pytest.mark.parametrize("ansatz,n,L,kb", [CASES[2], CASES[5]])
def test_spread_loads_without_direct_stages(be, dev, ansatz, n, L, kb):
    """The same plans by tile fill and drain only: the first LDS stage is stage 0, so one more stage is peeled."""
    be.set_option(dev, "tile_bits", kb)
    be.set_option(dev, "fast_workgroups_per_cu", 1)
    be.set_option(dev, "direct_stages", 0)
    th2, ref = two_rows(ansatz, n, L)
    pick = np.random.default_rng(7).integers(0, 2, 100)
    t = torch.as_tensor(th2[pick], dtype=torch.float64, device=dev).contiguous()
    q = be.circuit_probs(ansatz, n, L, t).cpu().numpy()
    np.testing.assert_allclose(q, ref[pick], rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(q, be.circuit_probs(ansatz, n, L, t).cpu().numpy())


@pytest.mark.parametrize("wgs", [1, 0], ids=["several_trips", "default_grid"])
@pytest.mark.parametrize("ansatz,n,L,kb", DOT_CASES)
def test_spread_loads_in_the_fused_dot(be, dev, ansatz, n, L, kb, wgs):
    """The DOT instantiation (always the single burst) with one stage in the last pass and with four, behind passes that spread
    their loads: q and loss
    bitwise, gradient to 1e-12 of its largest entry against the un-fused path; twice the same bits."""
    be.set_option(dev, "tile_bits", kb)
    be.set_option(dev, "fast_workgroups_per_cu", wgs)
    P = oc.num_params(ansatz, n, L)
    rng = np.random.default_rng(n + L)
    th = torch.as_tensor(rng.uniform(-np.pi, np.pi, P), device=dev)
    w = torch.as_tensor(rng.standard_normal(1 << n), device=dev)
    ksd2 = torch.tensor([3.7], dtype=torch.float64, device=dev)
    assert be.paramshift_dot_supported(ansatz, n, L, dev, P)
    probs = be.paramshift_probs(ansatz, n, L, th, 0, P, include_base=True).clone()
    loss_u, grad_u, _ = be.ksd_grad_finish(n, probs[1:], P, w, ksd2)
    q, tok = be.paramshift_dot_begin(ansatz, n, L, th, 0, P)
    loss_f, grad_f = be.paramshift_dot_finish(tok, w, ksd2)
    assert torch.equal(q, probs[0]) and torch.equal(loss_f, loss_u)
    assert float((grad_f - grad_u).abs().max()) <= 1e-12 * float(grad_u.abs().max())
    q2, tok2 = be.paramshift_dot_begin(ansatz, n, L, th, 0, P)
    loss_2, grad_2 = be.paramshift_dot_finish(tok2, w, ksd2)
    assert torch.equal(grad_2, grad_f) and torch.equal(q2, q)
    be.release_workspaces()
