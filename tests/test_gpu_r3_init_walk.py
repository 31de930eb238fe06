"""The INIT pass of circuit_pass_r3_kernel walks only the tiles it writes: the one non-zero tile of every circuit, spread over
all workgroups, then per circuit the zero tiles of the rows g != 0 with (g & mask) == 0, mask = CH_ZINFO of pass 0 (the rows
nobody reads cost no loop trip any more); when the mask covers every row bit the walk ends behind the real tiles, and the
workgroups beyond it leave at once.  These tests run such plans through the C ABI with persistent grids of several trips, of
one trip and with more workgroups than real INIT tiles: every row against the NumPy oracle (tolerance of
test_gpu_r3.py::test_r3_probs_match_oracle), twice the same bits, the same bits with zero_support = 0 (no mask: every zero
tile is written), and the bits the library computed when every tile had a trip (tests/golden/init_walk_rows_parent_bits.npz,
recorded on an MI355X by tests/golden/make_golden_init_walk_rows_bits.py, which also holds the cases and the grids).  The
plan words are read here and the shapes asserted, so a planner change cannot empty a case silently."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import circuit as oc

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-10, 1e-14
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "init_walk_rows_parent_bits.npz")
_spec = importlib.util.spec_from_file_location("make_golden_init_walk_rows_bits", os.path.join(HERE, "golden", "make_golden_init_walk_rows_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.CASES
GRIDS = ("partial_last_trip", "one_trip", "real_trips")
DOT_CASE = ("hardware_efficient", 14, 3, 11)      # 8 tile rows, all masked; three passes, the last one the fused dot
CH_NSTAGES, CH_DIRECT, CH_ZINFO = 0, 5, 6         # plan.hpp: CompactHeader


def pass_words(ansatz, n, L, kb):
    """[(stages, direct first stage, direct last stage, CH_ZINFO)] per pass, as the kernel and the launcher derive them."""
    from tensornetworks_amd import _ext
    Cw, offs = _ext.plan_compact_words(_ext.ANSATZ_IDS[ansatz], n, L, kb | 0x100)
    assert Cw is not None, (ansatz, n, L, kb)
    out = []
    for i, o in enumerate(offs):
        ns, d = int(Cw[o + CH_NSTAGES]), int(Cw[o + CH_DIRECT])
        out.append((ns, bool(d & 1) and i > 0 and ns > 0, bool(d & 2) and ns > 1, int(Cw[o + CH_ZINFO])))
    return out


def written_zero_rows(case, words):
    """Tile rows g != 0 whose zero tiles the INIT pass writes (support of |0..0> on), from CH_ZINFO of pass 0.  This restates
    zs_free of circuit_pass_r3_kernel: the assertions below say which walks the cases reach, the parity tests do not use it."""
    gbits = case[1] - case[3]
    return [g for g in range(1, 1 << gbits) if g & words[0][3] == 0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture()
def be(dev):
    from tensornetworks_amd import backend
    # (in this order on the way back: setting tile_bits also sets tile_bits_multi)
    keep = {k: backend.get_option(dev, k) for k in rec.OPTIONS}
    yield backend
    for k, v in keep.items():
        backend.set_option(dev, k, v)


@pytest.fixture(scope="module")
def cus(dev):
    n = torch.cuda.get_device_properties(dev).multi_processor_count
    assert n % 16 == 0, n       # (a multiple of the 4, 8 or 16 tiles per circuit of the cases)
    return n


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(GOLDEN), "tests/golden/init_walk_rows_parent_bits.npz is missing"
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def oracle_rows(case):
    ansatz, n, L, _ = case
    th = rec.thetas(case)
    ref = np.stack([oc.probs(ansatz, n, L, th[0]), oc.probs(ansatz, n, L, th[1])])
    ref.setflags(write=False)
    return ref


def test_the_cases_cover_every_walk():
    w = [pass_words(*c) for c in CASES]
    # case 0: a row bit outside the mask: the walk goes on into written zero tiles, and their rows are not 1 .. count
    assert written_zero_rows(CASES[0], w[0]) == [8], w[0]
    # cases 1 to 3: every zero tile is left out, the walk ends behind the real tiles; INIT passes of three stages and of six
    for c, ww in zip(CASES[1:], w[1:]):
        assert written_zero_rows(c, ww) == [] and ww[0][3] != 0, ww
    assert {ww[0][0] for ww in w} >= {3, 5, 6}, w
    for c, ww in zip(CASES, w):
        assert len(ww) >= 3 and c[3] >= 9 and 2 <= c[1] - c[3] <= 4       # whole waves; 256 workgroups are a multiple of the tiles per circuit
        assert ww[0][2] and not ww[0][1]                                    # the INIT pass stores from its last stage
    # pass 1 with one slot loaded and with two; direct last stage and drain
    assert {ww[1][3] & 0xff for ww in w} >= {0xfe, 0xee} and all(ww[1][1] for ww in w), w
    wd = pass_words(*DOT_CASE)
    assert len(wd) == 3 and written_zero_rows(DOT_CASE, wd) == [] and wd[0][3] != 0, wd


@pytest.mark.parametrize("zero_support", [1, 0])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", CASES, ids=rec.case_id)
def test_rows_are_the_oracles_and_the_parents(be, dev, cus, golden, case, grid, zero_support):
    """One persistent workgroup per CU.  partial_last_trip: 100 circuits of 4, 8 or 16 tiles, 1.56 to 6.25 trips (has_next
    turns false in different trips of different workgroups; the INIT pass has 100 real tiles for 256 workgroups: the others
    see only zero tiles, or none).  one_trip: as many tiles as workgroups.  real_trips: 600 circuits (an INIT workgroup
    runs two or three real tiles, then zero tiles if any are written)."""
    n, kb = case[1], case[3]
    batch = rec.grids(case, cus)[grid]
    tiles = batch << (n - kb)
    if grid == "one_trip":
        assert tiles == cus
    else:
        assert tiles > cus and tiles % cus != 0 and (batch < cus) == (grid == "partial_last_trip")
    pick, q = rec.rows_of(case, batch, zero_support)          # (asserts: two calls equal; a row does not depend on its place)
    np.testing.assert_allclose(q, oracle_rows(case)[pick], rtol=RTOL, atol=ATOL)
    assert np.array_equal(rec.row_bytes(q[:2]), golden[rec.case_id(case)]), "rows differ from the recorded parent bits"


def test_fused_dot_behind_the_short_walk(be, dev):
    """The fused dot against the un-fused gradient (1e-12 of its largest entry), q and loss bitwise, twice the same bits:
    the INIT pass in front of the DOT pass ends its walk behind the real tiles."""
    ansatz, n, L, kb = DOT_CASE
    be.set_option(dev, "reg_wires", 3)
    be.set_option(dev, "read_map", 1)
    be.set_option(dev, "tile_bits", kb)
    be.set_option(dev, "fast_workgroups_per_cu", 1)
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
