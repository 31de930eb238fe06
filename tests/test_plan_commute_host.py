"""The planner's commutation rule (csrc/plan.cpp: an op that stays behind blocks a wire diagonally where it acts as Z there,
and a later op that is diagonal on that wire passes it), on the host:

  * the op order a plan executes is recovered from its words -- the CNOT blocks from the GF(2) maps they were folded into --
    and every pair executed out of program order must commute as dense matrices;
  * the plans, run by tests/plan_emulator.py as the kernels run them, reproduce the oracle (tolerance of the emulator tests
    of test_host_logic.py: 1e-13 absolute);
  * no plan has more passes or more LDS stages than the planner gave before the rule (tests/golden/plan_shapes_parent.npz,
    recorded by tests/golden/make_golden_plan_shapes.py), and the two benchmark plans are pinned;
  * the circuits whose device results are recorded bit for bit plan word for word as they did.

The rule is taken where the library chooses the tile size itself (make_plan_impl): with a tile forced through `tile_bits` the
planner keeps the program-order plan, whose shapes the GPU tests of the pass kernels are built on.  So the small circuits
with forced tiles below run the scans with every block full (reorderings over disjoint wires only), and the rule itself is
reached through the default tile: single-tile plans up to n = 13, 2^13 tiles from n = 14 on (DEFAULT_TILE)."""
import functools
import itertools
import sys

import numpy as np
import pytest

from oracle import circuit as oc
import plan_emulator as pe
from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import make_golden_plan_shapes as shapes      # noqa: E402  (the fixture's layout and its reader of the stage counts)

R3, READ_MAP = 0x200, 0x100
SMALL = [(a, n, L) for a in oc.ANSATZ_TYPES for n in range(3, 7) for L in range(1, 4)]
MEDIUM = [(a, n, L, kb) for a in oc.ANSATZ_TYPES for n, L, kb in ((9, 2, 6), (9, 3, 7), (10, 2, 7), (10, 3, 8), (10, 2, 6))]
DEFAULT_TILE = ([(a, n, L) for a in oc.ANSATZ_TYPES for n, L in ((14, 2), (14, 3))]
                + [("hardware_efficient", 15, 2), ("hardware_efficient", 16, 6), ("hardware_efficient", 13, 6), ("hardware_efficient", 6, 3)])
ATOL = 1e-13


def words(ansatz, n, L, flags):
    from tensornetworks_amd import _ext
    return _ext.plan_words(_ext.ANSATZ_IDS[ansatz], n, L, flags)


@functools.lru_cache(maxsize=None)
def small_tiles(ansatz, n, L, flags):
    """Tile sizes (bits) at which this circuit plans in 2 to 4 passes."""
    return tuple(kb for kb in range(2, n) if 2 <= int(words(ansatz, n, L, kb | flags)[pe.PH_NPASSES]) <= 4)


# ------------------------------------------------------------------------------------------------ the executed order
def program_ops(ansatz, n, L, W):
    """The planner's ops in program order, restated from the gate list: ("U", wire, fused index) -- consecutive one-qubit
    gates of a wire, at most four, up to the next two-qubit gate on it --, ("CX", control, target), ("CZ", a, b); what
    follows the last U is not executed (phases; CNOTs applied to the outcome index) and is left out."""
    ops, open_, count, nf = [], {}, {}, 0
    for kind, wires, _ in oc.gate_list(ansatz, n, L):
        if len(wires) == 1:
            w = wires[0]
            if open_.get(w) is None or count[open_[w]] >= 4:
                open_[w] = nf
                count[nf] = 0
                ops.append(("U", w, nf))
                nf += 1
            count[open_[w]] += 1
        else:
            open_[wires[0]] = open_[wires[1]] = None
            ops.append(("CX" if kind == "CNOT" else "CZ", wires[0], wires[1]))
    assert nf == int(W[pe.PH_NFUSED])
    off = int(W[pe.PH_OFF_FUSED])
    assert all(int(W[off + 10 * f]) == w for k_, w, f in ops if k_ == "U")
    while ops and ops[-1][0] != "U":
        ops.pop()
    return ops


def gf2_inverse(rows, nbits):
    a = [r | (1 << (nbits + i)) for i, r in enumerate(rows)]
    for c in range(nbits):
        p = next(i for i in range(c, nbits) if a[i] >> c & 1)
        a[c], a[p] = a[p], a[c]
        for i in range(nbits):
            if i != c and a[i] >> c & 1:
                a[i] ^= a[c]
    return [r >> nbits for r in a]


def to_wires(rows_by_pos, wire_of):
    """A GF(2) map given as {extended position: mask over extended positions} -> rows over wires (identity elsewhere)."""
    n = len(wire_of)
    out = [1 << w for w in range(n)]
    for p, mask in rows_by_pos.items():
        out[wire_of[p]] = sum(1 << wire_of[q] for q in range(n) if mask >> q & 1)
    return out


def executed_blocks(W):
    """[("CX", rows over wires) | ("CZ", [(a, b), ...]) | ("U", [fused index, ...])] in the order the kernels apply them."""
    n, k, npass = int(W[pe.PH_N]), int(W[pe.PH_K]), int(W[pe.PH_NPASSES])
    off_fused = int(W[pe.PH_OFF_FUSED])
    swz = lambda v: int(pe.swz(np.int64(v)))               # (its own inverse)
    blocks = []
    for i in range(npass):
        P = W[int(W[int(W[pe.PH_OFF_PASSTAB]) + i]):]
        wire_of = [int(P[pe.PW_WIRE_OF_LDS + j]) for j in range(k)] + [int(P[pe.PW_WIRE_OF_G + m]) for m in range(n - k)]
        ldspos = {w: j for j, w in enumerate(wire_of[:k])}
        # CNOTs at the head of the pass, folded into the tile load: slot bit b = parity(row b & (u | g << k))
        cols = [swz(pe.thalf(P, pe.PW_IN_MASK, j)) for j in range(k)] + [swz(pe.thalf(P, pe.PW_IN_GMASK, m)) for m in range(n - k)]
        lead = {b: sum(((cols[j] >> b) & 1) << j for j in range(n)) for b in range(k)}
        blocks.append(("CX", to_wires(lead, wire_of)))
        S = P[pe.PW_STAGES:]
        for _ in range(int(P[pe.PW_NSTAGES])):
            hdr = int(S[0]); r = hdr & 0xFF; sflags = (hdr >> 8) & 0xFF; nwords = hdr >> 16
            rpos = [(int(S[1]) >> (8 * t)) & 0xFF for t in range(r)]
            loff = [swz(int(S[16 + (1 << t)])) for t in range(r)]
            soff = [swz(int(S[32 + (1 << t)])) for t in range(r)]
            inv_read = {}                                  # source bit of position p: the read map's inverse
            for p in range(k):
                ext = int(S[8 + rpos.index(p)]) if p in rpos else int(S[48 + p]) ^ (1 << p)
                inv_read[p] = ext | sum(((loff[t] >> p) & 1) << rpos[t] for t in range(r))
            full = [inv_read[p] for p in range(k)] + [1 << q for q in range(k, n)]
            read = gf2_inverse(full, n)
            blocks.append(("CX", to_wires({p: read[p] for p in range(k)}, wire_of)))
            q_off = pe.STAGE_HDR_WORDS

            def czs(Q):
                return [(wire_of[a], wire_of[b]) for a in range(n) for b in range(n) if int(Q[a]) >> b & 1]
            if sflags & pe.STAGE_SIGN_PRE:
                blocks.append(("CZ", czs(S[q_off: q_off + pe.SIGNQ_WORDS])))
                q_off += pe.SIGNQ_WORDS
            fi = [int(S[6]) & 0xFFFF, int(S[6]) >> 16, int(S[7]) & 0xFFFF, int(S[7]) >> 16]
            us = [f for f in fi if f != 0xFFFF]
            for t, f in enumerate(fi):
                assert f == 0xFFFF or (t < r and int(W[off_fused + 10 * f]) == wire_of[rpos[t]])
            blocks.append(("U", us))
            write = {rpos[t]: int(S[12 + t]) | sum(((soff[t2] >> rpos[t]) & 1) << rpos[t2] for t2 in range(r)) for t in range(r)}
            blocks.append(("CX", to_wires(write, wire_of)))
            if sflags & pe.STAGE_SIGN_POST:
                blocks.append(("CZ", czs(S[q_off: q_off + pe.SIGNQ_WORDS])))
            S = S[nwords:]
        # CNOTs at the tail, folded into the tile store: the out enumeration lists the wires that are low in the buffer
        # written (the next pass's first LDS positions; canonical in the last pass) first, then the other positions
        lo_out = int(P[pe.PW_LO_OUT])
        if i + 1 < npass:
            Pn = W[int(W[int(W[pe.PH_OFF_PASSTAB]) + i + 1]):]
            out_low = [int(Pn[pe.PW_WIRE_OF_LDS + j]) for j in range(lo_out)]
        else:
            out_low = [n - 1 - p for p in range(lo_out)]
        qs = [ldspos[w] for w in out_low] + [q for q in range(k) if wire_of[q] not in out_low]
        ocols = {qs[j]: swz(pe.thalf(P, pe.PW_OUT_MASK, j)) for j in range(k)}
        ocols.update({k + m: swz(pe.thalf(P, pe.PW_OUT_GMASK, m)) for m in range(n - k)})
        inv_tail = [sum(((ocols[q] >> b) & 1) << q for q in range(n)) for b in range(k)] + [1 << q for q in range(k, n)]
        tail = gf2_inverse(inv_tail, n)
        blocks.append(("CX", to_wires({p: tail[p] for p in range(k)}, wire_of)))
    return blocks


def cx_members(pending, ops, M, n):
    """The pending CNOTs, in program order, whose product is the map M (rows over wires); None if there is no such set."""
    ident = [1 << w for w in range(n)]
    cand, seen = [], set()              # the earliest pending copy of each CNOT: a fused U separates two copies, so a block holds one at most
    for i in pending:
        if ops[i][0] == "CX" and M[ops[i][2]] != ident[ops[i][2]] and ops[i] not in seen:
            seen.add(ops[i])
            cand.append(i)
    later_targets = [set(ops[i][2] for i in cand[j:]) for j in range(len(cand) + 1)]
    dead = set()

    def walk(j, C):
        if any(C[w] != M[w] and w not in later_targets[j] for w in range(n)) or (j, C) in dead:
            return None
        if j == len(cand):
            return []
        _, c, t = ops[cand[j]]
        C2 = list(C); C2[t] ^= C2[c]
        rest = walk(j + 1, tuple(C2))
        if rest is not None:
            return [cand[j]] + rest
        rest = walk(j + 1, C)
        if rest is None:
            dead.add((j, C))
        return rest
    return walk(0, tuple(ident))


def executed_order(ansatz, n, L, W):
    """Program indices of the ops in the order the plan executes them (every op exactly once)."""
    ops = program_ops(ansatz, n, L, W)
    pending = list(range(len(ops)))
    order = []
    for kind, what in executed_blocks(W):
        if kind == "CX":
            take = cx_members(pending, ops, what, n)
            assert take is not None, "a CNOT block of the plan is no product of CNOTs still to run"
        elif kind == "CZ":
            take = []
            for a, b in what:
                take.append(next(i for i in pending if i not in take and ops[i][0] == "CZ" and {ops[i][1], ops[i][2]} == {a, b}))
        else:
            take = [next(i for i in pending if ops[i][0] == "U" and ops[i][2] == f) for f in what]
        for i in sorted(take):
            pending.remove(i)
            order.append(i)
    assert not pending, [ops[i] for i in pending]
    return ops, order


GENERIC_U = np.array([[0.6 + 0.3j, -0.2 + 0.71j], [0.1 + 0.73j, 0.55 - 0.39j]])     # neither diagonal nor a permutation
GENERIC_U = np.linalg.qr(GENERIC_U)[0]


def dense(op, support):
    """The op as a matrix on the qubits of `support` (a generic unitary stands for every fused U)."""
    m = len(support)
    pos = {w: m - 1 - j for j, w in enumerate(support)}
    D = np.zeros((1 << m, 1 << m), dtype=complex)
    for x in range(1 << m):
        if op[0] == "U":
            b = x >> pos[op[1]] & 1
            for b2 in (0, 1):
                D[x ^ ((b ^ b2) << pos[op[1]]), x] += GENERIC_U[b2, b]
        elif op[0] == "CX":
            D[x ^ ((x >> pos[op[1]] & 1) << pos[op[2]]), x] = 1
        else:
            D[x, x] = -1 if (x >> pos[op[1]] & 1) and (x >> pos[op[2]] & 1) else 1
    return D


@functools.lru_cache(maxsize=None)
def commute(a, b):
    sup = tuple(sorted(set(wires_of(a)) | set(wires_of(b))))
    A, B = dense(a, sup), dense(b, sup)
    return bool(np.allclose(A @ B, B @ A, atol=1e-12))


def wires_of(op):
    return (op[1],) if op[0] == "U" else (op[1], op[2])


def key(op):
    return (op[0], op[1], -1) if op[0] == "U" else op


def test_out_of_order_pairs_commute():
    """Every ansatz at n = 3 ... 6, L = 1 ... 3, every tile size that gives 2 to 4 passes, both register-wire counts, read map
    on and off; and the default tile (DEFAULT_TILE), where the rule is in use: there some pairs run out of order although
    they share a wire, with forced tiles none does."""
    plans, sharing, sharing_forced = 0, 0, 0
    cases = [(c, f, kb) for c, f in itertools.product(SMALL, (0, READ_MAP, R3, R3 | READ_MAP)) for kb in small_tiles(*c, f)]
    cases += [(c, f, 0) for c, f in itertools.product(DEFAULT_TILE, (0, R3, R3 | READ_MAP))]
    for (ansatz, n, L), flags, kb in cases:
        W = words(ansatz, n, L, kb | flags)
        ops, order = executed_order(ansatz, n, L, W)
        assert sorted(order) == list(range(len(ops)))
        at = {i: t for t, i in enumerate(order)}
        for i, j in itertools.combinations(range(len(ops)), 2):
            if at[j] < at[i]:
                assert commute(key(ops[i]), key(ops[j])), (ansatz, n, L, kb, hex(flags), ops[i], ops[j])
                shared = bool(set(wires_of(ops[i])) & set(wires_of(ops[j])))
                sharing += shared and kb == 0
                sharing_forced += shared and kb != 0
        plans += 1
    assert plans >= 100 and sharing > 0 and sharing_forced == 0, (plans, sharing, sharing_forced)


def test_the_pair_check_sees_an_illegal_order():
    """The matrices tell apart what the rule does: Z-type pairs commute, an X-type meeting does not."""
    assert commute(("CZ", 0, 2), ("CZ", 2, 4)) and commute(("CZ", 0, 2), ("CX", 2, 3)) and commute(("CX", 1, 2), ("CX", 1, 3))
    assert commute(("CX", 0, 2), ("CX", 1, 2))                                  # (a shared target: legal, not taken by the planner)
    assert not commute(("CZ", 0, 2), ("CX", 1, 2)) and not commute(("CX", 0, 1), ("CX", 1, 2))
    assert not commute(("U", 2, -1), ("CZ", 0, 2)) and not commute(("U", 2, -1), ("CX", 2, 3)) and commute(("U", 1, -1), ("CZ", 0, 2))


# ------------------------------------------------------------------------------------------------ emulated plans
@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
def test_small_emulated_plans_match_the_oracle(ansatz):
    """The circuits of the legality test, run as the generic kernel runs a plan, with 8 and with 16 amplitudes per thread."""
    ran = 0
    for (a, n, L), flags in itertools.product(SMALL, (0, READ_MAP, R3, R3 | READ_MAP)):
        if a != ansatz:
            continue
        th = np.random.default_rng(n * 17 + L).uniform(-np.pi, np.pi, oc.num_params(a, n, L))
        ref = oc.probs(a, n, L, th)
        for kb in small_tiles(a, n, L, flags):
            W = words(a, n, L, kb | flags)
            np.testing.assert_allclose(pe.run_plan(W, pe.fused_matrices(W, th)), ref, rtol=0, atol=ATOL, err_msg=str((a, n, L, kb, hex(flags))))
            ran += 1
    assert ran >= 30, ran


@pytest.mark.parametrize("ansatz,n,L,kb", MEDIUM + [(a, n, L, 0) for a, n, L in DEFAULT_TILE if (n, L) != (16, 6)])
def test_medium_emulated_plans_match_the_oracle(ansatz, n, L, kb):
    """n = 9, 10 with 2^6 ... 2^8 tiles, and the default tile (kb = 0: the plans the rule changes): the stage headers of both plans with the read map on and off, and the compact
    tables run as circuit_pass_r3_kernel runs them, direct first / last stages on and off, support of |0..0> on and off."""
    from tensornetworks_amd import _ext
    aid = _ext.ANSATZ_IDS[ansatz]
    th = np.random.default_rng(n * 19 + L).uniform(-np.pi, np.pi, oc.num_params(ansatz, n, L))
    ref = oc.probs(ansatz, n, L, th)
    for flags in (0, READ_MAP, R3, R3 | READ_MAP):
        W = words(ansatz, n, L, kb | flags)
        assert int(W[pe.PH_NPASSES]) >= 2 or kb == 0
        np.testing.assert_allclose(pe.run_plan(W, pe.fused_matrices(W, th)), ref, rtol=0, atol=ATOL, err_msg=hex(flags))
    W = words(ansatz, n, L, kb | R3)
    Cw, coffs = _ext.plan_compact_words(aid, n, L, kb)           # (the compact emulator takes plans without cross reads)
    if n < 6:
        return                                                   # (tiles below 2^6: no compact tables)
    assert Cw is not None and len(coffs) == int(W[pe.PH_NPASSES])
    assert _ext.plan_compact_words(aid, n, L, kb | READ_MAP)[0] is not None        # (the builder's point evaluation accepts both)
    mats = pe.fused_matrices(W, th)
    for direct, zs in ((3, True), (3, False), (0, True), (0, False)):
        np.testing.assert_allclose(pe.run_plan_compact(W, (Cw, coffs), mats, direct=direct, zero_support=zs), ref, rtol=0, atol=ATOL)


def test_zero_support_on_the_changed_plans():
    """The INIT pass of these plans runs one stage more than it did: the tiles it leaves out and the slots the pass behind
    it does not load are still only zeros (the emulator poisons the former and asserts the latter), and the masks are in use."""
    from tensornetworks_amd import _ext
    used = 0
    for n, L, kb, flags in [(14, 3, 0, 0), (14, 3, 0, R3), (14, 3, 0, R3 | READ_MAP), (15, 2, 0, R3 | READ_MAP)]:
        W = words("hardware_efficient", n, L, kb | flags)
        F, offs = _ext.plan_fast_words(0, n, L, kb | flags)
        assert F is not None
        gmask, zslots = int(F[offs[0] + pe.FH_ZINFO]), int(F[offs[1] + pe.FH_ZINFO])
        assert (gmask == 0) == (zslots == 0)
        used += gmask != 0
        th = np.random.default_rng(n + L).uniform(-np.pi, np.pi, oc.num_params("hardware_efficient", n, L))
        q = pe.run_plan(W, pe.fused_matrices(W, th), fast=(F, offs))
        np.testing.assert_allclose(q, oc.probs("hardware_efficient", n, L, th), rtol=0, atol=ATOL)
    assert used >= 2


# ------------------------------------------------------------------------------------------------ against the parent
def test_passes_and_stages_never_rise():
    """All three ansaetze, n = 8 ... 24, L = 1 ... 8, read map on and off; three register wires with the default tile, four
    with the default tile up to n = 16 and with forced tiles beyond (the fixture's variants; forced tiles keep their plans)."""
    from tensornetworks_amd import _ext
    parent = golden("plan_shapes_parent.npz")["stages"]
    fewer, compared = 0, 0
    for a, n, L, rm in itertools.product(range(3), shapes.N_RANGE, shapes.L_RANGE, (0, 1)):
        for v, flags in enumerate(shapes.variant_flags(n)):
            was = [int(s) for s in parent[a, n - 8, L - 1, v, rm] if s != -1]
            if flags is None or was == [-2]:
                continue                                   # (not recorded; no plan before: more than 32 stages in one pass)
            now = shapes.stage_counts(_ext.plan_words(a, n, L, flags | (READ_MAP if rm else 0)))
            assert len(now) <= len(was) and sum(now) <= sum(was), (a, n, L, v, rm, was, now)
            if len(now) == len(was) and sum(now) == sum(was) and now != was:
                assert len(now) > 1 and now[0] > was[0], (a, n, L, v, rm, was, now)    # only the INIT pass may have taken more
            fewer += sum(now) < sum(was)
            compared += 1
    assert compared >= 2000 and fewer >= 40, (compared, fewer)


@pytest.mark.parametrize("n,L,pinned", [(16, 6, [8, 6, 5, 5, 5, 4, 2]), (20, 8, [8, 7, 5, 4, 5, 5, 4, 5, 5, 4, 5, 1])])
def test_benchmark_plans_are_pinned(n, L, pinned):
    """hardware_efficient under the default options (three register wires, read map): these per-pass stage counts or better
    -- no more passes, no more stages in all, outside the INIT pass, or in the last pass (the fused dot's)."""
    now = shapes.stage_counts(words("hardware_efficient", n, L, R3 | READ_MAP))
    assert len(now) <= len(pinned) and sum(now) <= sum(pinned) and sum(now[1:]) <= sum(pinned[1:]) and now[-1] <= pinned[-1], now


def test_bit_recorded_circuits_plan_word_for_word():
    fixture = golden("plan_shapes_parent.npz")
    for (ansatz, n, L), flags in itertools.product(shapes.BIT_CIRCUITS, shapes.FLAGS):
        np.testing.assert_array_equal(words(ansatz, n, L, flags), fixture[shapes.words_key(ansatz, n, L, flags)],
                                      err_msg=f"{ansatz} n={n} L={L} flags={flags:#x}")
    for n, L in ((12, 4), (8, 4)):                    # single-tile benchmark sizes: same stage count either way, so the same plan
        assert len(shapes.stage_counts(words("hardware_efficient", n, L, R3 | READ_MAP))) == 1
