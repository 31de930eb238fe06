"""Records tests/golden/plan_shapes_parent.npz: what the circuit planner (csrc/plan.cpp) emits, on the last commit before
diagonal gates were allowed to commute past blocked diagonal gates.  Host only: the planner needs no GPU.

  stages   int8 [ansatz 0..2][n - 8, n = 8..24][L - 1, L = 1..8][variant][read_map][pass]: LDS stages of every pass, -1
           behind the last pass; -2 in front where the planner refuses the circuit (more than MAX_STAGES stages in one
           pass: a deep single-tile circuit).  Variants (variant_flags below): three register wires with the default tile;
           four register wires with the default tile up to n = 16 and with 2^13 tiles forced beyond; four register wires
           with 2^11 tiles forced (n > 13 only).  With four register wires make_plan chooses between those two tile sizes
           by building the 16-amplitude kernel's tables, which takes most of a second per plan from n = 17 on: there both
           candidates are recorded in place of the choice.
  words/<ansatz>_<n>_<L>_<flags>   the serialised plan, word for word, of the circuits whose results are recorded bit for bit
           under tests/golden/ (quantum_step_parent_bits.npz and its neighbours), for reg_wires 3 and 4 with and without
           the read map (`flags` as _ext.plan_words takes them)

tests/test_plan_commute_host.py holds a later planner against both: never more passes or stages, and the same words for the
recorded circuits.  This file calls only _ext.plan_words, so it alone can be copied onto the commit to be recorded.
Run from the repository root: python tests/golden/make_golden_plan_shapes.py [output.npz [libbornvi_hip.so]]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

ANSATZE = ("hardware_efficient", "all_to_all", "basic")           # ids 0, 1, 2
N_RANGE, L_RANGE = range(8, 25), range(1, 9)
MAX_PASSES = 48
R3, READ_MAP = 0x200, 0x100


def variant_flags(n):
    """plan_words flags of the recorded variants at this n (None: not recorded)."""
    return (R3, 13 if n > 16 else 0, 11 if n > 13 else None)

BIT_CIRCUITS = (("hardware_efficient", 3, 2), ("basic", 4, 2), ("hardware_efficient", 14, 1))
FLAGS = (0x000, 0x100, 0x200, 0x300)                             # bit 8: read map, bit 9: 3 register wires


def stage_counts(W):
    """LDS stages per pass of a serialised plan (plan.hpp: PH_NPASSES, PH_OFF_PASSTAB, PW_NSTAGES)."""
    return [int(W[int(W[int(W[7]) + i]) + 3]) for i in range(int(W[3]))]


def words_key(ansatz, n, L, flags):
    return f"words/{ansatz}_{n}_{L}_{flags:#05x}"


if __name__ == "__main__":
    from tensornetworks_amd import _ext
    if len(sys.argv) > 2:
        _ext.LIB_PATH = sys.argv[2]           # (the library of the commit to record, built elsewhere)
    stages = np.full((len(ANSATZE), len(N_RANGE), len(L_RANGE), 3, 2, MAX_PASSES), -1, dtype=np.int8)
    for a, ansatz in enumerate(ANSATZE):
        assert _ext.ANSATZ_IDS[ansatz] == a
        for n in N_RANGE:
            for L in L_RANGE:
                for v, flags in enumerate(variant_flags(n)):
                    for rm in (0, 1):
                        if flags is None:
                            continue
                        try:
                            st = stage_counts(_ext.plan_words(a, n, L, flags | (READ_MAP if rm else 0)))
                        except _ext.BornviError:
                            st = [-2]
                        assert len(st) <= MAX_PASSES and max(st) < 128
                        stages[a, n - 8, L - 1, v, rm, :len(st)] = st
        print(ansatz, "recorded", flush=True)
    out = {"stages": stages}
    for ansatz, n, L in BIT_CIRCUITS:
        for flags in FLAGS:
            out[words_key(ansatz, n, L, flags)] = _ext.plan_words(_ext.ANSATZ_IDS[ansatz], n, L, flags)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "plan_shapes_parent.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
