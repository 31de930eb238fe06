"""Records tests/golden/init_walk_rows_parent_bits.npz: the rows circuit_probs computes on an MI355X, bit for bit, for
multi-pass plans of circuit_pass_r3_kernel, recorded with the library of the last commit in which an INIT pass still gave
every tile of the batch a loop trip.  The INIT pass now walks only the tiles it writes (kernels_circuit8.hip: zs_free); the
values, their addresses and the arithmetic are the same, so every row must come out with the recorded bits.

A batch draws its rows from two parameter vectors, and a circuit's row does not depend on its place in the batch or on the
grid, so a case keeps its two distinct rows: raw float64 when both fit in KEEP_UP_TO bytes, otherwise a SHA-256 per row.
rows_of() asserts that every row of every grid is one of the two before it returns them.

tests/test_gpu_r3_init_walk.py takes its cases, grids and rows_of() from here, and only backend calls are used, so this file
alone can be copied onto the commit whose bits are to be kept and run there.  Run from the repository root:
python tests/golden/make_golden_init_walk_rows_bits.py [output.npz]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

KEEP_UP_TO = 128 << 10
# (ansatz, n, L, tile_bits) with reg_wires = 3 and the read map on; per pass (stages, direct first, direct last, CH_ZINFO) as
# tests/test_gpu_r3_init_walk.py::test_the_cases_cover_every_walk reads them from the plan words:
CASES = [("hardware_efficient", 13, 3, 9),    # (5,0,1,0x07) (5,1,1,0xfe) ..: 16 tile rows, mask 0x7: INIT writes the zero tiles of row 8 only
         ("all_to_all", 12, 3, 9),            # (3,0,1,0x07) (4,1,1,0xfe) ..: 8 tile rows, all masked; a three-stage INIT pass
         ("hardware_efficient", 14, 4, 11),   # (6,0,1,0x07) (6,1,1,0xfe) ..: 8 tile rows, all masked: the walk ends behind the real tiles
         ("hardware_efficient", 13, 3, 11)]   # (6,0,1,0x03) (6,1,1,0xee) ..: 4 tile rows, all masked; pass 1 loads two slots
OPTIONS = ("tile_bits", "tile_bits_multi", "fast_workgroups_per_cu", "reg_wires", "read_map", "zero_support", "direct_stages")


def case_id(case):
    return "-".join(str(v) for v in case)


def grids(case, cus):
    """{name: batch} with one persistent workgroup per CU (cus workgroups).  partial_last_trip: 100 circuits, several trips
    with a partial last one, and fewer real INIT tiles than workgroups (the others walk zero tiles only, or leave at once);
    one_trip: as many tiles as workgroups (has_next is false in the first real trip);
    real_trips: 600 circuits, so an INIT workgroup runs two or three real tiles before its zero tiles.
    With zero_support = 0 nothing is masked: every zero tile is written, in the order the walk had before."""
    _, n, _, kb = case
    return {"partial_last_trip": 100, "one_trip": cus >> (n - kb), "real_trips": 600}


def thetas(case):
    from tensornetworks_amd import backend
    ansatz, n, L, _ = case
    th = np.random.default_rng(31 * n + L).uniform(-np.pi, np.pi, (2, backend.num_params(ansatz, n, L)))
    th.setflags(write=False)
    return th


def set_case_options(backend, dev, case, zero_support=1):
    backend.set_option(dev, "reg_wires", 3)
    backend.set_option(dev, "read_map", 1)
    backend.set_option(dev, "tile_bits", case[3])
    backend.set_option(dev, "fast_workgroups_per_cu", 1)
    backend.set_option(dev, "zero_support", zero_support)


def rows_of(case, batch, zero_support=1):
    """(pick, q): the batch's rows on the GPU (options as set_case_options; the caller restores them).  Two calls must give
    equal bits and every row must equal the first row of its parameter vector."""
    import torch
    from tensornetworks_amd import backend
    dev = backend.compute_device()
    set_case_options(backend, dev, case, zero_support)
    ansatz, n, L, _ = case
    pick = np.random.default_rng(batch).integers(0, 2, batch)
    pick[:2] = (0, 1)
    t = torch.as_tensor(thetas(case)[pick], dtype=torch.float64, device=dev).contiguous()
    q = backend.circuit_probs(ansatz, n, L, t).cpu().numpy()
    q2 = backend.circuit_probs(ansatz, n, L, t).cpu().numpy()
    assert np.array_equal(q.view(np.uint64), q2.view(np.uint64)), f"{case_id(case)} batch {batch}: two calls differ"
    assert np.array_equal(q.view(np.uint64), q[:2][pick].view(np.uint64)), f"{case_id(case)} batch {batch}: a row depends on its place"
    return pick, q


def row_bytes(two):
    """The two distinct rows as stored: raw, or a SHA-256 per row."""
    raw = np.ascontiguousarray(two).tobytes()
    if len(raw) <= KEEP_UP_TO:
        return np.frombuffer(raw, dtype=np.uint8)
    return np.frombuffer(b"".join(hashlib.sha256(np.ascontiguousarray(r).tobytes()).digest() for r in two), dtype=np.uint8)


if __name__ == "__main__":
    import torch
    from tensornetworks_amd import backend
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = backend.compute_device()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    keep = {k: backend.get_option(dev, k) for k in OPTIONS}
    out = {}
    for case in CASES:
        got = None
        for zs in (1, 0):
            for name, batch in grids(case, cus).items():
                _, q = rows_of(case, batch, zs)
                b = row_bytes(q[:2])
                # (with zero_support = 0 pass 1 loads the zeros pass 0 then writes instead of leaving the slots out: same bits)
                assert got is None or np.array_equal(b, got), f"{case_id(case)} {name} zero_support {zs}: rows differ from the first grid's"
                got = b
        out[case_id(case)] = got
        print(f"{case_id(case)}: {got.size} bytes, sha256 {hashlib.sha256(got.tobytes()).hexdigest()[:16]}", flush=True)
    for k, v in keep.items():
        backend.set_option(dev, k, v)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "init_walk_rows_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")
