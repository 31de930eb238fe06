"""Records tests/golden/mps_query_parent_bits.npz: what the posterior-query, log-marginal-gradient and canonical-form backend
calls compute on an MI355X, bit for bit, at the smallest shapes at which each of their paths can go wrong.  Per case: the three
workspace sizes; mps_log_marginals over Q evidences (logm, status); mps_log_marginals_vjp with seeded weights, the last of them
exactly 0.0 (grad, logm, status); mps_sample_clamped at B = 65 under evidence 2 (idx, logq, logm, status); mps_marginals with
pairs (m1, m2); mps_canonicalise at D_out = D and at D_out = max(1, D // 2), both with cutoff 0 (all six outputs).  Cores,
weights and evidences come from numpy.random.RandomState on the host: evidence 0 is the empty mask, evidence 1 the full one, the
last one clamps site 1 (bit n - 1) among others; in a "zero" case every even evidence from 2 on clamps site 1 to 1, which
A_1[1] = 0 makes impossible.  A case is stored as one byte string, its pieces in the order pieces() yields them; a piece of
more than KEEP_UP_TO bytes is stored as the SHA-256 of its bytes.

tests/test_gpu_mps_query_bits.py takes its cases, pieces() and piece_bytes() from here, and only backend calls are used, so
this file alone can be copied onto the commit whose bits are to be kept and run there.  The file in the repository was
recorded on the last commit before the clamped environment sweep and the workgroup-level products moved into
mps_sample_dev.hpp.  Run from the repository root: python tests/golden/make_golden_mps_query_bits.py [output.npz]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

SEED = 13
SAMPLER_SEED, SAMPLER_EPOCH, SAMPLER_BATCH = 5, 3, 65
KEEP_UP_TO = 64 * 1024
# (n, D, Q, kind)
CASES = [(1, 2, 3, "plain"),           # no k < n step anywhere; the canon kernel's n = 1 branch
         (3, 3, 5, "plain"),           # odd D; Q below the vjp's 256 workgroups
         (5, 5, 300, "plain"),         # Q above 256: a vjp workgroup takes queries g and g + 256, its partial is added to
         (4, 17, 3, "plain"),          # D D = 289 > 256: the second slot of the environment step's four; the canon groups' second column
         (2, 32, 3, "plain"),          # D D = 1024: all four slots, no padding anywhere
         (63, 4, 4, "plain"),          # every bit of the words; 63 rescales; a mask with bit 62 set
         (8, 3, 6, "scaled"),          # site k times 2^+200 (k odd), 2^-200 (k even): the exponent bookkeeping of both sweeps
         (3, 2, 8, "zero")]            # A_1[1] = 0 and evidences that clamp site 1 to 1: logm -inf, status 1, the vjp's `continue`


def case_id(case):
    return "-".join(str(v) for v in case)


def host_inputs(case):
    """(cores [n, 2, D, D] float64, mask [Q] int64, value [Q] int64, weights [Q] float64) of one case, on the host."""
    n, D, Q, kind = case
    rs = np.random.RandomState(SEED)
    cores = rs.standard_normal((n, 2, D, D)) / np.sqrt(D)
    c = rs.standard_normal(Q)
    c[Q - 1] = 0.0
    bits = rs.randint(0, 2, size=(2, Q, n)).astype(np.uint64)
    words = (bits << np.arange(n, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)        # bit n - k of a word: site k
    mask, value = words[0], words[1]
    top = np.uint64(1) << np.uint64(n - 1)
    mask[0] = 0
    mask[1] = (np.uint64(1) << np.uint64(n)) - np.uint64(1)
    mask[Q - 1] |= top
    if kind == "scaled":
        for k in range(1, n + 1):
            cores[k - 1] = np.ldexp(cores[k - 1], 200 if k & 1 else -200)
    if kind == "zero":
        cores[0, 1] = 0.0
        mask[2::2] |= top
        value[2::2] |= top
    return cores, mask.astype(np.int64), value.astype(np.int64), c


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def pieces(case):
    """[(name, array), ...] of one case, in a fixed order."""
    import torch
    from tensornetworks_amd import backend
    n, D, Q, kind = case
    dev = backend.compute_device()
    cores, mask, value, c = (torch.from_numpy(a).to(dev) for a in host_inputs(case))
    h = backend._ext.handle_for(dev)
    sizes = [h.size("bornvi_mps_query_workspace_bytes", n, D, Q), h.size("bornvi_mps_log_marginals_vjp_workspace_bytes", n, D, Q),
             h.size("bornvi_mps_canon_workspace_bytes", n, D)]
    out = [("workspace_bytes", np.asarray(sizes, dtype=np.int64))]
    logm, status = backend.mps_log_marginals(cores, mask, value)
    out += [("log_marginals/logm", _host(logm)), ("log_marginals/status", _host(status))]
    grad, logm, status = backend.mps_log_marginals_vjp(cores, mask, value, c)
    out += [("vjp/grad", _host(grad)), ("vjp/logm", _host(logm)), ("vjp/status", _host(status))]
    epoch = torch.tensor([SAMPLER_EPOCH], dtype=torch.int64, device=dev)
    idx, logq, logm, status = backend.mps_sample_clamped(cores, SAMPLER_BATCH, mask[2:3].contiguous(), value[2:3].contiguous(),
                                                         SAMPLER_SEED, epoch)
    out += [("clamped/idx", _host(idx)), ("clamped/logq", _host(logq)), ("clamped/logm", _host(logm)), ("clamped/status", _host(status))]
    m1, m2 = backend.mps_marginals(cores, want_pairs=True)
    out += [("marginals/m1", _host(m1)), ("marginals/m2", _host(m2))]
    for tag, Do in (("full", D), ("half", max(1, D // 2))):
        names = ("cores", "schmidt", "discarded", "rank", "log_norm", "status")
        out += [(f"canon/{tag}/{name}", _host(a)) for name, a in zip(names, backend.mps_canonicalise(cores, Do, 0.0))]
    return out


def piece_bytes(a, keep_up_to=None):
    raw = np.ascontiguousarray(a).tobytes()
    return hashlib.sha256(raw).digest() if len(raw) > (KEEP_UP_TO if keep_up_to is None else keep_up_to) else raw


def blob(ps, keep_up_to=None):
    return np.frombuffer(b"".join(piece_bytes(a, keep_up_to) for _, a in ps), dtype=np.uint8)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    out = {}
    for case in CASES:
        b = blob(pieces(case))
        assert np.array_equal(b, blob(pieces(case))), f"{case_id(case)}: two runs differ"
        out[case_id(case)] = b
        print(f"{case_id(case)}: {b.size} bytes, sha256 {hashlib.sha256(b.tobytes()).hexdigest()[:16]}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "mps_query_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")
