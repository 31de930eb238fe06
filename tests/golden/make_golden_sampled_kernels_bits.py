"""Records tests/golden/sampled_kernels_parent_bits.npz: what every sampled-MPS backend call computes on an MI355X, bit for
bit, at the smallest shapes at which each of its paths can go wrong.  Per case, after mps_environments (log Z): mps_sample
(idx, logq, status), mps_score_vjp with seeded weights (grad, logq, status), mps_score_rows for all sites and for a proper
sub-range of them (rows, status), mps_score_sample_gram where B <= 1024 (T, status) and mps_score_jvp with a seeded
direction and scale = 1 / B (t, status).  Cores, weights and directions come from numpy.random.RandomState on the host.
A case is stored as one byte string, its pieces in the order pieces() yields them; a piece of more than KEEP_UP_TO bytes
is stored as the SHA-256 of its bytes.

tests/test_gpu_sampled_kernels_bits.py takes its cases, pieces() and piece_bytes() from here, and only backend calls are
used, so this file alone can be copied onto the commit whose bits are to be kept and run there.  The file in the
repository was recorded on the last commit before the kernels' site sweeps moved into mps_sample_dev.hpp.  Run from the
repository root: python tests/golden/make_golden_sampled_kernels_bits.py [output.npz]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

SEED = 11
SAMPLER_SEED, SAMPLER_EPOCH = 5, 3
KEEP_UP_TO = 64 * 1024
GRAM_MAX_BATCH = 1024
# (n, D, B, kind)
CASES = [(1, 2, 65, "plain"),          # the k < n branches never taken; a partial second tile
         (3, 3, 130, "plain"),         # DP = 4 with padding; odd D
         (5, 5, 65, "plain"),          # DP = 8
         (4, 9, 130, "plain"),         # DP = 16
         (3, 17, 65, "plain"),         # DP = 32 with padding: the second 16-wide matrix-core tile partly masked
         (2, 32, 65, "plain"),         # DP = 32 without padding
         (63, 4, 130, "plain"),        # every bit of the index word; 63 rescales
         (3, 2, 16449, "plain"),       # more tiles than workgroups: the partials are added, not stored.  No Gram
         (8, 3, 130, "scaled"),        # site k times 2^+200 (k odd), 2^-200 (k even): the exponent bookkeeping
         (3, 2, 65, "zero")]           # A_1[1] = 0 and idx = arange(B) % 8: zero-amplitude samples in every score kernel


def case_id(case):
    return "-".join(str(v) for v in case)


def host_inputs(case):
    """(cores [n, 2, D, D], weights [B], direction [n, 2, D, D]) of one case, float64 on the host."""
    n, D, B, kind = case
    rs = np.random.RandomState(SEED)
    cores = rs.standard_normal((n, 2, D, D)) / np.sqrt(D)
    w = rs.standard_normal(B)
    v = rs.standard_normal((n, 2, D, D))
    if kind == "scaled":
        for k in range(1, n + 1):
            cores[k - 1] = np.ldexp(cores[k - 1], 200 if k & 1 else -200)
    if kind == "zero":
        cores[0, 1] = 0.0
    return cores, w, v


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def pieces(case):
    """[(name, array), ...] of one case, in a fixed order."""
    import torch
    from tensornetworks_amd import backend
    n, D, B, kind = case
    dev = backend.compute_device()
    cores_h, w_h, v_h = host_inputs(case)
    cores, w, v = (torch.from_numpy(a).to(dev) for a in (cores_h, w_h, v_h))
    out = [("environments/log_Z", _host(backend.mps_environments(cores, B)))]
    epoch = torch.tensor([SAMPLER_EPOCH], dtype=torch.int64, device=dev)
    idx, logq, status = backend.mps_sample(cores, B, SAMPLER_SEED, epoch)
    out += [("sample/idx", _host(idx)), ("sample/logq", _host(logq)), ("sample/status", _host(status))]
    if kind == "zero":
        idx = (torch.arange(B, dtype=torch.int64) % 8).to(dev)
    grad, logq, status = backend.mps_score_vjp(cores, idx, w)
    out += [("vjp/grad", _host(grad)), ("vjp/logq", _host(logq)), ("vjp/status", _host(status))]
    rows, status = backend.mps_score_rows(cores, idx)
    out += [("rows/all", _host(rows)), ("rows/all/status", _host(status))]
    if n >= 3:                           # a proper sub-range: k_begin >= 1, k_begin + k_count < n
        rows, status = backend.mps_score_rows(cores, idx, 1, n - 2)
        out += [("rows/sub", _host(rows)), ("rows/sub/status", _host(status))]
    if B <= GRAM_MAX_BATCH:
        T, status = backend.mps_score_sample_gram(cores, idx)
        out += [("gram/T", _host(T)), ("gram/status", _host(status))]
    t, status = backend.mps_score_jvp(cores, idx, v, 1.0 / B)
    return out + [("jvp/t", _host(t)), ("jvp/status", _host(status))]


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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sampled_kernels_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")
