"""Records tests/golden/reduce_parent_bits.npz: what the backend calls whose kernels took their fixed-order reductions from
csrc/reduce_dev.hpp compute on an MI355X, bit for bit, for the calls the other parent-bit tests do not reach or reach at
one workgroup only.  What those reach: test_gpu_sampled_kernels_bits.py mps_environments, mps_sample, mps_score_vjp,
mps_score_rows, mps_score_sample_gram, mps_score_jvp; test_gpu_gram_bits.py fisher_gram, qfi_gram; the recorded epochs of
test_gpu_sampled_natgrad_trainer.py (natural_gradient=None) the first three of those plus bn_logjoint_samples,
bn_score_samples and stein_pairs_rowsum inside five epochs (B = 1024 and 257); test_gpu_family_surface_bits.py born_table_probs,
born_table_vjp, elbo_weights, mps_probs, mps_vjp at n = 3 and n = 6 (a single chunk, a single fused launch); and
test_gpu_quantum_step_bits.py the circuit, Stein, Fisher and QFI calls, spd_solve, shots_histogram at n = 3 (one level: no
mass kernel) and the adjoint calls at n = 3.  Per call below the smallest cases that reach every branch of its reduction:
one workgroup with fewer elements than threads, and more than one partial.

  table    born_table_probs (q32, q64, H) and born_table_vjp (grad, loss) in both modes, elbo_weights: 2 rows at n = 3 and
           at n = 13 (two chunks of 4096)
  reinforce  reinforce_step twice (first call, then the running baseline) at n = 13: B = 5 and B = 2500 (three sample chunks)
  cg       cg_init, three cg_step with F = a positive diagonal, cg_finish: P = 7 and P = 3000 (more elements than threads)
  mps      enumerated mps_probs and mps_vjp: n = 3, D = 2 and n = 12, D = 3 (one streamed level: partials of Z and of dA)
  stein    bn_score_samples and stein_pairs_rowsum on synthetic_network(5): B = 65 and B = 257
  shots    shots_histogram, n = 13 (two levels: the mass kernel runs), 3 rows
  adjoint  adjoint_state and adjoint_vjp, hardware-efficient ansatz, n = 4, two layers
  query    mps_log_marginals (Q = 3), mps_marginals with pairs, mps_sample_clamped (B = 100): n = 5, D = 3

Inputs come from numpy.random.RandomState on the host.  A case is stored as one byte string, its pieces in the order
pieces() yields them; a piece of more than KEEP_UP_TO bytes is stored as the SHA-256 of its bytes.

tests/test_gpu_reduce_bits.py takes its cases, pieces() and piece_bytes() from here, and only backend calls are used, so
this file alone can be copied onto the commit whose bits are to be kept and run there.  The file in the repository was
recorded with the library of the last commit before reduce_dev.hpp.  Run from the repository root:
python tests/golden/make_golden_reduce_bits.py [output.npz]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

SEED = 13
KEEP_UP_TO = 4096
CASES = [("table", 3), ("table", 13),
         ("reinforce", 13, 5), ("reinforce", 13, 2500),
         ("cg", 7), ("cg", 3000),
         ("mps", 3, 2), ("mps", 12, 3),
         ("stein", 5, 65), ("stein", 5, 257),
         ("shots", 13, 3),
         ("adjoint", 4, 2),
         ("query", 5, 3, 3, 100)]


def case_id(case):
    return "-".join(str(v) for v in case)


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _named(prefix, names, tensors):
    return [(f"{prefix}/{name}", _host(t)) for name, t in zip(names, tensors)]


def _table(dev, rs, n):
    import torch
    from tensornetworks_amd import backend
    N, rows = 1 << n, 2
    w = torch.from_numpy(rs.standard_normal((rows, N)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.standard_normal((rows, N))).to(dev)
    ksd2 = torch.from_numpy(rs.random_sample(rows) + 0.5).to(dev)
    log_p = torch.from_numpy(-4.0 * rs.random_sample(N) - 1.0).to(dev)
    out = []
    for mode in (0, 1):
        q32, q64, H = backend.born_table_probs(w, mode)
        loss = torch.empty(rows, dtype=torch.float64, device=dev)
        grad = backend.born_table_vjp(w, q64, mode, y=y, ksd2=ksd2, entropy_weight=0.01, loss_out=loss)
        out += _named(f"mode{mode}", ("q32", "q64", "H", "grad", "loss"), (q32, q64, H, grad, loss))
        if mode == 0:
            out += _named("elbo", ("neg_elbo", "entropy", "w"), backend.elbo_weights(q64, log_p))
    return out


def _reinforce(dev, rs, n, B):
    import torch
    from tensornetworks_amd import backend
    N = 1 << n
    idx = torch.from_numpy(rs.randint(0, N, B).astype(np.int64)).to(dev)
    logit = torch.from_numpy(rs.standard_normal(B).astype(np.float32)).to(dev)
    log_p = torch.from_numpy((-4.0 * rs.random_sample(N) - 1.0).astype(np.float32)).to(dev)
    q = rs.random_sample(N) + 0.01
    q32 = torch.from_numpy((q / q.sum()).astype(np.float32)).to(dev)
    baseline = torch.zeros(1, dtype=torch.float64, device=dev)
    out = []
    for call, first in enumerate((True, False)):
        dLdq, loss, found = backend.reinforce_step(idx, logit, log_p, q32, baseline, first, 0.9)
        out += _named(f"call{call}", ("dLdq", "loss", "found_inf", "baseline"), (dLdq, loss, found, baseline))
    return out


def _cg(dev, rs, P):
    import torch
    from tensornetworks_amd import backend
    g = torch.from_numpy(rs.standard_normal(P)).to(dev)
    d = torch.from_numpy(rs.random_sample(P) + 0.5).to(dev)          # F = diag(d): F p is one exactly rounded product per entry
    x, r, p, state, info = backend.cg_init(g)
    out = _named("init", ("x", "r", "p", "state", "info"), (x, r, p, state, info))
    for it in range(3):
        backend.cg_step(d * p, x, r, p, state, 1e-3, 1e-12)
        out += _named(f"step{it}", ("x", "r", "p", "state"), (x, r, p, state))
    return out + _named("finish", ("x", "info", "iters", "relres"), backend.cg_finish(g, x, state))


def _mps(dev, rs, n, D):
    import torch
    from tensornetworks_amd import backend
    cores = torch.from_numpy(rs.standard_normal((n, 2, D, D)) / np.sqrt(D)).to(dev)
    g = torch.from_numpy(rs.standard_normal(1 << n)).to(dev)
    out = _named("probs", ("q32", "q64", "psi", "Z"), backend.mps_probs(cores, want_q32=True, want_psi=True))
    return out + [("vjp/grad", _host(backend.mps_vjp(cores, g)))]


def _stein(dev, rs, n, B):
    import torch
    from tensornetworks_amd import backend
    from tensornetworks_amd.bayesian_network import pack_network, synthetic_network
    bn, lat, obs, x = synthetic_network(n, 0)
    keep, desc = backend.bn_descriptor(pack_network(bn, lat, x), dev)
    idx = torch.from_numpy(rs.randint(0, 1 << n, B).astype(np.int64)).to(dev)
    S, logp = backend.bn_score_samples(desc, n, idx, want_logp=True)
    r, total = backend.stein_pairs_rowsum(idx, S, n)
    torch.cuda.synchronize()             # `keep` (the descriptor's arrays) outlives the kernels
    return _named("stein", ("S", "logp", "r", "total"), (S, logp, r, total))


def _shots(dev, rs, n, B):
    import torch
    from tensornetworks_amd import backend
    p = rs.random_sample((B, 1 << n)) ** 4
    p[rs.random_sample(p.shape) < 0.25] = 0.0
    probs = torch.from_numpy(p / p.sum(axis=1, keepdims=True)).to(dev)
    epoch = torch.tensor([2], dtype=torch.int64, device=dev)
    return [("shots/freq", _host(backend.shots_histogram(probs, n, 1000, 17, epoch)))]


def _adjoint(dev, rs, n, layers):
    import torch
    from tensornetworks_amd import backend
    ansatz = "hardware_efficient"
    theta = torch.from_numpy(rs.uniform(-np.pi, np.pi, backend.num_params(ansatz, n, layers))).to(dev)
    dLdq = torch.from_numpy(rs.standard_normal(1 << n)).to(dev)
    state, probs = backend.adjoint_state(ansatz, n, layers, theta)
    grad = backend.adjoint_vjp(ansatz, n, layers, theta, state, dLdq)
    return [("adjoint/state", _host(torch.view_as_real(state)))] + _named("adjoint", ("probs", "grad"), (probs, grad))


def _query(dev, rs, n, D, Q, B):
    import torch
    from tensornetworks_amd import backend
    cores = torch.from_numpy(rs.standard_normal((n, 2, D, D)) / np.sqrt(D)).to(dev)
    mask = torch.from_numpy(rs.randint(0, 1 << n, Q).astype(np.int64)).to(dev)
    value = torch.from_numpy(rs.randint(0, 1 << n, Q).astype(np.int64)).to(dev) & mask
    epoch = torch.tensor([3], dtype=torch.int64, device=dev)
    out = _named("log_marginals", ("logm", "status"), backend.mps_log_marginals(cores, mask, value))
    out += _named("marginals", ("m1", "m2"), backend.mps_marginals(cores, want_pairs=True))
    return out + _named("sample_clamped", ("idx", "logq", "logm", "status"),
                        backend.mps_sample_clamped(cores, B, mask[:1].clone(), value[:1].clone(), 5, epoch))


def pieces(case):
    """[(name, array), ...] of one case, in a fixed order."""
    from tensornetworks_amd import backend
    kind = {"table": _table, "reinforce": _reinforce, "cg": _cg, "mps": _mps, "stein": _stein, "shots": _shots,
            "adjoint": _adjoint, "query": _query}[case[0]]
    return kind(backend.compute_device(), np.random.RandomState(SEED), *case[1:])


def piece_bytes(a):
    raw = np.ascontiguousarray(a).tobytes()
    return hashlib.sha256(raw).digest() if len(raw) > KEEP_UP_TO else raw


def blob(ps):
    return np.frombuffer(b"".join(piece_bytes(a) for _, a in ps), dtype=np.uint8)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    out = {}
    for case in CASES:
        b = blob(pieces(case))
        assert np.array_equal(b, blob(pieces(case))), f"{case_id(case)}: two runs differ"
        out[case_id(case)] = b
        print(f"{case_id(case)}: {b.size} bytes, sha256 {hashlib.sha256(b.tobytes()).hexdigest()[:16]}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "reduce_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")
