"""Records tests/golden/quantum_step_parent_bits.npz: what the two quantum trainers (KSD and exact ELBO) compute on an
MI355X through their public surface, bit for bit, at the smallest sizes at which the host plumbing between trainer,
gradient route and kernels can go wrong.  Four sorts of case:

  step   one eager device step (loss, gradient, q, every _step_extras() entry) per kind x network x route (stored rows at
         n = 3 and n = 4, adjoint at n = 3, fused dot at n = 14: the first size that has it) x K_p form (KSD) x
         preconditioner (None, classical Fisher -- stored rows only --, quantum Fisher)
  shots  KSD with 64 shots: two consecutive steps (the second draws at epoch 1) and the shot-epoch counter
  deal   the strided deal of two ranks (theta64, r, P, 2), r = 0, 1, stored (n = 3) and fused (n = 14): through
         elbo_and_grad_local on the ELBO side; on the KSD side the whole step (its local method is younger than the
         recorded commit: tests/test_gpu_quantum_step_bits.py interleaves the halves against the whole)
  train  3 epochs with a host read-back per epoch (theta at home on the CPU and on the GPU, Adam and SGD, a tensor TVD
         table), 6 epochs without read-backs and without a TVD (the HIP-graph replay with DeviceAdam), the same with a TVD
         table (eager training_step_async): the whole history and the final theta

Every kernel of these steps sums in a specified order and the library's only atomics are integer histogram counts, so a
case is a pure function of its seeds: the recorder runs every case twice and refuses a difference.  A case is stored as
one byte string, its pieces in the order pieces() yields them; a piece of more than KEEP_UP_TO elements is stored as the
SHA-256 of its bytes.

tests/test_gpu_quantum_step_bits.py takes its cases, pieces() and piece_bytes() from here, and this file calls only what
the trainers had before the gradient routes moved to quantum_trainer.py, so it alone can be copied onto the commit whose
bits are to be kept and run there.  The file in the repository was recorded on the last commit before that move.
Run from the repository root: python tests/golden/make_golden_quantum_step_bits.py [output.npz]"""
import contextlib
import hashlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

SEED = 7
KEEP_UP_TO = 512
CIRCUITS = {3: ("hardware_efficient", 2), 4: ("basic", 2), 14: ("hardware_efficient", 1)}    # n -> (ansatz, layers)
KINDS = ("ksd", "elbo")


def _grams(kind, route):
    """K_p forms of a case: dense (symmetric) and matrix-free for KSD -- matrix-free only at n = 14 --, none for ELBO."""
    return ("-",) if kind == "elbo" else ("kron",) if route == "fused" else ("auto", "kron")


STEPS = [("step", kind, net, route, gram, ng)
         for kind in KINDS
         for net, route in (("synthetic3", "stored"), ("synthetic4", "stored"), ("sprinkler", "stored"),
                            ("synthetic3", "adjoint"), ("sprinkler", "adjoint"), ("synthetic14", "fused"))
         for gram in _grams(kind, route)
         for ng in ((None, True, "quantum") if route == "stored" else (None, "quantum"))]
SHOTS = [("shots", "ksd", net, "stored", "auto", None) for net in ("synthetic3", "sprinkler")]
DEALS = [("deal", kind, net, route, _grams(kind, route)[-1], None)
         for kind in KINDS for net, route in (("synthetic3", "stored"), ("synthetic14", "fused"))]
TRAIN_MODES = ("sync-cpu-adam", "sync-cuda-adam", "sync-cpu-sgd", "sync-cuda-sgd",      # read-back, home of theta, optimiser
               "graph-cuda-adam", "asynctvd-cuda-adam")
TRAINS = ([("train", kind, net, mode, _grams(kind, "stored")[0], None)
           for kind in KINDS for net in ("synthetic3", "sprinkler") for mode in TRAIN_MODES]
          + [("train", kind, "sprinkler", mode, _grams(kind, "stored")[0], ng)
             for kind in KINDS for mode in ("sync-cuda-adam", "graph-cuda-adam") for ng in (True, "quantum")])
CASES = STEPS + SHOTS + DEALS + TRAINS


def case_id(case):
    return "-".join(str(v) for v in case)


def _network(name):
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
    if name == "sprinkler":
        return get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], {'W': 1}
    return synthetic_network(int(name[len("synthetic"):]), 2)


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def make(case, home="cuda:0", **kw):
    """The case's trainer, seeded and prepared for its observation -> (vi, its step method, x)."""
    import torch
    from tensornetworks_amd.elbo_vi_quantum import ELBOVariationalInference
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    _, kind, net, _, gram, ng = case
    bn, lat, obs, x = _network(net)
    n = len(lat)
    ansatz, L = CIRCUITS[n]
    if kind == "ksd":
        kw["gram_mode"] = gram
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        vi = (KSDVariationalInference if kind == "ksd" else ELBOVariationalInference)(
            bn, lat, obs, qbm_num_latent_vars=n, qbm_ansatz_layers=L, qbm_ansatz_type=ansatz, pytorch_device=home,
            natural_gradient=ng, **kw)
        vi._prepare_observation(x)
    return vi, (vi.ksd_and_grad if kind == "ksd" else vi.elbo_and_grad), x


def set_route(vi, route):
    """Points the trainer at `route` and says so: the fused dot exists from n = 14 on, below it the rows are stored."""
    import torch
    from tensornetworks_amd import backend
    bm = vi.born_machine
    P = bm.num_ansatz_params
    dev = torch.device("cuda", 0)
    fused = [backend.paramshift_dot_supported(bm.ansatz_type, bm.num_latent_vars, bm.ansatz_layers, dev, c)
             for c in (P, P - P // 2, P // 2)]
    assert all(fused) if route == "fused" else not any(fused), (route, bm.num_latent_vars, fused)
    vi.grad_engine = "adjoint" if route == "adjoint" else "paramshift"


def _step_pieces(tag, vi, out):
    loss, grad, q = out
    ps = [(f"{tag}loss", _host(loss)), (f"{tag}grad", _host(grad)), (f"{tag}q", _host(q))]
    return ps + [(f"{tag}extra{i}", _host(e)) for i, e in enumerate(vi._step_extras())]


def pieces(case):
    """[(name, array), ...] of one case, in a fixed order."""
    import torch
    from tensornetworks_amd.stein_utils import true_posterior_table
    sort, kind, net, route, _, _ = case
    if sort == "train":
        sync, home, optimiser = route.split("-")
        vi, _, x = make(case, home="cuda:0" if home == "cuda" else "cpu")
        bn, lat, _, _ = _network(net)
        tvd = sync in ("sync", "asynctvd")
        post = true_posterior_table(bn, x, lat, "cuda:0")[0] if tvd else None
        with contextlib.redirect_stdout(io.StringIO()):
            hist = vi.train(x, 3 if sync == "sync" else 6, 0.05, verbose=False, true_posterior_for_tvd=post,
                            optimizer_type=optimiser, host_sync=sync == "sync")
        return ([(f"history/{k}", np.asarray([float(v) for v in hist[k]], dtype=np.float64)) for k in sorted(hist)]
                + [("final/theta", _host(vi.born_machine.theta))])
    if sort == "shots":
        vi, step, _ = make(case, qbm_shots=64, shot_seed=5)
        set_route(vi, route)
        out = _step_pieces("first/", vi, step()) + _step_pieces("second/", vi, step())
        return out + [("shot_epoch", _host(vi.born_machine.shot_epoch(torch.device("cuda", 0))))]
    vi, step, _ = make(case)
    set_route(vi, route)
    if sort == "deal" and kind == "elbo":
        theta64 = vi.born_machine.theta.detach().double().contiguous()
        P = theta64.numel()
        return [p for r in (0, 1) for p in _step_pieces(f"rank{r}/", vi, vi.elbo_and_grad_local(theta64, r, P, 2))]
    return _step_pieces("", vi, step())


def piece_bytes(a):
    raw = np.ascontiguousarray(a).tobytes()
    return hashlib.sha256(raw).digest() if a.size > KEEP_UP_TO else raw


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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "quantum_step_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")
