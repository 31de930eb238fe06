"""Records tests/golden/family_surface_parent_bits.npz: what the classical trainers compute on an MI355X through their
public surface, bit for bit, at the smallest sizes at which the host plumbing between trainer, machine and kernels can
go wrong.  Per enumerated case (network x parameters' device x machine x trainer x entropy weight): one loss_and_grads
call followed by apply_grads (loss, entropy, q, every parameter's .grad), then a 5-epoch train() (the whole history and
the final parameters).  Per sampled case ((n, D, B) x device): loss_and_grad(0) and loss_and_grad(1) (all four outputs),
then a 3-epoch train() (history, final cores).  A case is stored as one byte string, its pieces in the order pieces()
yields them; a piece of more than KEEP_UP_TO elements (the MLP's weights) is stored as the SHA-256 of its bytes.

tests/test_gpu_family_surface_bits.py takes its cases, pieces() and blob() from here, so this file alone can be copied
onto the commit whose bits are to be kept and run there.  The file in the repository was recorded on the last commit
before the families moved onto born_machine_base.py.  Run from the repository root:
python tests/golden/make_golden_family_surface_bits.py [output.npz]"""
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
MACHINES = {"softmax": {'use_logits': True}, "absnorm": {'use_logits': False},
            "mlp": {'use_logits': True, 'conditioning_dim': 1},
            "mps1": {'family': 'mps', 'bond_dim': 1}, "mps2": {'family': 'mps', 'bond_dim': 2},
            "mps4": {'family': 'mps', 'bond_dim': 4}}
ENUMERATED = [(net, home, machine, trainer, lam) for net in ("sprinkler", "synthetic6") for home in ("cpu", "cuda")
              for machine in MACHINES for trainer in ("ksd", "elbo") for lam in (0.0, 0.01)]
SAMPLED = [(n, D, B, home) for n, D, B in ((6, 2, 64), (40, 4, 256)) for home in ("cpu", "cuda")]


def case_id(case):
    return "-".join(str(v) for v in case)


def _network(name):
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
    if name == "sprinkler":
        return get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], {'W': 1}
    return synthetic_network(int(name[len("synthetic"):]), 0)


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _history(hist):
    return [(f"history/{k}", np.asarray(hist[k], dtype=np.float64)) for k in sorted(hist)]


def pieces(case):
    """[(name, array), ...] of one case, in a fixed order."""
    import torch
    from tensornetworks_amd.stein_utils import true_posterior_table
    quiet = contextlib.redirect_stdout(io.StringIO())
    torch.manual_seed(SEED)
    if len(case) == 4:
        from tensornetworks_amd.elbo_vi_sampled import SampledELBOVariationalInference
        n, D, B, home = case
        bn, lat, obs, x = _network(f"synthetic{n}")
        vi = SampledELBOVariationalInference(bn, lat, obs, {'bond_dim': D, 'num_samples': B, 'seed': 5}, device=home)
        vi._prepare_observation(x)
        out = []
        for epoch in (0, 1):
            out += [(f"epoch{epoch}/{name}", _host(t)) for name, t in zip(("loss", "grad", "logq_mean", "status"),
                                                                           vi.loss_and_grad(epoch))]
        post = true_posterior_table(bn, x, lat, home)[0] if n <= 26 else None
        hist = vi.train(x, 3, 0.05, verbose=False, true_posterior_for_tvd=post)
        return out + _history(hist) + [("final/cores", _host(vi.born_machine.cores))]
    from tensornetworks_amd.elbo_vi import ELBOVariationalInference
    from tensornetworks_amd.ksd_vi import KSDVariationalInference
    net, home, machine, trainer, lam = case
    bn, lat, obs, x = _network(net)
    cls = KSDVariationalInference if trainer == "ksd" else ELBOVariationalInference
    with quiet:
        vi = cls(bn, lat, obs, dict(MACHINES[machine]), device=home)
        vi._prepare_observation(x)
    bm = vi.born_machine
    xc = torch.tensor([x[o] for o in obs], dtype=torch.float32, device=home) if bm.conditioning_dim > 0 else None
    loss, entropy, q, grads = vi.loss_and_grads(xc, lam)
    vi.apply_grads(grads)
    out = [("loss", _host(loss)), ("entropy", _host(entropy)), ("q", _host(q))]
    out += [(f"grad/{name}", _host(p.grad)) for name, p in bm.named_parameters()]
    post = true_posterior_table(bn, x, lat, home)[0]
    with quiet:
        hist = vi.train(x, 5, 0.05, verbose=False, true_posterior_for_tvd=post, entropy_weight=lam)
    return out + _history(hist) + [(f"final/{name}", _host(p)) for name, p in bm.named_parameters()]


def piece_bytes(a):
    raw = np.ascontiguousarray(a).tobytes()
    return hashlib.sha256(raw).digest() if a.size > KEEP_UP_TO else raw


def blob(ps):
    return np.frombuffer(b"".join(piece_bytes(a) for _, a in ps), dtype=np.uint8)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    out = {}
    for case in ENUMERATED + SAMPLED:
        b = blob(pieces(case))
        assert np.array_equal(b, blob(pieces(case))), f"{case_id(case)}: two runs differ"
        out[case_id(case)] = b
        print(f"{case_id(case)}: {b.size} bytes, sha256 {hashlib.sha256(b.tobytes()).hexdigest()[:16]}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "family_surface_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")
