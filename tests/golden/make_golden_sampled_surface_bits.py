"""Records tests/golden/sampled_surface_parent_bits.npz: what the three sampled MPS families (real, complex cores, locally
purified) compute on an MI355X through their public surface, bit for bit, on the last commit before they moved onto one
shared surface.

Per family at (n, D, B) = (3, 2, 65) and (12, 5, 257) -- an odd bond padded to 8, a partial last tile at both the 64-sample
and the 16-sample tiling; purified cores with m = 3, so the sampler's cumulative loop over mu runs -- with cores from
init_method='random' under torch.manual_seed(11) and the machine's seed 11: sample_indices(B) and sample_indices(B, seed=9,
epoch=2); two successive sample(B) (the counter of draws); score_vjp(idx, w) for a fixed Gaussian w; log_prob(idx);
probabilities64(), and for the real family the gradient of probabilities64().square().sum() in the cores.
Per `cores` kind: three epochs of SampledELBOVariationalInference on the sprinkler network (W = 1, bond_dim 2, num_samples
65, Adam): history, final cores, last_idx; for 'real' the same with natural_gradient='site'.

A case is stored as one byte string, its pieces in the order pieces() yields them; a piece of more than KEEP_UP_TO elements
is stored as the SHA-256 of its bytes.  Every kernel sums in a specified order, so a case is a pure function of its seeds:
the recorder runs every case twice and refuses a difference.  tests/test_gpu_sampled_surface_bits.py takes its cases,
pieces() and piece_bytes() from here; this file uses only public names, so it alone can be copied onto the commit whose
bits are to be kept and run there.
Run from the repository root: python tests/golden/make_golden_sampled_surface_bits.py [output.npz]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

SEED = 11
KEEP_UP_TO = 512
EPOCHS = 3
FAMILIES = ("real", "complex", "purified")
MACHINES = [(family, n, D, B) for family in FAMILIES for n, D, B in ((3, 2, 65), (12, 5, 257))]
TRAINERS = [("train", kind, None) for kind in FAMILIES] + [("train", "real", "site")]


def case_id(case):
    return "-".join(str(v) for v in case)


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _machine_pieces(family, n, D, B):
    import torch
    from tensornetworks_amd import ComplexSampledMPSBornMachine, PurifiedSampledMPSBornMachine, SampledMPSBornMachine
    torch.manual_seed(SEED)
    if family == "purified":
        bm = PurifiedSampledMPSBornMachine(n, bond_dim=D, purification_dim=3, init_method='random', seed=SEED)
    else:
        cls = ComplexSampledMPSBornMachine if family == "complex" else SampledMPSBornMachine
        bm = cls(n, bond_dim=D, init_method='random', seed=SEED)
    bm = bm.to('cuda')
    idx, logq = bm.sample_indices(B)
    out = [("sample_indices/idx", _host(idx)), ("sample_indices/logq", _host(logq))]
    idx2, logq2 = bm.sample_indices(B, seed=9, epoch=2)
    out += [("sample_indices92/idx", _host(idx2)), ("sample_indices92/logq", _host(logq2))]
    out += [("sample/0", _host(bm.sample(B))), ("sample/1", _host(bm.sample(B)))]
    w = torch.randn(B, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    grad, logq_s = bm.score_vjp(idx, w)
    out += [("score_vjp/grad", _host(grad)), ("score_vjp/logq", _host(logq_s)), ("log_prob", _host(bm.log_prob(idx)))]
    q = bm.probabilities64()
    out.append(("probabilities64", _host(q)))
    if family == "real":
        q.square().sum().backward()
        out.append(("probabilities64/grad", _host(bm.cores.grad)))
    return out


def _trainer_pieces(kind, natural_gradient):
    import torch
    from tensornetworks_amd import SampledELBOVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    torch.manual_seed(SEED)
    kw = {} if natural_gradient is None else {"natural_gradient": natural_gradient}
    vi = SampledELBOVariationalInference(get_sprinkler_network(False), ['C', 'S', 'R'], ['W'],
                                         {'bond_dim': 2, 'num_samples': 65, 'seed': 5, 'cores': kind}, device='cuda', **kw)
    hist = vi.train({'W': 1}, EPOCHS, 0.05, verbose=False, optimizer_type="adam")
    out = [(f"history/{k}", np.asarray([float(v) for v in hist[k]], dtype=np.float64)) for k in sorted(hist)]
    return out + [("final/cores", _host(vi.born_machine.cores)), ("last/idx", _host(vi.last_idx))]


def pieces(case):
    """[(name, array), ...] of one case, in a fixed order."""
    if case[0] == "train":
        return _trainer_pieces(case[1], case[2])
    return _machine_pieces(*case)


def piece_bytes(a):
    raw = np.ascontiguousarray(a).tobytes()
    return hashlib.sha256(raw).digest() if a.size > KEEP_UP_TO else raw


def blob(ps):
    return np.frombuffer(b"".join(piece_bytes(a) for _, a in ps), dtype=np.uint8)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    out = {}
    for case in MACHINES + TRAINERS:
        b = blob(pieces(case))
        assert np.array_equal(b, blob(pieces(case))), f"{case_id(case)}: two runs differ"
        out[case_id(case)] = b
        print(f"{case_id(case)}: {b.size} bytes, sha256 {hashlib.sha256(b.tobytes()).hexdigest()[:16]}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sampled_surface_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")
