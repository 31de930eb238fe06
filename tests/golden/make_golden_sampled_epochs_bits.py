"""Records tests/golden/sampled_epochs_parent_bits.npz: five epochs of each sampled MPS trainer (ELBO and KSD) on an MI355X
through their public surface, bit for bit -- the losses, the gradient norms, the final cores and the last epoch's outcome
indices -- on the last commit before the trainers gained their `natural_gradient` keyword.  Two cases per trainer:

  sprinkler     W = 1, n = 3, D = 2, B = 1024, Adam with the cosine schedule
  synthetic12   synthetic_network(12, 0), D = 3, B = 257 (no multiple of the 64-sample tile), SGD

Every kernel of an epoch sums in a specified order, so a case is a pure function of its seeds: the recorder runs every case
twice and refuses a difference.  tests/test_gpu_sampled_natgrad_trainer.py takes `CASES` and `run` from here and passes
natural_gradient=None; this file itself uses only what the trainers had before, so it alone can be copied onto the commit
whose bits are to be kept and run there.
Run from the repository root: python tests/golden/make_golden_sampled_epochs_bits.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

EPOCHS = 5
CASES = [(kind, net) for kind in ("elbo", "ksd") for net in ("sprinkler", "synthetic12")]


def case_id(case):
    return "-".join(case)


def run(case, **trainer_kw):
    """{piece name: array} of one case; trainer_kw goes to the trainer's constructor."""
    import torch
    from tensornetworks_amd import SampledELBOVariationalInference, SampledKSDVariationalInference
    from tensornetworks_amd.bayesian_network import get_sprinkler_network, synthetic_network
    kind, net = case
    if net == "sprinkler":
        bn, lat, obs, x = get_sprinkler_network(False), ['C', 'S', 'R'], ['W'], {'W': 1}
        cfg, opt, lr = {'bond_dim': 2, 'num_samples': 1024, 'seed': 5}, "adam", 0.05
    else:
        bn, lat, obs, x = synthetic_network(12, 0)
        cfg, opt, lr = {'bond_dim': 3, 'num_samples': 257, 'seed': 4}, "sgd", 0.02
    torch.manual_seed(11)
    cls = SampledELBOVariationalInference if kind == "elbo" else SampledKSDVariationalInference
    vi = cls(bn, lat, obs, cfg, device='cuda', **trainer_kw)
    hist = vi.train(x, EPOCHS, lr, verbose=False, optimizer_type=opt)
    out = {f"history/{k}": np.asarray([float(v) for v in hist[k]], dtype=np.float64) for k in sorted(hist)}
    out["final/cores"] = np.ascontiguousarray(vi.born_machine.cores.detach().cpu().numpy())
    out["last/idx"] = np.ascontiguousarray(vi.last_idx.cpu().numpy())
    return out


def same(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    out = {}
    for case in CASES:
        r = run(case)
        assert same(r, run(case)), f"{case_id(case)}: two runs differ"
        for k, v in r.items():
            out[f"{case_id(case)}/{k}"] = v
        print(f"{case_id(case)}: loss {r['history/' + ('loss_elbo' if case[0] == 'elbo' else 'loss_ksd2')]}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sampled_epochs_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
