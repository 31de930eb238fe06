"""Records tests/golden/family_init_seed7.npz: the starting parameters of the three classical Born-machine families after
torch.manual_seed(7), for n = 3 -- the table with every init_method, one MLP with the default hidden sizes, and both MPS
machines with D in {1, 4} and every init_method.  tests/test_family_surface_host.py takes its cases and parameters() from
here, so this file alone can be copied onto the commit whose draws are to be kept and run there.  The file in the
repository was recorded on the last commit before the families moved onto born_machine_base.py.  Needs no GPU.  Run from
the repository root:  python tests/golden/make_golden_family_init.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

SEED, N = 7, 3
CASES = [("table", m) for m in ("zero", "small_random", "uniform", "random")] + [("mlp", "default")] + \
    [(fam, f"{m}_D{D}") for fam in ("mps", "mps_sampled") for D in (1, 4) for m in ("small_random", "zero", "random")]


def parameters(family, variant):
    """{key: array} of the machine's named parameters, constructed right after torch.manual_seed(SEED)."""
    import torch
    from tensornetworks_amd.born_machine_classical_sim import ClassicalBornMachine
    from tensornetworks_amd.born_machine_mps import MPSBornMachine
    from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine
    torch.manual_seed(SEED)
    if family == "table":
        bm = ClassicalBornMachine(N, init_method=variant)
    elif family == "mlp":
        bm = ClassicalBornMachine(N, conditioning_dim=1)
    else:
        method, D = variant.rsplit("_D", 1)
        bm = (MPSBornMachine if family == "mps" else SampledMPSBornMachine)(N, bond_dim=int(D), init_method=method)
    return {f"{family}/{variant}/{name}": p.detach().numpy().copy() for name, p in bm.named_parameters()}


if __name__ == "__main__":
    out = {}
    for family, variant in CASES:
        out.update(parameters(family, variant))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "family_init_seed7.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
