"""Records tests/golden/sampled_init_parent_bits.npz: the parameters the three sampled MPS families (real, complex cores,
locally purified) construct on the host, bit for bit, on the last commit before they moved onto one shared surface.  Per
family and init_method under torch.manual_seed(11), at n = 5, D = 3 (purified: m = 3): the cores of the plain constructor;
from_real of the real machine of that seed (complex and purified; purified also at purification_dim = 2); from_complex of
the complex machine of that seed (purified); from_statevector of a fixed vector of 2^4 complex amplitudes at bond_dim = 2,
cutoff = 0.0, cores and `discarded` (complex).  No library call is made: this runs on any machine.

The order and shapes of the torch.randn draws in a constructor are part of what is kept: a given seed gives the same cores.
The recorder runs every case twice and refuses a difference.  tests/test_sampled_surface_host.py takes CASES and run() from
here; this file uses only public names, so it alone can be copied onto the commit whose bits are to be kept and run there.
Run from the repository root: python tests/golden/make_golden_sampled_init_bits.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)),) if p not in sys.path]

SEED, N, D, M = 11, 5, 3, 3
CASES = [(family, init) for family in ("real", "complex", "purified") for init in ("zero", "small_random", "random")]


def case_id(case):
    return "-".join(case)


def statevector():
    """A fixed vector of 2^4 complex amplitudes (no generator involved)."""
    k = np.arange(16, dtype=np.float64)
    return np.cos(0.7 * k + 0.1) + 1j * np.sin(1.3 * k - 0.4)


def _host(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def run(case):
    """{piece name: array} of one case."""
    import torch
    from tensornetworks_amd import ComplexSampledMPSBornMachine, PurifiedSampledMPSBornMachine, SampledMPSBornMachine
    family, init = case

    def seeded(cls, **kw):
        torch.manual_seed(SEED)
        return cls(N, bond_dim=D, init_method=init, seed=3, **kw)
    if family == "real":
        return {"cores": _host(seeded(SampledMPSBornMachine).cores)}
    if family == "complex":
        machine, discarded = ComplexSampledMPSBornMachine.from_statevector(torch.from_numpy(statevector()), 2, cutoff=0.0)
        return {"cores": _host(seeded(ComplexSampledMPSBornMachine).cores),
                "from_real": _host(ComplexSampledMPSBornMachine.from_real(seeded(SampledMPSBornMachine)).cores),
                "from_statevector/cores": _host(machine.cores), "from_statevector/discarded": _host(discarded)}
    cls = PurifiedSampledMPSBornMachine
    return {"cores": _host(seeded(cls, purification_dim=M).cores),
            "from_real": _host(cls.from_real(seeded(SampledMPSBornMachine)).cores),
            "from_real/m2": _host(cls.from_real(seeded(SampledMPSBornMachine), purification_dim=2).cores),
            "from_complex": _host(cls.from_complex(seeded(ComplexSampledMPSBornMachine)).cores)}


def same(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                                          a[k].tobytes() == b[k].tobytes() for k in a)


if __name__ == "__main__":
    out = {}
    for case in CASES:
        r = run(case)
        assert same(r, run(case)), f"{case_id(case)}: two runs differ"
        for k, v in r.items():
            out[f"{case_id(case)}/{k}"] = v
        print(f"{case_id(case)}: {sorted((k, v.shape) for k, v in r.items())}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sampled_init_parent_bits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
