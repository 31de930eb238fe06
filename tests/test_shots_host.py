"""Host side of finite-shot training: the NumPy mirror of the sampler's Philox4x32-10 against the Random123 known-answer
vectors and rocRAND's engine, the mirror's multinomial invariants, and the argument checks of the shots extras
(QuantumBornMachine(shots=...), KSDVariationalInference(qbm_shots=...)).  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import shots_mirror as sm

# Random123 kat_vectors, philox4x32_10: (key, counter) -> output
KAT = [((0x00000000, 0x00000000), (0x00000000, 0x00000000, 0x00000000, 0x00000000),
        (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff),
        (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_mirror_known_answers():
    for (k0, k1), c, want in KAT:
        got = sm.philox4x32_10(*c, k0, k1)
        assert tuple(int(w) for w in got) == want


_DRIVER = r"""
#include <rocrand/rocrand_philox4x32_10.h>
#include <cstdio>
#include <cstdlib>
struct Engine : rocrand_device::philox4x32_10_engine { using philox4x32_10_engine::ten_rounds; };
int main(int argc, char** argv) {   // groups of six hex words: key0 key1 ctr0 ctr1 ctr2 ctr3
  Engine e;
  for (int i = 1; i + 5 < argc; i += 6) {
    uint2 k{(unsigned)strtoul(argv[i], 0, 16), (unsigned)strtoul(argv[i + 1], 0, 16)};
    uint4 c{(unsigned)strtoul(argv[i + 2], 0, 16), (unsigned)strtoul(argv[i + 3], 0, 16),
            (unsigned)strtoul(argv[i + 4], 0, 16), (unsigned)strtoul(argv[i + 5], 0, 16)};
    uint4 r = e.ten_rounds(c, k);
    printf("%08x %08x %08x %08x\n", r.x, r.y, r.z, r.w);
  }
  return 0;
}
"""


def test_philox_mirror_equals_rocrand_engine(tmp_path):
    """The round function and constants against rocRAND's host-callable Philox4x32-10 (header only, compiled into a tiny
    host driver), on counters shaped like the sampler's (pair, level/block, circuit id, epoch) and random ones."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc")
    if not hipcc and os.environ.get("ROCM_PATH"):
        hipcc = os.path.join(os.environ["ROCM_PATH"], "bin", "hipcc")
    if not hipcc or not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))      # <ROCm root>/bin/hipcc
    header = os.path.join(rocm, "include", "rocrand", "rocrand_philox4x32_10.h")
    if not os.path.exists(header):
        pytest.skip("the rocRAND header is not installed")
    src = tmp_path / "philox.cpp"
    src.write_text(_DRIVER)
    exe = str(tmp_path / "philox")
    b = subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", str(src), "-o", exe], capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    rng = np.random.default_rng(5)
    cases = [tuple(int(v) for v in rng.integers(0, 1 << 32, 6, dtype=np.uint64)) for _ in range(40)]
    cases += [(0x12345678, 0x9abcdef0, m, (1 << 24) | 3, 2 * p + 2, 7) for m, p in ((0, 0), (1, 5), (65535, 40))]
    args = [f"{v:x}" for c in cases for v in c]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    for (k0, k1, c0, c1, c2, c3), line in zip(cases, lines):
        got = sm.philox4x32_10(c0, c1, c2, c3, k0, k1)
        assert " ".join(f"{int(w):08x}" for w in got) == line


def _dyadic(rng, N, zeros=0.3):
    a = rng.integers(0, 64, N).astype(np.int64)
    a[rng.random(N) < zeros] = 0
    a[rng.integers(N)] += 1
    K = 1 << int(np.ceil(np.log2(a.sum())))
    a[np.nonzero(a)[0][-1]] += K - a.sum()
    return a / K


@pytest.mark.parametrize("n", [1, 3, 13])
def test_mirror_invariants(n):
    rng = np.random.default_rng(n)
    p = np.stack([_dyadic(rng, 1 << n) for _ in range(3)])
    c = sm.histogram(p, 5000, 99, 4)
    assert (c.sum(axis=1) == 5000).all()
    assert (c[p == 0] == 0).all()
    assert np.array_equal(c, sm.histogram(p, 5000, 99, 4))
    assert not np.array_equal(c, sm.histogram(p, 5000, 99, 5))
    assert not np.array_equal(c[1], c[2]) or n == 1        # rows have their own circuit ids


def test_mirror_uniforms_are_53_bit_and_paired():
    u = sm.uniforms(7, 0, 0, 0, 0, 11)
    assert u.shape == (11,) and (u >= 0).all() and (u < 1).all()
    assert np.all(u * 2.0 ** 53 == np.floor(u * 2.0 ** 53))
    assert np.array_equal(u[:10], sm.uniforms(7, 0, 0, 0, 0, 10))


def test_born_machine_shots_arguments():
    from tensornetworks_amd.quantum_born_machine import QuantumBornMachine
    for bad in (0, -3, 1.5, 1000.0, True, "100", 1 << 31):
        with pytest.raises(ValueError):
            QuantumBornMachine(3, 2, shots=bad)
    torch.manual_seed(3)
    exact = QuantumBornMachine(3, 2)
    after_exact = torch.rand(1)
    torch.manual_seed(3)
    qbm = QuantumBornMachine(3, 2, shots=1000)
    assert qbm.dev.shots == 1000 and exact.dev.shots is None and exact.shot_seed is None
    assert torch.equal(qbm.theta, exact.theta)           # the seed is drawn after theta's initialisation
    assert not torch.equal(torch.rand(1), after_exact)   # ... and only with shots: one draw more
    torch.manual_seed(3)
    assert QuantumBornMachine(3, 2, shots=1000).shot_seed == qbm.shot_seed
    assert QuantumBornMachine(3, 2, shots=10, shot_seed=42).shot_seed == 42


def test_trainer_shots_arguments():
    from tensornetworks_amd.bayesian_network import get_sprinkler_network
    from tensornetworks_amd.ksd_vi_quantum import KSDVariationalInference
    bn = get_sprinkler_network(False)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            KSDVariationalInference(bn, ["C", "S", "R"], ["W"], 3, 2, qbm_shots=bad)
    vi = KSDVariationalInference(bn, ["C", "S", "R"], ["W"], 3, 2, qbm_shots=256, shot_seed=5)
    assert vi.born_machine.shots == 256 and vi.born_machine.dev.shots == 256 and vi.born_machine.shot_seed == 5
    assert KSDVariationalInference(bn, ["C", "S", "R"], ["W"], 3, 2).born_machine.dev.shots is None
