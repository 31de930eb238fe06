"""csrc/reduce_dev.hpp on the host: chunk_geom, the one chunk geometry of the kernels' partial sums, compiled into a host driver
(the kernels' own text, as test_shots_host.py runs shots_dev.hpp) and compared, exactly, with the restatements the
extended-precision bounds are built on: classical_hp.bt_geom (table kernels and the ELBO: chunks of a multiple of 4),
classical_hp.rf_geom (REINFORCE: outcome chunks and sample chunks) and the formula of test_gpu_mps_kernel.constants (the
elementwise passes of the enumerated MPS); and bond_dp, the padded bond dimension.  No GPU needed."""
import os
import subprocess

import pytest

import classical_hp as chp
from test_shots_host import _hipcc

_DRIVER = r"""
#include "reduce_dev.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {   // per_wg max_wg align, then counts: one line "chunk G" per count; no counts: bond_dp(1 .. 32)
  if (argc < 4) {
    for (int D = 1; D <= 32; ++D) printf("%d\n", bornvi::bond_dp(D));
    return 0;
  }
  const long long per_wg = atoll(argv[1]), max_wg = atoll(argv[2]);
  const int align = atoi(argv[3]);
  char line[64];
  while (fgets(line, sizeof line, stdin)) {
    const bornvi::ChunkGeom g = bornvi::chunk_geom(atoll(line), per_wg, max_wg, align);
    printf("%lld %d\n", g.chunk, g.G);
  }
  return 0;
}
"""

POWERS = [1 << k for k in range(31)]
BATCHES = list(range(1, 5001)) + [1 << 24]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed")
    tmp = tmp_path_factory.mktemp("reduce_host")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensornetworks_amd", "csrc")
    src = tmp / "geom.cpp"
    src.write_text(_DRIVER)
    exe = str(tmp / "geom")
    b = subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + csrc, str(src), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]

    def run(per_wg, max_wg, align, counts):
        r = subprocess.run([exe, str(per_wg), str(max_wg), str(align)], input="".join(f"{c}\n" for c in counts),
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
        assert len(got) == len(counts)
        return got
    run.exe = exe
    return run


def test_chunk_geom_is_the_table_kernels_geometry(driver):
    assert driver(chp.BT_PER_WG, chp.MAX_WG, 4, POWERS) == [chp.bt_geom(N) for N in POWERS]


@pytest.mark.parametrize("per_wg", [chp.RF_SAMPLES_PER_WG, chp.RF_OUTCOMES_PER_WG])
def test_chunk_geom_is_the_reinforce_geometry(driver, per_wg):
    counts = POWERS + BATCHES
    assert driver(per_wg, chp.MAX_WG, 1, counts) == [chp.rf_geom(c, per_wg) for c in counts]


def test_chunk_geom_is_the_enumerated_mps_geometry(driver):
    def mps_q(N):                      # test_gpu_mps_kernel.constants: Gq workgroups of ceil(N / Gq) entries
        Gq = min(1024, -(-N // 4096))
        chunk = -(-N // Gq)
        return chunk, -(-N // chunk)
    got = driver(4096, 1024, 1, POWERS)
    assert got == [mps_q(N) for N in POWERS]
    assert all(G == min(1024, -(-N // 4096)) for N, (_, G) in zip(POWERS, got))       # (no workgroup is lost to the rounding)


def test_chunk_geom_covers_the_count(driver):
    for per_wg, align in ((4096, 4), (4096, 1), (1024, 1)):
        counts = POWERS + BATCHES
        for c, (chunk, G) in zip(counts, driver(per_wg, 1024, align, counts)):
            assert 1 <= G <= 1024 and chunk % align == 0 and (G - 1) * chunk < c <= G * chunk, (per_wg, align, c, chunk, G)


def test_bond_dp(driver):
    r = subprocess.run([driver.exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    want = [next(p for p in (2, 4, 8, 16, 32) if p >= D) for D in range(1, 33)]
    assert [int(v) for v in r.stdout.split()] == want
