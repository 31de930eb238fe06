"""Host side of finite-shot training: the NumPy mirror of the sampler's Philox4x32-10 against the Random123 known-answer
vectors and rocRAND's engine, the mirror's multinomial invariants, and the argument checks of the shots extras
(QuantumBornMachine(shots=...), KSDVariationalInference(qbm_shots=...)).  The sampler on rows that are not dyadic: the
device-order mirrors (device_cdf, device_mass) against extended precision with derived constants, the thread-boundary hazard
of the scan and rule R on it, the kernel's own pick function (csrc/shots_dev.hpp) run by a host driver, and the inputs of
the real-row GPU tests shown free of undecided draws.  No GPU needed."""
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


_dyadic = sm.dyadic_row


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


# ---- rows that are not dyadic ---------------------------------------------------------------------------------------------
# Error constants, in units of 2^-52 of the block total.  All entries are >= 0, so a sum in which every input passes through
# at most d additions errs by at most d roundings of at most 2^-53 of the total each; every rounding is counted as a whole
# unit (2^-52), which also covers the second-order terms.
#   draw kernel's cdf: 7 adds inside a thread (the first of its 8 adds 0), 9 levels of the scan, 1 add of the prefix;
#   mass kernel:       16 adds inside a thread, 6 butterfly steps, 4 adds of the wave totals.
C_SCAN = 7 + 9 + 1
C_MASS = 16 + 6 + 4
C_REF = 2.0 ** -5          # the extended-precision reference itself: at most 128 additions of 2^-64 each (see _cdf_ld)
MAX_LEVEL = 2              # n <= 30: 2^30 -> 2^18 -> 2^6


def boundary_shift(level):
    """Bound, in u, on the distance between the kernel's decision boundary cdf~[i] = fl(u total~) and the exact one
    u = cdf[i] / total on `level`: the level's values carry `level` mass sums (C_MASS each, relative), both cdf~[i] and total~
    carry C_SCAN more, and the product rounds once."""
    c = C_SCAN + level * C_MASS
    return (2 * c + 1) * 2.0 ** -52


def _cdf_ld(v):
    """Inclusive prefix sums in extended precision, two levels of 64: no entry passes through more than 128 additions."""
    r = np.cumsum(np.asarray(v, dtype=sm.LD).reshape(-1, 64), axis=1)
    r[1:] += np.cumsum(r[:-1, -1])[:, None]
    return r.reshape(-1)


def _hazard_rows():
    """40 rows of 4096 entries: r^4, half of them zeroed, normalised."""
    rng = np.random.default_rng(0)
    rows = []
    for _ in range(40):
        x = rng.random(sm.BLOCK) ** 4
        x[rng.random(sm.BLOCK) < 0.5] = 0.0
        rows.append(x / x.sum())
    return np.stack(rows)


def _zero_mass_row():
    """n = 20: 256 block masses, half of them zero, the others a handful of positive entries each."""
    rng = np.random.default_rng(20)
    row = np.zeros((256, sm.BLOCK))
    for b in np.nonzero(rng.random(256) < 0.5)[0]:
        row[b, rng.integers(0, sm.BLOCK, 5)] = rng.random(5) ** 4
    return (row / row.sum()).reshape(-1)


def _rising_zeros(vals, cdf):
    """Zero entries whose cdf exceeds their predecessor's, and for each every float64 x in [cdf[i-1], cdf[i])."""
    out = []
    for i in np.nonzero((vals[1:] == 0) & (cdf[1:] > cdf[:-1]))[0] + 1:
        xs, x = [], cdf[i - 1]
        while x < cdf[i]:
            xs.append(x)
            x = np.nextafter(x, np.inf)
        out.append((int(i), xs))
    return out


@pytest.mark.skipif(not sm.hp.HAVE_LONGDOUBLE, reason="np.longdouble has no 64-bit mantissa on this machine")
def test_device_order_mirrors_within_derived_constants():
    rng = np.random.default_rng(11)
    blocks = np.concatenate([_hazard_rows(), np.stack([sm.real_row(k, 12, rng) for k in "abc" for _ in range(4)]),
                             sm.dyadic_row(rng, sm.BLOCK)[None]])
    worst_cdf = worst_mass = 0.0
    for v in blocks:
        ref = _cdf_ld(v)
        unit = ref[-1] * sm.LD(2.0 ** -52)
        worst_cdf = max(worst_cdf, float((np.abs(sm.device_cdf(v).astype(sm.LD) - ref) / unit).max()))
        worst_mass = max(worst_mass, float(abs(sm.LD(sm.device_mass(v)) - v.astype(sm.LD).sum()) / unit))
    print(f"device_cdf: worst {worst_cdf:.3f} units of 2^-52 total, C_SCAN = {C_SCAN};  device_mass: worst {worst_mass:.3f}, "
          f"C_MASS = {C_MASS};  boundary shift by level {[boundary_shift(l) for l in range(MAX_LEVEL + 1)]}, margin {sm.MARGIN}")
    assert worst_cdf <= C_SCAN + C_REF and worst_mass <= C_MASS + C_REF
    assert worst_cdf > 0 and worst_mass > 0                      # the rows do round
    for short in (2, 8, 256):                                    # blocks shorter than 4096: the same order on a prefix
        v = blocks[0, :short]
        assert np.abs(sm.device_cdf(v).astype(sm.LD) - np.cumsum(v.astype(sm.LD))).max() <= C_SCAN * 2.0 ** -52 * v.sum()
    assert np.array_equal(sm.device_cdf(blocks[-1]), np.cumsum(blocks[-1]))      # dyadic: exact in any order
    assert np.array_equal(sm.device_cdf(blocks[:3]), np.stack([sm.device_cdf(b) for b in blocks[:3]]))
    for level in range(MAX_LEVEL + 1):
        assert boundary_shift(level) < sm.MARGIN / 16            # the undecided margin covers every order of summation


def test_rule_r_on_the_scan_hazard():
    """At a thread boundary of the scan a zero entry's cdf can exceed its predecessor's.  "First i with cdf[i] > x" alone
    (the rule before R) returns that zero entry there: entry 280 of the first row is the known witness."""
    rows = _hazard_rows()
    total = total_bare = 0
    for r, v in enumerate(rows):
        cdf = sm.device_cdf(v)
        hazards = _rising_zeros(v, cdf)
        assert hazards, r                                        # every row has some: the test cannot pass vacuously
        total += len(hazards)
        bare = 0
        for i, xs in hazards:
            assert 1 <= len(xs) <= 4 and v[i] == 0.0                  # a rise of a few ulps at the most
            lo0 = sm.first_greater(cdf, xs)                      # what the bare search returns: mostly i itself (where the
            bare += int((v[lo0] == 0).any())                     # cdf also falls back by an ulp further on, a later index)
            got = sm.pick(cdf, v > 0, xs)
            assert (v[got] > 0).all(), (r, i)
            for g, l in zip(got, lo0):                           # rule R, restated entry by entry
                assert g >= l and not (v[l:g] > 0).any(), (r, i)
        assert bare > 0, r                                       # the rule before R draws a zero entry on every row
        total_bare += bare
        if r == 0:
            assert 280 in [i for i, _ in hazards] and v[280] == 0.0
            assert sm.first_greater(cdf, cdf[279])[0] == 280 and v[sm.pick(cdf, v > 0, cdf[279])[0]] > 0
    assert total == 2406
    print("rising zero entries:", total, "of which the bare search returns a zero entry for", total_bare)


def test_rule_r_loses_no_draw_to_a_zero_mass_block():
    row = _zero_mass_row()
    masses = sm.device_mass(row.reshape(-1, sm.BLOCK))
    cdf = sm.device_cdf(masses)
    hazards = _rising_zeros(masses, cdf)
    assert hazards
    xs = np.array([x for _, xs in hazards for x in xs])
    assert (masses[sm.first_greater(cdf, xs)] == 0).any()       # the bare search hands such draws to an all-zero block
    assert (masses[sm.pick(cdf, masses > 0, xs)] > 0).all()

    def x_of(level, block, m, total):
        return np.resize(xs, m) if level == 1 else (np.arange(m) + 0.5) / m * total
    S = 4 * len(xs)
    counts = sm.row_counts(row, S, 1, 0, 0, order="device", x_of=x_of)
    assert counts.sum() == S and (counts[row == 0] == 0).all()


_PICK_DRIVER = r"""
#include "shots_dev.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {   // records of: int32 blk, int32 nx, blk doubles cdf, 129 mask words, nx doubles x
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f) return 2;
  int hdr[2];
  while (fread(hdr, sizeof(int), 2, f) == 2) {
    const int blk = hdr[0], nx = hdr[1];
    if (blk < 1 || blk > bornvi::SHOTS_BLOCK || nx < 0) return 3;
    std::vector<double> cdf(blk), x(nx);
    uint32_t pos[bornvi::SHOTS_MASK_WORDS];
    if (fread(cdf.data(), sizeof(double), blk, f) != (size_t)blk) return 4;
    if (fread(pos, sizeof(uint32_t), bornvi::SHOTS_MASK_WORDS, f) != (size_t)bornvi::SHOTS_MASK_WORDS) return 4;
    if (fread(x.data(), sizeof(double), nx, f) != (size_t)nx) return 4;
    int last = -1;
    for (int i = 0; i < blk; ++i)
      if ((pos[i >> 5] >> (i & 31)) & 1u) last = i;
    int k = 0;
    for (; k + 1 < nx; k += 2) {                      // pairs, as the kernel calls it; an odd tail alone
      const double xs[2] = {x[k], x[k + 1]};
      int out[2];
      bornvi::shots_pick<2>(cdf.data(), pos, blk, last, xs, out);
      printf("%d\n%d\n", out[0], out[1]);
    }
    if (k < nx) {
      const double xs[1] = {x[k]};
      int out[1];
      bornvi::shots_pick<1>(cdf.data(), pos, blk, last, xs, out);
      printf("%d\n", out[0]);
    }
  }
  fclose(f);
  return 0;
}
"""


def _hipcc():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc")
    if not hipcc and os.environ.get("ROCM_PATH"):
        hipcc = os.path.join(os.environ["ROCM_PATH"], "bin", "hipcc")
    if not hipcc and os.path.exists("/opt/rocm/bin/hipcc"):
        hipcc = "/opt/rocm/bin/hipcc"
    return hipcc if hipcc and os.path.exists(hipcc) else None


def test_kernel_pick_function_on_the_host(tmp_path):
    """csrc/shots_dev.hpp, the text the draw kernel calls, compiled into a host driver: its picks equal sm.pick on every
    hazard x (the branch no feasible number of shots reaches on the device) and on 10^4 random (block, x) pairs."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensornetworks_amd", "csrc")
    src = tmp_path / "pick.cpp"
    src.write_text(_PICK_DRIVER)
    exe = str(tmp_path / "pick")
    b = subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + csrc, str(src), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    records = []                                                 # (cdf, positive, x)
    rows = _hazard_rows()
    for v in rows:
        cdf = sm.device_cdf(v)
        records.append((cdf, v > 0, np.array([x for _, xs in _rising_zeros(v, cdf) for x in xs])))
    masses = sm.device_mass(_zero_mass_row().reshape(-1, sm.BLOCK))
    cdf = sm.device_cdf(masses)
    records.append((cdf, masses > 0, np.array([x for _, xs in _rising_zeros(masses, cdf) for x in xs])))
    n_hazard = sum(len(r[2]) for r in records)
    rng = np.random.default_rng(7)
    blocks = [rows[1], rows[2][:2], rows[3][:8], rows[4][:512], np.zeros(64), np.eye(4096)[0], np.eye(4096)[4095], masses,
              np.concatenate([rows[5][:3000], np.zeros(1096)])]
    blocks += [sm.real_row(k, n, rng) for k in "abc" for n in (3, 12)] + [sm.dyadic_row(rng, 1 << n) for n in (1, 5, 12)]
    per = -(-10 ** 4 // len(blocks))
    for v in blocks:
        cdf = sm.device_cdf(v)
        x = rng.random(per) * cdf[-1]
        x[:per // 4] = rng.choice(cdf, per // 4)                  # on a cdf value exactly
        x[per // 4:per // 4 + 8] = [cdf[-1], np.nextafter(cdf[-1], np.inf), np.nextafter(cdf[-1], 0), 0.0, cdf[0], 2 * cdf[-1] + 1,
                                    np.nextafter(cdf[0], 0), cdf[len(cdf) // 2]]
        records.append((cdf, v > 0, x))
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:
        for cdf, positive, x in records:
            mask = np.zeros(sm.BLOCK + 32, dtype=bool)           # the kernel's mask: one zero word past bit 4095
            mask[:len(cdf)] = positive
            f.write(np.array([len(cdf), len(x)], dtype="<i4").tobytes() + cdf.astype("<f8").tobytes()
                    + np.packbits(mask, bitorder="little").tobytes() + x.astype("<f8").tobytes())
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = np.array(r.stdout.split(), dtype=np.int64)
    want = np.concatenate([sm.pick(cdf, positive, x) for cdf, positive, x in records])
    assert n_hazard >= 2406 and len(want) - n_hazard >= 10 ** 4
    assert np.array_equal(got, want)
    assert (want == -1).sum() == per                             # the all-zero block counts nothing


@pytest.mark.skipif(not sm.hp.HAVE_LONGDOUBLE, reason="np.longdouble has no 64-bit mantissa on this machine")
@pytest.mark.parametrize("case", sm.synthetic_cases(), ids=lambda c: c[0])
def test_gpu_inputs_have_no_undecided_draw(case):
    """Every synthetic input of the real-row GPU tests: no draw within the margin of a boundary (a condition of those tests,
    not a measurement), and the sequential, the device-order and the exact histogram agree."""
    name, make, S, seed, epoch, ids = case
    probs = make()
    exact, undecided = sm.histogram_exact(probs, S, seed, epoch, **ids)
    assert undecided == 0, name
    assert (exact.sum(axis=1) == S).all() and (exact[probs == 0] == 0).all()
    assert np.array_equal(sm.histogram(probs, S, seed, epoch, order="device", **ids), exact)
    assert np.array_equal(sm.histogram(probs, S, seed, epoch, **ids), exact)


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
