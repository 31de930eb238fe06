"""Guard rails that need no GPU (verdict r1 item 8, advisor r1):

  * tools/check_async_regs.py -- the fast circuit kernel issues its prefetch loads / tile stores from inline asm and
    waits with hand-counted `s_waitcnt vmcnt(N)`; the script compiles the kernel file to gfx950 assembly (hipcc -S
    cross-compiles here) and fails if the compiler touches a register whose load is still in flight;
  * the planner (plan.cpp) compiled with g++ -fsanitize=address,undefined and run over a sweep of configurations,
    its plans and fast tables compared word-hash for word-hash with the production library's;
  * every stage kind the planner hands to the fast kernel is one the kernel has a specialised body for;
  * the library reads no environment variable: its results depend only on its arguments and its handle's options.
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "tensornetworks_amd", "csrc")


def test_async_register_check_is_clean():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_async_regs.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 problem(s)" in r.stdout and "prefetch loads checked" in r.stdout


def test_library_reads_no_environment():
    """No source of libbornvi_hip.so calls getenv: a variable in a job's environment must not change what the library
    computes (per-handle settings go through bornvi_set_option)."""
    calls = []
    for root, dirs, files in os.walk(CSRC):
        dirs[:] = [d for d in dirs if not d.startswith(("_", "."))]
        for f in sorted(files):
            if f.endswith((".hip", ".cpp", ".hpp")):
                path = os.path.join(root, f)
                for i, line in enumerate(open(path, encoding="utf-8"), 1):
                    if re.search(r"getenv\s*\(", line):
                        calls.append(f"{os.path.relpath(path, REPO)}:{i}: {line.strip()}")
    assert not calls, "getenv in the library's sources:\n" + "\n".join(calls)


def _fnv(words):
    h = 1469598103934665603
    for b in np.asarray(words, dtype="<u4").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


CASES = [(0, 3, 4, 0), (0, 8, 4, 0), (0, 12, 4, 0), (0, 14, 3, 11), (0, 16, 6, 0), (0, 16, 2, 12), (0, 17, 2, 0),
         (1, 14, 2, 0), (1, 16, 6, 0), (2, 15, 3, 0), (2, 16, 6, 0), (0, 9, 3, 6), (0, 6, 3, 4), (2, 1, 1, 0),
         (0, 20, 8, 0), (-1, 16, 0, 0), (-1, 20, 0, 0), (-1, 9, 0, 6), (0, 12, 2, 8), (0, 13, 2, 13),
         # the 3-register-wire plan (0x200) and its compact tables, with and without the read map (0x100)
         (0, 16, 6, 0x200), (0, 16, 6, 0x300), (0, 20, 8, 0x300), (1, 14, 2, 0x200 | 11), (2, 15, 3, 0x300 | 12), (0, 12, 4, 0x300),
         (-1, 20, 0, 0x200), (-1, 13, 0, 0x200 | 10), (0, 9, 2, 0x200), (1, 16, 3, 0x300)]


def test_planner_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    exe = str(tmp_path / "plan_sanitize")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + CSRC, "-I" + os.path.join(REPO, "include"),
                            os.path.join(CSRC, "plan.cpp"), os.path.join(REPO, "tests", "plan_sanitize_driver.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stderr
    args = [str(v) for c in CASES for v in c]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900, env=env)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(CASES)
    from tensornetworks_amd import _ext
    for (ansatz, n, L, kb), line in zip(CASES, lines):
        tok = line.split()
        assert tok[:4] == [str(ansatz), str(n), str(L), str(kb)] and tok[4] == "plan", line
        W = _ext.plan_words(ansatz, n, L, kb)
        assert int(tok[5]) == len(W) and int(tok[6], 16) == _fnv(W), f"plan differs under the sanitizers: {line}"
        F, _ = _ext.plan_fast_words(ansatz, n, L, kb)
        if F is None:
            assert int(tok[8]) == 0, line
        else:
            assert int(tok[8]) == len(F) and int(tok[9], 16) == _fnv(F), f"fast tables differ under the sanitizers: {line}"
        assert tok[11] == "1", f"a stage kind outside the fast kernel's switch: {line}"
        if kb & 0x200:
            Cw, _ = _ext.plan_compact_words(ansatz, n, L, kb & 0x1ff)
            if Cw is None:
                assert int(tok[13]) == 0, line
            else:
                assert int(tok[13]) == len(Cw) and int(tok[14], 16) == _fnv(Cw), f"compact tables differ under the sanitizers: {line}"


@pytest.mark.parametrize("ansatz,n,L,kb", [(0, 16, 6, 0), (1, 16, 3, 0), (2, 16, 6, 0), (0, 20, 8, 0), (0, 14, 3, 11), (-1, 20, 0, 0)])
def test_fast_stage_kinds_are_the_kernels_twenty(ansatz, n, L, kb):
    """FS_KIND = gates (0..4, on register bits 0..ng-1) | pre sign << 3 | post sign << 4 for every stage of every pass
    of a fast-eligible plan: the 20 cases of stage_dispatch (kernels_circuit.hip); anything else would make a wave
    skip its 16 tile stores and desynchronise the hand-counted vmcnt waits."""
    from tensornetworks_amd import _ext
    F, offs = _ext.plan_fast_words(ansatz, n, L, kb)
    assert F is not None
    FH_WORDS, FS_WORDS, FS_KIND = 16, 16, 10
    seen = set()
    for o in offs:
        for s in range(int(F[o])):
            seen.add(int(F[o + FH_WORDS + s * FS_WORDS + FS_KIND]))
    allowed = {ng | (pre << 3) | (post << 4) for ng in range(5) for pre in (0, 1) for post in (0, 1)}
    assert seen and seen <= allowed, seen - allowed


def test_hot_kernels_stay_inside_their_register_budget():
    """The compiler's resource remarks of the last build (kept beside the objects by csrc/build.py): no scratch and no
    VGPR spills in the contraction kernels and the Gram builder, at most the set-up code's 20 bytes in the circuit engine.  A small source edit
    has turned a 2.6 ms kernel into a 6.6 ms one this way, with identical results -- only the build can see it."""
    from tensornetworks_amd.csrc import build as b
    objs = [os.path.join(b.OBJ, s + ".o") for s in b.SOURCES]
    if not all(os.path.exists(o + ".remarks") for o in objs):
        pytest.skip("no compiler remarks beside the objects (library built elsewhere)")
    res = b.check_resources(objs, verbose=False)          # raises on a violation
    sym = [v for k, v in res.items() if "quadform_sym_kernel" in k]
    assert sym and sym[0]["vgprs"] + sym[0].get("agprs", 0) <= 256      # two waves per SIMD
