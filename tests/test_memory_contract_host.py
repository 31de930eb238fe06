"""The memory-contract harness (tests/memory_contract.py) shown to catch what it is for, without a faulty GPU kernel: host
stand-ins behind the same Case interface, one correct and one per fault, each of which must fail exactly the assertion named
for it.  The toy entry:  y[n] = 2 x[n] through a workspace of n words (ws = 3 x; y = ws - x), s[1] = sum x or NULL; int64
throughout, so that 0xFF bytes are -1 and nothing is a NaN."""
import os

import numpy as np
import pytest
import torch

import memory_contract as mc

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "bornvi.h")


def words(mem, addr, n, start=0):
    return mem[addr + 8 * start:addr + 8 * (start + n)].view(torch.int64)


def stand_in(fault=None):
    def run(n):
        def call(mem, addr):
            x, y, ws = (words(mem, addr[k], n) for k in ("x", "y", "ws"))
            stale = int(ws[0])
            beyond = int(words(mem, addr["x"], 1, start=n)[0])
            ws.copy_(3 * x)
            y.copy_(ws - x)
            if addr["s"] is not None:
                words(mem, addr["s"], 1)[0] = x.sum()
            if fault == "writes one element past an output":
                words(mem, addr["y"], 1, start=n)[0] = 7
            elif fault == "writes one byte past the workspace":
                mem[addr["ws"] + 8 * n] = 7
            elif fault == "reads a workspace slot before writing it":
                y[0] += stale
            elif fault == "leaves an output tail unwritten":
                y[n - 1] = before_tail[0]
            elif fault == "reads one element past an input into a result":
                y[n - 1] += beyond
            elif fault == "modifies an input":
                x[0] += 1
            elif fault == "changes an output when an optional one is NULL":
                if addr["s"] is None:
                    y[0] += 1
            elif fault == "needs more than the stated alignment":
                if addr["y"] % 16:
                    y[0] += 1
            else:
                assert fault is None, fault
        before_tail = [0]

        def call_keeping_tail(mem, addr):
            before_tail[0] = int(words(mem, addr["y"], n)[n - 1])
            call(mem, addr)
        return call_keeping_tail
    return run


def toy_case(n, seed, fault=None):
    x = np.random.default_rng(seed).integers(-1000, 1000, n)
    bufs = [mc.Buffer("x", "in", data=x.astype(np.int64)), mc.Buffer("y", "out", nbytes=8 * n),
            mc.Buffer("s", "out", nbytes=8, optional=True), mc.Buffer("ws", "workspace", nbytes=8 * n, align=mc.WS_ALIGN)]
    return mc.Case(bufs, stand_in(fault)(n))


def check(fault, n=37):
    return mc.check_case(toy_case(n, 0, fault), toy_case(n + 27, 1, fault), "cpu")


def test_correct_stand_in_passes_all_five():
    out = check(None)
    x = np.random.default_rng(0).integers(-1000, 1000, 37)
    assert np.array_equal(out["y"].view(torch.int64).numpy(), 2 * x) and int(out["s"].view(torch.int64)[0]) == x.sum()


@pytest.mark.parametrize("fault,error", [
    ("writes one element past an output", mc.ExtentError),
    ("writes one byte past the workspace", mc.ExtentError),
    ("reads a workspace slot before writing it", mc.PriorDependence),
    ("leaves an output tail unwritten", mc.PriorDependence),
    ("reads one element past an input into a result", mc.PriorDependence),
    ("modifies an input", mc.InputModified),
    ("changes an output when an optional one is NULL", mc.OptionalChanged),
    ("needs more than the stated alignment", mc.PlacementChanged),
])
def test_each_fault_fails_the_assertion_named_for_it(fault, error):
    with pytest.raises(mc.ContractError) as e:
        check(fault)
    assert type(e.value) is error, (fault, e.value)


def test_documented_unwritten_part_must_keep_the_fill():
    """An `out` with a documented unwritten tail: leaving it alone passes, writing it fails assertion 2."""
    def case(n, seed, write_tail):
        x = np.random.default_rng(seed).integers(-9, 9, n).astype(np.int64)
        mask = np.zeros(8 * n, bool)
        mask[8 * (n - 2):] = True

        def run(mem, addr):
            y = words(mem, addr["y"], n)
            y[:n - 2] = words(mem, addr["x"], n)[:n - 2]
            if write_tail:
                y[n - 1] = 0
        return mc.Case([mc.Buffer("x", "in", data=x), mc.Buffer("y", "out", nbytes=8 * n, unwritten=mask)], run)
    mc.check_case(case(9, 0, False), case(12, 1, False), "cpu")
    with pytest.raises(mc.PriorDependence):
        mc.check_case(case(9, 0, True), case(12, 1, True), "cpu")


def test_guard_bands_are_at_least_the_largest_buffer_and_a_mebibyte():
    small = toy_case(5, 0).buffers
    big = [mc.Buffer("a", "out", nbytes=3 << 20), mc.Buffer("b", "out", nbytes=8)]
    for bufs in (small, big):
        G = mc.guard_bytes(bufs)
        assert G - 2 * mc.MARGIN >= max(mc.MIN_GUARD, max(b.nbytes for b in bufs))
        for least in (False, True):
            offs, size = mc.layout(bufs, 0x1000, least)
            ends = [0] + [offs[b.name] + b.nbytes for b in bufs]
            assert all(offs[b.name] - e >= G for b, e in zip(bufs, ends)) and size - ends[-1] >= G
            for b in bufs:
                a = 0x1000 + offs[b.name]
                assert a % b.align == 0 and (a % (2 * b.align) != 0) == least


def test_completeness_check_rejects_an_uncovered_declaration():
    with open(HEADER) as f:
        text = f.read()
    covered = set(mc.ROLES)
    assert mc.check_complete(text, mc.ROLES, covered) == []
    mark = "#if defined(__GNUC__)\n#pragma GCC visibility pop"
    assert text.count(mark) == 1
    more = text.replace(mark, "int bornvi_new_thing(bornvi_handle h, int n, const double* a, double* b, bornvi_stream stream);\n" + mark)
    assert mc.check_complete(more, mc.ROLES, covered) == ["bornvi_new_thing: no memory contract"]
    roles = dict(mc.ROLES, bornvi_new_thing=dict(a="in"))
    assert mc.check_complete(more, roles, covered) == ["bornvi_new_thing: no case runs it", "bornvi_new_thing: pointer 'b' has no role"]
    # a host-only declaration (no stream) needs none
    host_only = text.replace(mark, "int bornvi_new_query(int n, int* out);\n" + mark)
    assert mc.check_complete(host_only, mc.ROLES, covered) == []
