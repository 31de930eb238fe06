"""Every launching entry point of include/bornvi.h held to its memory contract (tests/memory_contract.py): each case runs the
call, or the sequence, from an arena whose guard bands the test compares, three times on the same inputs -- prior contents all
0x00 (run Z), the leftovers of a larger valid call of the same entry (run L), all 0xFF (run F: every double a NaN, every int -1)
-- then once per optional output with that pointer NULL, once with other bytes in the documented never-read parts of the inputs,
and once with every buffer at the least alignment the header allows.  Asserted: nothing outside the writable buffers changes
(which also proves that the *_workspace_bytes size suffices: the workspace is exactly that long), the outputs are bitwise the
same in every run, documented unwritten parts keep the run's fill, and the inputs are untouched.

The completeness test needs no GPU: every declared function with a `stream` parameter has its contract written down, with a
role for every pointer, and a case that runs it."""
import ctypes as C
import os

import pytest
import torch

import memory_contract as mc

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "bornvi.h")
CASES = [pytest.param(fam, i, id=f"{fam.name}-{'-'.join(str(v) for v in (s if isinstance(s, tuple) else (s,)))}")
         for fam in mc.FAMILIES for i, s in enumerate(fam.shapes)]


def test_every_launching_function_has_its_contract_written_down():
    with open(HEADER) as f:
        text = f.read()
    assert mc.check_complete(text, mc.ROLES, mc.covered()) == []
    launching = set(mc.launching_functions(text))
    assert set(mc.ROLES) == launching and mc.covered() == launching       # and nothing is specified that the header does not declare


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tensornetworks_amd import _ext
    return _ext.handle_for(torch.device("cuda", 0))


@pytest.fixture()
def options(handle):
    """The handle's options as they were, put back after the case (in this order: setting tile_bits also sets tile_bits_multi)."""
    keep = {}
    for name in mc.OPTION_NAMES:
        v = C.c_longlong(0)
        handle.call("bornvi_get_option", name.encode(), C.byref(v))
        keep[name] = int(v.value)
    yield handle
    for name, v in keep.items():
        handle.call("bornvi_set_option", name.encode(), v)


@pytest.mark.gpu
@pytest.mark.parametrize("fam,i", CASES)
def test_memory_contract(options, fam, i):
    case = fam.case(options, i, 0)
    donor = fam.donor(options, i)
    mc.check_case(case, donor, torch.device("cuda", 0))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [pytest.param(f, id=f.name) for f in mc.FAMILIES
                                 if any(mc.role_of(fn, p)[2] for fn in f.covers for p in mc.ROLES[fn])])
def test_stated_alignment_is_enforced_before_any_launch(options, fam):
    """Every pointer whose 16-byte alignment the header states: 8 bytes off, the call is refused and nothing is written."""
    from tensornetworks_amd import _ext
    case = fam.case(options, 0, 0)
    names = [b.name for b in case.buffers if b.stated]
    assert names
    for name in names:
        mc.check_refusal(case, name, torch.device("cuda", 0), _ext.BornviError)
