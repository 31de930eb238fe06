"""What the library refuses, and in which words, against the answers recorded before the binding, the limits and the option
table were derived from include/bornvi.h: tests/golden/abi_refusals_parent.json, written on an MI355X by
tests/golden/make_golden_abi_refusals.py.  Every case is refused in the argument checks, before a device is selected or
anything is launched; return values and texts must be the recorded ones.

One difference is allowed.  The recorded library could set "workgroups_per_cu" and "max_threads" but answered a read of them
with "unknown option"; the option table answers reads for every name it sets.  For exactly those two reads the test accepts
either the recorded refusal or success with the value last set (here the default, since no case sets them)."""
import importlib.util
import json
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "abi_refusals_parent.json")
# the cases and the way a case is run are the recording script's own: what is compared is what was recorded
_spec = importlib.util.spec_from_file_location("make_golden_abi_refusals", os.path.join(HERE, "golden", "make_golden_abi_refusals.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def session():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    s = rec.Session()
    yield s
    s.close()


def test_every_case_was_recorded(golden):
    assert sorted(golden) == sorted([c[0] for c in rec.CASES] + [c[0] for c in rec.OPTION_CASES])


@pytest.mark.gpu
def test_refusals_are_the_recorded_ones(golden, session):
    wrong = {}
    for case in rec.CASES:
        got = session.run_case(case)
        if got != golden[case[0]]:
            wrong[case[0]] = (got, golden[case[0]])
    assert not wrong, wrong


@pytest.mark.gpu
def test_options_answer_as_recorded(golden, session):
    wrong = {}
    for case in rec.OPTION_CASES:
        got, want = session.run_option_case(case), golden[case[0]]
        _, kind, name, _ = case
        if kind == "get" and name in rec.SET_ONLY_OPTIONS:
            assert want == [-1, f"unknown option {name}", None], (case[0], want)
            ok = got == want or got == [0, f"unknown option {rec.SENTINEL}", rec.SET_ONLY_OPTIONS[name]]
        else:
            ok = got == want
        if not ok:
            wrong[case[0]] = (got, want)
    assert not wrong, wrong
