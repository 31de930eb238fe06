"""The posterior-query, log-marginal-gradient and canonical-form backend calls, bit for bit, against the results recorded
before the clamped environment sweep and the workgroup-level products moved into mps_sample_dev.hpp:
tests/golden/mps_query_parent_bits.npz, written on an MI355X by tests/golden/make_golden_mps_query_bits.py.  The kernels'
orders of summation are specified and their inputs come from a seeded host generator, so each piece (the workspace sizes;
mps_log_marginals; mps_log_marginals_vjp; mps_sample_clamped; mps_marginals with pairs; mps_canonicalise at two output bond
dimensions) is a pure function of its case.  A change of the arithmetic on purpose re-records the file and says so."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mps_query_parent_bits.npz")
# cases, pieces() and piece_bytes() are the recording script's own: what is compared is what was recorded
_spec = importlib.util.spec_from_file_location("make_golden_mps_query_bits", os.path.join(HERE, "golden", "make_golden_mps_query_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.CASES, ids=rec.case_id)
def test_bits_are_the_recorded_ones(golden, case):
    want, at = golden[rec.case_id(case)].tobytes(), 0
    for name, a in rec.pieces(case):
        got = rec.piece_bytes(a)
        assert got == want[at:at + len(got)], (rec.case_id(case), name, a.dtype, a.shape)
        at += len(got)
    assert at == len(want), (rec.case_id(case), at, len(want))
