"""Every sampled-MPS backend call, bit for bit, against the results recorded before the kernels' site sweeps moved into
mps_sample_dev.hpp: tests/golden/sampled_kernels_parent_bits.npz, written on an MI355X by
tests/golden/make_golden_sampled_kernels_bits.py.  The kernels' orders of summation are specified and their inputs come
from a seeded host generator, so each piece (log Z; the sampler's idx, logq and status; the vjp's grad, logq and status;
the score rows of all sites and of a sub-range; the sample-space Gram; the jvp) is a pure function of its case.  A change of
the arithmetic on purpose re-records the file and says so."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sampled_kernels_parent_bits.npz")
# cases, pieces() and piece_bytes() are the recording script's own: what is compared is what was recorded
_spec = importlib.util.spec_from_file_location("make_golden_sampled_kernels_bits",
                                               os.path.join(HERE, "golden", "make_golden_sampled_kernels_bits.py"))
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
