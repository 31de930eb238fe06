"""The three sampled MPS families through their public surface, bit for bit, against the results recorded before they moved
onto born_machine_sampled.SampledSurface: tests/golden/sampled_surface_parent_bits.npz, written on an MI355X by
tests/golden/make_golden_sampled_surface_bits.py.  Every case is a pure function of its seeds (the kernels' summation orders
are specified), so host plumbing that launches the same kernels on the same values in the same order reproduces every bit:
the draws, the counter behind sample(), score_vjp, log_prob, probabilities64 (and its gradient for the real family), and
three epochs of the ELBO trainer per `cores` kind.  A change of the arithmetic on purpose re-records the file and says so."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sampled_surface_parent_bits.npz")
# cases, pieces() and piece_bytes() are the recording script's own: what is compared is what was recorded
_spec = importlib.util.spec_from_file_location("make_golden_sampled_surface_bits",
                                               os.path.join(HERE, "golden", "make_golden_sampled_surface_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.MACHINES + rec.TRAINERS, ids=rec.case_id)
def test_bits_are_the_recorded_ones(golden, case):
    want, at = golden[rec.case_id(case)].tobytes(), 0
    for name, a in rec.pieces(case):
        got = rec.piece_bytes(a)
        assert got == want[at:at + len(got)], (rec.case_id(case), name, a.dtype, a.shape)
        at += len(got)
    assert at == len(want), (rec.case_id(case), at, len(want))
