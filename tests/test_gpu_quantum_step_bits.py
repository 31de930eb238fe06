"""The two quantum trainers through their public surface, bit for bit, against the results recorded before the gradient
routes moved to quantum_trainer.py: tests/golden/quantum_step_parent_bits.npz, written on an MI355X by
tests/golden/make_golden_quantum_step_bits.py.  Every case is a pure function of its seeds (the kernels' summation orders
are specified, the only atomics are integer histogram counts), so host plumbing that launches the same kernels on the
same values in the same order reproduces every bit: loss, gradient, q and extras of one step on every route, kind,
K_p form and preconditioner, two steps with finite shots, the two ranks of a strided deal, the history and final theta
of the short epoch loops.  A change of the arithmetic on purpose re-records the file and says so."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "quantum_step_parent_bits.npz")
# cases, pieces() and piece_bytes() are the recording script's own: what is compared is what was recorded
_spec = importlib.util.spec_from_file_location("make_golden_quantum_step_bits",
                                               os.path.join(HERE, "golden", "make_golden_quantum_step_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
def test_every_case_was_recorded(golden):
    assert sorted(golden) == sorted(rec.case_id(c) for c in rec.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.CASES, ids=rec.case_id)
def test_bits_are_the_recorded_ones(golden, case):
    want, at = golden[rec.case_id(case)].tobytes(), 0
    for name, a in rec.pieces(case):
        got = rec.piece_bytes(a)
        assert got == want[at:at + len(got)], (rec.case_id(case), name, a.dtype, a.shape)
        at += len(got)
    assert at == len(want), (rec.case_id(case), at, len(want))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", rec.KINDS)
def test_stored_halves_interleave_to_the_recorded_whole(golden, kind):
    """The strided deal (theta64, r, P, 2), r = 0, 1, through the trainers' shared local method on the stored route:
    both halves return the whole step's loss and q, and their gradient entries interleave to its gradient, bitwise --
    the whole step being the recorded one (on the KSD side the recorded commit had no local method to record)."""
    case = next(c for c in rec.DEALS if c[1] == kind and c[3] == "stored")
    vi, step, _ = rec.make(case)
    rec.set_route(vi, "stored")
    loss, grad, q = (t.clone() for t in step())
    theta64 = vi.born_machine.theta.detach().double().contiguous()
    P = theta64.numel()
    halves = [vi.loss_and_grad_local(theta64, r, P, 2) for r in (0, 1)]
    assert [h[1].numel() for h in halves] == [P - P // 2, P // 2]
    deal = torch.empty_like(grad)
    deal[0::2], deal[1::2] = halves[0][1], halves[1][1]
    assert all(torch.equal(h[0], loss) and torch.equal(h[2], q) for h in halves)
    assert torch.equal(deal, grad)
    whole = golden[rec.case_id(("step", kind, case[2], "stored", case[4], None))].tobytes()
    assert whole.startswith(b"".join(rec.piece_bytes(rec._host(t)) for t in (loss, grad, q)))
