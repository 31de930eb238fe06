"""bornvi_fisher_gram and bornvi_qfi_gram, bit for bit, against the results recorded before both kernels moved onto the
shared split-K core (csrc/syrk_f64.hpp): tests/golden/gram_parent_bits.npz, written on an MI355X by
tests/golden/make_golden_gram_bits.py from the kernel tests' seeded inputs.  The kernels' summation order is specified
(per slab inside the MFMAs, the workgroup's slabs in order, the G partial tiles in index order), so a change that keeps
the layout reproduces every bit; a change of the layout on purpose re-records the file and says so.

Every shape carries the SHA-256 of the result's bytes; shapes with P <= 65 also the matrix, so that a mismatch names
its entries."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gram_parent_bits.npz")
# shapes, compute() and digest() are the recording script's own: what is compared is what was recorded
_spec = importlib.util.spec_from_file_location("make_golden_gram_bits", os.path.join(HERE, "golden", "make_golden_gram_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,P,n", [("fisher", P, n) for P, n in rec.FISHER_SHAPES] + [("qfi", P, n) for P, n in rec.QFI_SHAPES])
def test_bits_are_the_recorded_ones(dev, golden, kind, P, n):
    key = f"{kind}_{P}_{n}"
    M = rec.compute(kind, P, n, dev)
    if P <= rec.KEEP_MATRIX_UP_TO:
        want = golden[key]
        differ = np.argwhere(M.view(np.uint64) != want.view(np.uint64))
        assert differ.size == 0, (key, len(differ), differ[:8].tolist())
    assert rec.digest(M) == str(golden[key + "_sha256"]), key
