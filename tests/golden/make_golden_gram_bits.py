"""Records tests/golden/gram_parent_bits.npz: the bits of bornvi_fisher_gram and bornvi_qfi_gram on an MI355X for the
shapes below, from the kernel tests' seeded inputs -- per shape the SHA-256 of the matrix's bytes and, up to P = 65, the
matrix.  tests/test_gpu_gram_bits.py takes its shapes, compute() and digest() from here, so this file alone (with the two
kernel test modules it imports) can be copied onto the commit whose bits are to be kept and run there.  The file in the
repository was recorded on the last commit before both kernels moved onto csrc/syrk_f64.hpp.  Run from the repository
root:  python tests/golden/make_golden_gram_bits.py [output.npz]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)) if p not in sys.path]

import test_gpu_fisher_kernel as fisher  # noqa: E402
import test_gpu_qfi_kernel as qfi  # noqa: E402

FISHER_SHAPES = [(3, 2), (17, 5), (65, 9), (130, 9), (2, 19)]               # (n_shift, n)
QFI_SHAPES = [(2, 3), (17, 9), (65, 9), (127, 3), (288, 9), (2, 18)]        # (P, n)
KEEP_MATRIX_UP_TO = 65


def compute(kind, P, n, dev):
    """The kernel's matrix for the kernel test's inputs of this shape, as a C-contiguous float64 array on the host."""
    mod = fisher if kind == "fisher" else qfi
    return np.ascontiguousarray(mod.run(*mod.inputs(P, n)[:2], dev).cpu().numpy())


def digest(M):
    return hashlib.sha256(M.tobytes()).hexdigest()


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    out = {}
    for kind, shapes in (("fisher", FISHER_SHAPES), ("qfi", QFI_SHAPES)):
        for P, n in shapes:
            M = compute(kind, P, n, dev)
            assert M.shape == (P, P) and np.isfinite(M).all() and digest(M) == digest(compute(kind, P, n, dev))
            out[f"{kind}_{P}_{n}_sha256"] = np.array(digest(M))
            if P <= KEEP_MATRIX_UP_TO:
                out[f"{kind}_{P}_{n}"] = M
            print(f"{kind} P={P} n={n}: sha256 {digest(M)[:16]}")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "gram_parent_bits.npz")
    np.savez(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
