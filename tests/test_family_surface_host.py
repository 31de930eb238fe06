"""born_machine_base.py without a GPU: the outcome index <-> bit row helpers (round trips up to n = 63, the validation and
its message, the same out of all three machines), and the three families' starting parameters after torch.manual_seed(7),
bit for bit, against tests/golden/family_init_seed7.npz (tests/golden/make_golden_family_init.py, recorded before the
families moved onto the shared module)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tensornetworks_amd.born_machine_base import bits_to_indices, indices_to_bits
from tensornetworks_amd.born_machine_classical_sim import ClassicalBornMachine
from tensornetworks_amd.born_machine_mps import MPSBornMachine
from tensornetworks_amd.born_machine_mps_sampled import SampledMPSBornMachine

HERE = os.path.dirname(os.path.abspath(__file__))
# cases and parameters() are the recording script's own: what is compared is what was recorded
_spec = importlib.util.spec_from_file_location("make_golden_family_init", os.path.join(HERE, "golden", "make_golden_family_init.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.mark.parametrize("n", [1, 26, 63])
def test_round_trip(n):
    top = (1 << n) - 1                                   # the all-ones index: 2^63 - 1 at n = 63, the largest int64
    idx = torch.tensor(sorted({0, 1, top, top - 1, top >> 1, (top >> 1) + 1, 0x5555555555555555 & top}), dtype=torch.int64)
    bits = indices_to_bits(idx, n)
    assert bits.shape == (idx.numel(), n) and bits.dtype == torch.float32
    want = [[(int(i) >> (n - 1 - k)) & 1 for k in range(n)] for i in idx]
    assert bits.tolist() == want
    assert torch.equal(bits[idx.tolist().index(top)], torch.ones(n))
    back = bits_to_indices(bits, n)
    assert back.dtype == torch.int64 and torch.equal(back, idx)
    assert torch.equal(indices_to_bits(idx.reshape(1, -1), n), bits.unsqueeze(0))        # leading dimensions are kept


BAD_ROWS = [(torch.tensor([[0., 1., 0.], [0., 2., 1.]]), r"Sample \(0, 2, 1\) is not a valid outcome\."),
            (torch.tensor([[1., -1., 0.]]), r"Sample \(1, -1, 0\) is not a valid outcome\."),
            (torch.tensor([[0., 1., 0., 1.]]), r"Sample \(0, 1, 0, 1\) is not a valid outcome\."),
            (torch.tensor([0., 1., 1.]), r"Sample \(0, 1, 1\) is not a valid outcome\.")]


@pytest.mark.parametrize("z,message", BAD_ROWS)
def test_invalid_rows_raise(z, message):
    with pytest.raises(ValueError, match=message):
        bits_to_indices(z, 3)
    uniform = torch.full((8,), 0.125)
    for bm in (ClassicalBornMachine(3), MPSBornMachine(3, bond_dim=2)):
        bm.set_fixed_probs(uniform)                       # the check comes after q: fixed probabilities need no GPU
        with pytest.raises(ValueError, match=message):
            bm.get_log_q_z_x(z)
    with pytest.raises(ValueError, match=message):        # the sampled machine checks before it asks for a GPU
        SampledMPSBornMachine(3, bond_dim=2).get_log_q_z_x(z)


@pytest.mark.parametrize("family,variant", rec.CASES)
def test_seeded_parameters_are_the_recorded_ones(golden_loader, family, variant):
    got = rec.parameters(family, variant)
    with golden_loader("family_init_seed7.npz") as want:
        assert got and set(got) == {k for k in want.files if k.startswith(f"{family}/{variant}/")}
        for key, a in got.items():
            assert a.dtype == want[key].dtype and a.shape == want[key].shape, key
            assert a.tobytes() == want[key].tobytes(), key
