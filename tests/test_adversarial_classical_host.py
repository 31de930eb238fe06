"""Classical adversarial trainer, host-side checks (no GPU): the reference trace with gradients
(tests/golden/adversarial_classical_trace.npz) against the float64 NumPy statement of bornvi_reinforce_step and
bornvi_born_table_vjp in adversarial_mirror.py -- this pins the mirror and the fixture to each other."""
import numpy as np
import pytest

from adversarial_mirror import reinforce_numpy, table_vjp_numpy
from conftest import golden


@pytest.mark.parametrize("tag", ["logits", "abs"])
def test_fixture_is_self_consistent(tag):
    """The documented formulas, in float64 on the recorded (idx, logits, log_p, q, w), give the reference's own
    params.grad before clipping (1e-6 of its largest entry), its running baseline (1e-6 relative) and its loss_q (1e-6 of max(1, |loss_q|)), for
    every one of the 4 recorded Born steps."""
    g = golden("adversarial_classical_trace.npz")
    decay = float(g["baseline_decay"])
    base = 0.0
    table = g[f"{tag}_log_p_table"]
    assert g[f"{tag}_idx"].shape == (4, 64) and g[f"{tag}_grad"].shape == (4, 8) and table.shape == (8,)
    for e in range(4):
        idx, logit, q, w = g[f"{tag}_idx"][e], g[f"{tag}_logits"][e], g[f"{tag}_q"][e], g[f"{tag}_w"][e]
        assert np.array_equal(table[idx], g[f"{tag}_log_p"][e])
        d, loss, base = reinforce_numpy(idx, logit, table, q, base, e == 0, decay)
        grad = table_vjp_numpy(w, q, d, 0 if tag == "logits" else 1)
        ref = g[f"{tag}_grad"][e].astype(np.float64)
        err = np.abs(grad - ref).max() / np.abs(ref).max()
        print(f"{tag} epoch {e}: grad err {err:.3e} of max, baseline {base!r} vs {g[f'{tag}_baseline'][e]!r}, "
              f"loss {loss!r} vs {g[f'{tag}_loss_q'][e]!r}")
        assert err <= 1e-6
        assert abs(base - g[f"{tag}_baseline"][e]) <= 1e-6 * abs(g[f"{tag}_baseline"][e])
        # (the reference's loss_q is a float32 mean of terms of magnitude ~1: the form of the tolerance is the one of
        # test_host_logic.py::test_reinforce_step_against_the_reference_trace)
        assert abs(loss - g[f"{tag}_loss_q"][e]) <= 1e-6 * max(1.0, abs(g[f"{tag}_loss_q"][e]))


def test_reinforce_numpy_edge_rules():
    """Outcomes no sample hit and outcomes whose q is below the floor get an exact zero; the loss uses the floor."""
    q = np.array([0.5, 0.5 - 1e-11, 1e-11, 0.0], dtype=np.float32)
    idx = np.array([0, 2, 2, 0])
    logit = np.array([1.0, -2.0, 3.0, 0.5], dtype=np.float32)
    d, loss, base = reinforce_numpy(idx, logit, np.zeros(4, dtype=np.float32), q, 0.0, True, 0.9)
    assert base == pytest.approx(0.625) and d[1] == 0.0 and d[2] == 0.0 and d[3] == 0.0
    assert d[0] == pytest.approx(((1.0 - 0.625 + 0.01) + (0.5 - 0.625 + 0.01)) / (4 * 0.5))
    w = logit.astype(np.float64) - 0.625 + 0.01
    expect = (np.log(0.5) * (w[0] + w[3]) + np.log(float(np.float32(1e-10))) * (w[1] + w[2])) / 4
    assert loss == pytest.approx(expect, rel=1e-12)
