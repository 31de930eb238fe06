"""The fused-dot last pass (circuit_pass_r3_kernel<true>: the parameter-shift dot product accumulated inside the shifted
circuits' final pass) against the stored-probability path (probabilities written, then bornvi_ksd_grad_finish), at the
shapes the pass is scheduled for: n = 14, 16 and 20, both entangling layouts, a small-tile plan (2^11 amplitudes: four
workgroups per CU), angles that put fused gates' pivots in the other row (the exchange flag permutes which weight a
register slot meets), and a strided share of the parameters (one rank's deal).

Bounds: the base circuit does not go through the fused kernel, so q is bitwise equal; the loss is sqrt(ksd2) on both
sides, bitwise; the two gradients sum the same 2^n products in different orders, and agree to 1e-12 of the largest
entry (the bound tests/test_gpu_r3.py holds the two paths to).  The fused path sums in a fixed order: two runs are
bitwise equal."""
import numpy as np
import pytest
import torch

from oracle import circuit as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture()
def be(dev):
    from tensornetworks_amd import backend
    defaults = {k: backend.get_option(dev, k) for k in ("reg_wires", "read_map")}
    yield backend
    backend.release_workspaces()
    backend.set_option(dev, "tile_bits", 13)
    backend.set_option(dev, "tile_bits_multi", 0)
    for k, v in defaults.items():
        backend.set_option(dev, k, v)


def angles(kind, P, rng):
    th = rng.uniform(-np.pi, np.pi, P)
    if kind == "pivot":
        # every other angle a multiple of pi / 2 (RY(pi), RY(pi / 2) and neighbours within 1e-9): |u10| >= |u00| in the
        # fused records, and the +-pi / 2 shifts move more pivots across; the rest stay generic so the gradient is not null
        sel = rng.random(P) < 0.5
        th = np.where(sel, rng.integers(0, 4, P) * np.pi / 2 + 1e-9 * rng.standard_normal(P), th)
    return th


CASES = [("hardware_efficient", 14, 3, 13, "random"), ("all_to_all", 14, 2, 13, "random"),
         ("hardware_efficient", 14, 3, 11, "random"), ("all_to_all", 14, 2, 11, "pivot"),
         ("hardware_efficient", 16, 3, 13, "random"), ("all_to_all", 16, 2, 13, "random"),
         ("hardware_efficient", 16, 2, 13, "pivot"),
         ("hardware_efficient", 20, 2, 13, "random"), ("all_to_all", 20, 1, 13, "random")]


@pytest.mark.parametrize("ansatz,n,L,kb,kind", CASES)
def test_fused_dot_pass_equals_stored_probabilities(be, dev, ansatz, n, L, kb, kind):
    be.set_option(dev, "reg_wires", 3)
    be.set_option(dev, "read_map", 1)
    be.set_option(dev, "tile_bits", kb)
    P = oc.num_params(ansatz, n, L)
    rng = np.random.default_rng(1000 * n + 10 * L + kb)
    th = torch.as_tensor(angles(kind, P, rng), device=dev)
    w = torch.as_tensor(rng.standard_normal(1 << n), device=dev)
    ksd2 = torch.tensor([2.3], dtype=torch.float64, device=dev)
    assert be.paramshift_dot_supported(ansatz, n, L, dev, P)
    for lo, hi, step in ((0, P, 1), (1, P, 3)):          # all parameters; a sharded range with p_stride 3
        cnt = len(range(lo, hi, step))
        probs = be.paramshift_probs(ansatz, n, L, th, lo, hi, include_base=True, p_stride=step).clone()
        loss_u, grad_u, _ = be.ksd_grad_finish(n, probs[1:], cnt, w, ksd2)
        q, tok = be.paramshift_dot_begin(ansatz, n, L, th, lo, hi, p_stride=step)
        loss_f, grad_f = be.paramshift_dot_finish(tok, w, ksd2)
        gmax = float(grad_u.abs().max())
        err = float((grad_f - grad_u).abs().max())
        print(f"{ansatz} n={n} L={L} tile_bits={kb} {kind} range=({lo},{hi},{step}): max|grad|={gmax:.6e} "
              f"max|fused - stored|={err:.3e} ({err / gmax:.3e} of max|grad|)")
        assert grad_f.shape == (cnt,) and gmax > 0.0
        assert torch.equal(q, probs[0]) and torch.equal(loss_f, loss_u)
        assert err <= 1e-12 * gmax
        q2, tok2 = be.paramshift_dot_begin(ansatz, n, L, th, lo, hi, p_stride=step)
        loss_2, grad_2 = be.paramshift_dot_finish(tok2, w, ksd2)
        assert torch.equal(grad_2, grad_f) and torch.equal(q2, q)
        del probs
