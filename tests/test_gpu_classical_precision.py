"""bornvi_born_table_probs / bornvi_born_table_vjp and bornvi_reinforce_step on the MI355X against extended precision, per
entry (classical_hp.py: the references, the constants counted on the kernels' chains, the allowed error of every output).
Every ratio printed here is |kernel - reference| / allowed and must not exceed 1; the constants that `allowed` is built
from are printed beside it.  test_classical_precision_host.py shows on the CPU that these bounds hold for a plain float64
evaluation and that seven seeded mistakes leave them.

Shapes are the smallest on both sides of every path change, not the workload's: N = 2 (scalar loads), N = 4 (the first
float4 size), n = 12 / 13 (one workgroup per row / two), n = 21 (the first G > 256: the second trip of the loops over a
row's partials); for the REINFORCE step one and two sample workgroups (B = 1024 / 1025), more zeroing workgroups than
sample workgroups (n = 13, B = 1) and the reverse (n = 3, B = 5000)."""
import ctypes as C

import numpy as np
import pytest
import torch

import classical_hp as chp

if chp.unavailable():
    pytest.skip(chp.unavailable(), allow_module_level=True)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached inputs are read-only)


def host(t):
    return None if t is None else t.cpu().numpy()


def table_constants_line(n, mode):
    c = chp.table_constants(n, mode)
    return f"C_Q {c['q']:g} C_H {c['H']:g} C_1 {c['g1']:g} C_c {c['gc']:g} (G {c['G']}, chain {c['L']})"


# ---- table kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,family", chp.TABLE_FAMILIES)
@pytest.mark.parametrize("n,rows", chp.TABLE_SHAPES)
def test_table_kernels_against_extended_precision(n, rows, mode, family):
    from tensornetworks_amd import backend
    w, ref = chp.forward_case(n, rows, mode, family)
    wd = dev(w)
    q32, q64, H = backend.born_table_probs(wd, mode)
    r = chp.forward_check(w, mode, host(q32), host(q64), host(H), ref)
    ties = chp.tie_exceptions(ref[0], chp.table_constants(n, mode)["q"])
    print(f"kernel n={n} rows={rows} mode={mode} {family}: q32 ratio {r['q'][0]:.3g} at {r['q'][1]} ({ties} entries near a "
          f"tie), H ratio {r['H'][0]:.3g}; float32 underflow: {chp.underflow_mode(host(q32), ref[0])}; "
          f"{table_constants_line(n, mode)}")
    assert r["q"][0] <= 1.0 and r["H"][0] <= 1.0, r
    q32b, q64b, none = backend.born_table_probs(wd, mode, want_entropy=False)
    assert none is None and torch.equal(q32b, q32) and torch.equal(q64b, q64)

    y, ksd2 = chp.vjp_inputs(n, rows)
    q64h = host(q64)
    for has_y, has_k, lam in chp.VJP_CONFIGS:
        yy, kk = (y if has_y else None), (ksd2 if has_k else None)
        loss = torch.full((rows,), -1.0, dtype=torch.float64, device=DEV) if has_k else None
        g = backend.born_table_vjp(wd, q64, mode, y=dev(yy), ksd2=dev(kk), entropy_weight=lam, loss_out=loss)
        rg = chp.vjp_check(w, q64h, yy, kk, lam, mode, host(g), host(loss))["g"]
        print(f"  vjp y={has_y} ksd2={has_k} lambda={lam}: dL/dw ratio {rg[0]:.6g} at {rg[1]}")
        assert rg[0] <= 1.0, (has_y, has_k, lam, rg)
        if family == "zeros":
            assert bool((g[:, ::3] == 0).all())


def offset_view(t):
    """t's values one element into a larger buffer (not 16-byte aligned), with a guard element on either side."""
    buf = torch.full((t.numel() + 2,), 7.0, dtype=t.dtype, device=t.device)
    buf[1:-1] = t.reshape(-1)
    return buf, buf[1:-1].view(t.shape)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [3, 13])
def test_unaligned_views_give_the_same_bits(n, mode):
    """w, q32, q64, y and the gradient one element into a larger buffer: the kernels take their scalar path (vec = 0) over
    one and two workgroups per row.  Every entry equals the aligned call's bit for bit (each entry is a function of its own
    input and of the row's sums; the sums move in their last bits with the order of the additions, which changes an entry
    only across a float32 tie); H, a sum, is held to its bound instead.  The C ABI is called directly: the wrappers
    allocate q32 and q64 themselves."""
    from tensornetworks_amd import _ext, backend
    rows, N = 3, 1 << n
    w, ref = chp.forward_case(n, rows, mode, "random")
    y, ksd2 = chp.vjp_inputs(n, rows)
    wd, yd, kd = dev(w), dev(y), dev(ksd2)
    q32, q64, H = backend.born_table_probs(wd, mode)
    loss = torch.empty(rows, dtype=torch.float64, device=DEV)
    g = backend.born_table_vjp(wd, q64, mode, y=yd, ksd2=kd, entropy_weight=chp.LAMBDA, loss_out=loss)

    h = _ext.handle_for(DEV)
    ws = torch.empty(h.size("bornvi_born_table_workspace_bytes", n, rows), dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    bufs = [offset_view(t) for t in (wd, torch.zeros_like(q32), torch.zeros_like(q64), yd, torch.zeros_like(g))]
    (_, wu), (_, q32u), (_, q64u), (_, yu), (_, gu) = bufs
    assert all(v.data_ptr() % 16 for v in (wu, q32u, q64u, yu, gu))
    Hu, lossu = torch.empty_like(H), torch.empty_like(loss)
    h.call("bornvi_born_table_probs", n, rows, mode, p(wu), p(q32u), p(q64u), p(Hu), p(ws), ws.numel(), _ext.stream_ptr(DEV))
    h.call("bornvi_born_table_vjp", n, rows, mode, p(wu), p(q64u), p(yu), p(kd), chp.LAMBDA, p(gu), p(lossu), p(ws),
           ws.numel(), _ext.stream_ptr(DEV))
    torch.cuda.synchronize()
    for buf, _ in bufs:
        assert float(buf[0]) == 7.0 and float(buf[-1]) == 7.0          # nothing outside the views was written
    assert torch.equal(q32u, q32) and torch.equal(q64u, q64) and torch.equal(gu, g) and torch.equal(lossu, loss)
    r = chp.forward_check(w, mode, host(q32u), host(q64u), host(Hu), ref)
    print(f"unaligned n={n} mode={mode}: q32 ratio {r['q'][0]:.3g} H ratio {r['H'][0]:.3g} (aligned H == unaligned H: "
          f"{torch.equal(Hu, H)}); {table_constants_line(n, mode)}")
    assert r["q"][0] <= 1.0 and r["H"][0] <= 1.0, r
    # one operand unaligned is enough for the scalar path: the aligned outputs again, from the offset w alone
    q32m, q64m, _ = backend.born_table_probs(wu, mode)
    assert torch.equal(q32m, q32) and torch.equal(q64m, q64)
    assert torch.equal(backend.born_table_vjp(wd, q64, mode, y=yu, ksd2=kd, entropy_weight=chp.LAMBDA), g)


# ---- REINFORCE -----------------------------------------------------------------------------------------------------
def run_step(idx, logit, log_p, q32, baseline, first, decay):
    from tensornetworks_amd import backend
    base = torch.tensor([baseline], dtype=torch.float64, device=DEV)
    d, loss, found = backend.reinforce_step(dev(idx), dev(logit), dev(log_p), dev(q32), base, first, decay)
    return d, loss, found, base


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("kind", chp.REINFORCE_KINDS)
@pytest.mark.parametrize("n,B", chp.REINFORCE_SHAPES)
def test_reinforce_step_against_extended_precision(n, B, kind, first):
    inp = chp.step_inputs(n, B, kind, chp.step_seed(n, B, kind, first))
    ref = chp.reinforce_reference(*inp, chp.BASELINE, first, chp.DECAY)
    d, loss, found, base = run_step(*inp, chp.BASELINE, first, chp.DECAY)
    assert float(found) == 0.0
    r = chp.reinforce_check(ref, host(d), host(loss).astype(np.float64), host(base))
    big = inp[3] > 0.1
    r_big = chp.hp.worst(chp.allowed_ratio(host(d)[big], ref["d"][0][big], ref["d"][1][big]))[0] if big.any() else 0.0
    print(f"kernel n={n} B={B} {kind} first={first}: dLdq ratio {r['d'][0]:.3g} at {r['d'][1]} (q > 0.1: {r_big:.3g}), "
          f"loss ratio {r['loss'][0]:.3g}, baseline ratio {r['base'][0]:.3g}; u 2^{int(np.log2(ref['u']))} "
          f"T_mean {ref['T_mean']:g} T_loss {ref['T_loss']:g}")
    assert max(v[0] for v in r.values()) <= 1.0, r
    hit = ref["hits"] > 0
    assert torch.count_nonzero(d[dev(~hit)]).item() == 0               # never sampled: exact zeros, no store
    assert torch.count_nonzero(d[dev(inp[3] < chp.CLAMP32)]).item() == 0      # q below the floor


@pytest.mark.parametrize("kind", ["mixed", "peaked"])
@pytest.mark.parametrize("n,B", [(12, 65536), (8, 1025)])
def test_reinforce_step_is_order_independent_bit_for_bit(n, B, kind):
    """first = False and baseline_decay = 1: the new baseline is 1 * baseline + 0 * mean, the old one bit for bit whatever
    the last bits of the mean; W is a maximum; the sums are integer sums.  So dLdq, loss and baseline after a permutation of
    the samples (idx and logit together) are required to equal the unpermuted call's bits."""
    idx, logit, log_p, q32 = chp.step_inputs(n, B, kind, chp.step_seed(n, B, kind, False) + 3)
    d0, loss0, found0, base0 = run_step(idx, logit, log_p, q32, chp.BASELINE, False, 1.0)
    assert float(found0) == 0.0 and float(base0) == chp.BASELINE and torch.count_nonzero(d0).item() > 0
    for s in (1, 2):
        perm = np.random.default_rng([n, B, s]).permutation(B)
        d, loss, _, base = run_step(idx[perm], logit[perm], log_p, q32, chp.BASELINE, False, 1.0)
        assert torch.equal(base.view(torch.int64), base0.view(torch.int64))
        assert torch.equal(d.view(torch.int64), d0.view(torch.int64)), int((d != d0).sum())
        assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32))
