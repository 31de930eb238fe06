"""bornvi_mps_twosite_sweep against its mirror (mps_twosite_mirror.py: the same round trip in float64 and in extended precision),
against bornvi_mps_canonicalise and bornvi_mps_score_vjp on the same cores, and its contract: the entry gauge on return, exact
zeros, the status bits, bitwise reproducible, capturable, refused arguments.

Shapes (n, D, B): one bond touching both boundaries with a 2 x 2 matrix; the smallest real bond matrix; odd D (an idle Jacobi
pair) with a partial second tile; 2 D = 10 rows, uneven over a lane group; the full 32 x 32 factorisation and a full MFMA tile;
depth; more tiles than workgroups (the accumulate grid is capped at 256).

Inputs: canonical cores (the mirror's canonical form of random ones) and samples DRAWN FROM q of those cores, so that no psi_b
is small against its terms and the descent is well conditioned: the float64 mirror then stays within a few units of the
extended one (printed as r64), which is the condition under which a bound on a chaotic iteration means something.

Bounds.  The compared quantities are gauge-free (loss, schmidt, discarded, psi over all states), in units of EPS64 against 1
(the state has norm 1, Schmidt values are <= 1), norm-wise as in test_gpu_mps_canon_kernel.py: hp.measured_constant(r64,
derived), r64 what the float64 mirror shows against the extended one, derived = mps_twosite_mirror.derived_constant (DESIGN.md
section 6o).  loss is compared in units of loss_scale = |L| + 2 sum_b w_b / |psi_b|: a norm-wise error e of the state moves
log psi_b^2 by 2 e / |psi_b|.  No constant is fitted to the device; every test prints its worst ratio beside the bound.
Cuts: every case asserts with the mirror that the gap between the smallest kept and the largest dropped normalised value is
above 1e-6, far above the bound, so that the ranks are well defined."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import hp_reference as hp
import mps_canon_mirror as cm
import mps_sampled_mirror as sm
import mps_twosite_mirror as tm
import test_gpu_mps_sampled_kernel as tk
from tensornetworks_amd import _ext, backend

pytestmark = pytest.mark.gpu

EPS = hp.EPS64
SHAPES = [(2, 1, 1), (2, 2, 3), (3, 3, 65), (6, 5, 200), (12, 16, 1000), (63, 4, 130), (5, 4, 16449)]
UNSUPPORTED = -4
dev = tk.dev


def t_(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(dev())


@functools.lru_cache(maxsize=None)
def inputs(n, D, B):
    """(canonical cores [n, 2, D, D], idx [B] drawn from their q): enumerated for n <= 12, bornvi_mps_sample above."""
    rng = np.random.default_rng(100 * n + D)
    c = tm.canonical((np.eye(D) + 0.3 * rng.standard_normal((n, 2, D, D))) / np.sqrt(2.0))
    if n <= 12:
        q = tm.probabilities(c)
        idx = rng.choice(1 << n, size=B, p=q / q.sum()).astype(np.int64)
    else:
        ct = t_(c)
        backend.mps_environments(ct, B)
        idx = backend.mps_sample(ct, B, 99, torch.tensor([0], dtype=torch.int64, device=dev()))[0].cpu().numpy()
    return c, idx


def run(cores, idx, w=None, lr=0.0, steps=1, keep=None, cutoff=0.0):
    ct = t_(cores).clone()
    out = backend.mps_twosite_sweep(ct, t_(idx, torch.int64), None if w is None else t_(w), lr, steps, keep, cutoff)
    torch.cuda.synchronize()
    loss, schmidt, discarded, rank, status = (x.cpu().numpy() for x in out)
    return dict(cores=ct.cpu().numpy(), loss=loss, schmidt=schmidt, discarded=discarded, rank=rank, status=int(status[0]), dev_cores=ct)


@functools.lru_cache(maxsize=None)
def case(n, D, B, lr, steps, keep, cutoff):
    """The GPU's result and both mirrors' on inputs(n, D, B), computed once and shared."""
    c, idx = inputs(n, D, B)
    kw = dict(lr=lr, steps=steps, D_keep=keep, cutoff=cutoff)
    return dict(c=c, idx=idx, gpu=run(c, idx, None, lr, steps, keep, cutoff), m64=tm.sweep(c, idx, **kw), mld=tm.sweep(c, idx, dtype=tm.LD, **kw))


def units(got, ref, scale=None):
    got, ref = np.asarray(got).astype(tm.LD), np.asarray(ref).astype(tm.LD)
    if got.size == 0:
        return 0.0
    d = np.abs(got - ref)
    return float((d / (1 if scale is None else scale)).max() / tm.LD(EPS))


def score_logq(cores_np, idx, w):
    """(logq [B] of bornvi_mps_score_vjp, its bound per sample in units of EPS64) for cores and samples on the host."""
    n, D = cores_np.shape[0], cores_np.shape[2]
    ct, it = t_(cores_np), t_(idx, torch.int64)
    backend.mps_environments(ct, len(idx))
    lq = backend.mps_score_vjp(ct, it, t_(w))[1].cpu().numpy()
    ref = sm.conditionals(cores_np, tm.bits_of(idx, n))
    env = sm.environments(cores_np)
    kb = hp.to_f64(ref["psi_abs"] / np.abs(ref["psi"]))
    return lq, tk.logq_bound(n, D, kb, float(env["Z_abs"] / env["Z"]), hp.to_f64(ref["logq"]), float(np.log(env["Z"])))


# ---- 1. lr = 0 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,B", SHAPES)
def test_lr_zero_is_the_identity_on_the_state(n, D, B):
    r = case(n, D, B, 0.0, 1, None, 0.0)
    g, m64, mld, c, idx = r["gpu"], r["m64"], r["mld"], r["c"], r["idx"]
    derived = tm.derived_constant(n, D, 1)
    assert g["status"] == 0 and mld["status"] == 0
    if n <= 12:
        psi_in = cm.psi_of(c)[0]
        r64 = float(np.abs(cm.psi_of(hp.to_f64(m64["cores"]))[0] - psi_in).max() / tm.LD(EPS))
        e = float(np.abs(cm.psi_of(g["cores"])[0] - psi_in).max() / tm.LD(EPS))
        Cp = hp.measured_constant(r64, derived)
        print(f"({n}, {D}, {B}): max_z |psi_out - psi_in| = {e:.1f} EPS64 (C {Cp:.0f}, float64 mirror {r64:.1f})")
        assert e <= Cp                                            # + psi: the sign is kept
    # schmidt and rank agree with bornvi_mps_canonicalise on the same cores (its values over all D of them; here over the kept)
    _, sch_c, _, rank_c, _, st_c = backend.mps_canonicalise(t_(c))
    can64, canld = cm.canonicalise(c), cm.canonicalise(c, dtype=cm.LD)
    Cs = hp.measured_constant(units(m64["schmidt"], mld["schmidt"]), derived) + \
        hp.measured_constant(units(can64["schmidt"], canld["schmidt"]), cm.derived_constant(n, D))
    es = units(g["schmidt"], sch_c.cpu().numpy())
    print(f"    schmidt against the canonicaliser's: {es:.1f} EPS64 (C {Cs:.0f}); ranks {g['rank'].tolist()}")
    assert int(st_c.item()) == 0 and np.array_equal(g["rank"], rank_c.cpu().numpy()) and np.array_equal(g["rank"], mld["rank"])
    assert es <= Cs
    # every loss[j] is -sum_b w_b log q(z_b)
    w = np.full(B, 1.0 / B)
    lq, lqb = score_logq(c, idx, w)
    want = -math.fsum((w * lq).tolist())
    Cl = hp.measured_constant(units(m64["loss"], mld["loss"], mld["loss_scale"]), derived)
    bound = EPS * (float((w * lqb).sum()) + float((w * np.abs(lq)).sum()) + Cl * hp.to_f64(mld["loss_scale"]))
    worst = float((np.abs(g["loss"] - want) / bound).max())
    print(f"    loss[j] against -sum w logq of the score call: worst error / bound = {worst:.3f} (C {Cl:.0f})")
    assert worst <= 1.0


# ---- 2. lr > 0 against the extended mirror -------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,B", SHAPES)
@pytest.mark.parametrize("steps,keep_less,cutoff", [(1, 0, 0.0), (3, 1, 1e-3)])
def test_descent_steps_against_the_extended_mirror(n, D, B, steps, keep_less, cutoff):
    keep = max(1, D - keep_less)
    r = case(n, D, B, 0.02, steps, keep, cutoff)
    g, m64, mld = r["gpu"], r["m64"], r["mld"]
    derived = tm.derived_constant(n, D, steps)
    assert mld["gap"] > 1e-6 and m64["gap"] > 1e-6               # conditions on the inputs: no value sits at the cut, and the
    assert np.array_equal(m64["rank"], mld["rank"])               # two mirrors cut alike
    assert g["status"] == 0 and mld["status"] == 0
    assert np.array_equal(g["rank"], mld["rank"]), (g["rank"], mld["rank"])
    out = []
    for name, scale in (("loss", mld["loss_scale"]), ("schmidt", None), ("discarded", None)):
        Cq = hp.measured_constant(units(m64[name], mld[name], scale), derived)
        e = units(g[name], mld[name], scale)
        out.append(f"{name} {e:.1f} (C {Cq:.0f})")
        assert e <= Cq, (name, e, Cq)
    if n <= 12:
        ref = cm.psi_of(hp.to_f64(mld["cores"]))[0]
        own = float(np.abs(hp.to_f64(mld["cores"]).astype(tm.LD) - mld["cores"]).max() / tm.LD(EPS))      # rounding the reference's cores
        r64 = float(np.abs(cm.psi_of(hp.to_f64(m64["cores"]))[0] - ref).max() / tm.LD(EPS))
        e = float(np.abs(cm.psi_of(g["cores"])[0] - ref).max() / tm.LD(EPS))
        Cp = hp.measured_constant(r64, derived) + n * own
        out.append(f"psi {e:.1f} (C {Cp:.0f}, float64 mirror {r64:.1f})")
        assert e <= Cp
    print(f"({n}, {D}, {B}) steps {steps} keep {keep} cutoff {cutoff}: ranks {g['rank'].tolist()}; EPS64: " + "; ".join(out))
    assert np.all(g["schmidt"] >= 0) and np.all(np.diff(g["schmidt"], axis=1) <= 0)
    for k in range(1, n):
        assert np.all(g["schmidt"][k - 1, int(g["rank"][k - 1]):] == 0.0)


# ---- 3. the entry gauge again ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,B", SHAPES)
def test_output_is_canonical_with_exact_zeros(n, D, B):
    keep = max(1, D - 1)
    r = case(n, D, B, 0.02, 3, keep, 1e-3)
    g, m64 = r["gpu"], r["m64"]
    out = g["cores"]
    derived = tm.derived_constant(n, D, 3)
    assert np.all(out[0, :, 1:, :] == 0.0) and np.all(out[n - 1, :, :, 1:] == 0.0)
    worst_g = worst_m = 0.0
    for k in range(2, n + 1):
        rk = int(g["rank"][k - 2])
        assert np.all(out[k - 1, :, rk:, :] == 0.0) and np.all(out[k - 2, :, :, rk:] == 0.0)
        for o, which in ((out, "g"), (hp.to_f64(m64["cores"]), "m")):
            A = o[k - 1].astype(cm.LD)
            d = float(np.abs(A[0] @ A[0].T + A[1] @ A[1].T - np.eye(D, dtype=cm.LD))[:rk, :rk].max() / cm.LD(EPS))
            if which == "g":
                worst_g = max(worst_g, d)
            else:
                worst_m = max(worst_m, d)
    Cg = hp.measured_constant(worst_m, derived)
    env = sm.environments(out)
    logZ = float(backend.mps_environments(g["dev_cores"], 1).item())
    env_bound = EPS * (tk.c_env(n, D) * float(env["Z_abs"] / env["Z"]) + 8 * (abs(float(np.log(env["Z"]))) + 4))
    print(f"({n}, {D}, {B}): gauge {worst_g:.1f} EPS64 (C {Cg:.0f}); log Z of the output {logZ:.2e} (bound {env_bound + 2 * Cg * EPS:.2e})")
    assert worst_g <= Cg
    assert abs(logZ) <= env_bound + 2 * Cg * EPS


# ---- 4. weights and reproducibility -----------------------------------------------------------------------------------
def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("cores", "loss", "schmidt", "discarded", "rank")) and a["status"] == b["status"]


@pytest.mark.parametrize("n,D,B", [(3, 3, 65), (12, 16, 1000), (5, 4, 16449)])
def test_null_weights_two_calls_and_a_replayed_graph_are_bitwise_equal(n, D, B):
    c, idx = inputs(n, D, B)
    a = run(c, idx, None, 0.02, 2, None, 1e-6)
    assert same_bytes(a, run(c, idx, np.full(B, 1.0 / B), 0.02, 2, None, 1e-6))
    assert same_bytes(a, run(c, idx, None, 0.02, 2, None, 1e-6))
    ct, it = t_(c), t_(idx, torch.int64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        backend.mps_twosite_sweep(ct.clone(), it, None, 0.02, 2, None, 1e-6)      # warm-up: the side stream's workspace exists before capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    work = ct.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = backend.mps_twosite_sweep(work, it, None, 0.02, 2, None, 1e-6)
    for t in captured:
        t.zero_()
    work.copy_(ct)
    graph.replay()
    torch.cuda.synchronize()
    got = dict(zip(("loss", "schmidt", "discarded", "rank"), (x.cpu().numpy() for x in captured[:4])), cores=work.cpu().numpy(),
               status=int(captured[4].item()))
    assert same_bytes(a, got)


# ---- 5. bad inputs ------------------------------------------------------------------------------------------------
def test_status_2_leaves_the_sample_out():
    n, D = 5, 3
    rng = np.random.default_rng(9)
    prod = np.zeros((n, 2, D, D))
    prod[:, :, 0, 0] = rng.uniform(0.3, 1.0, (n, 2))
    prod[2, 1] = 0.0                                              # site 3 never takes the value 1
    prod /= np.sqrt((prod[:, :, 0, 0] ** 2).sum(axis=1))[:, None, None, None]      # every site normalised: canonical, Z = 1
    good = np.array([0b00000, 0b10010, 0b01001, 0b11011, 0b00010, 0b11000, 0b01011], dtype=np.int64)
    idx = np.insert(good, 3, 0b00100)                             # a sample with a 1 at site 3: psi = 0 at every bond
    B = len(idx)
    w = np.full(B, 1.0 / B)
    g = run(prod, idx, None, 0.05, 2, None, 0.0)
    mld = tm.sweep(prod, good, w=w[:len(good)], lr=0.05, steps=2, dtype=tm.LD)       # the mirror with that sample dropped
    m64 = tm.sweep(prod, good, w=w[:len(good)], lr=0.05, steps=2)
    assert g["status"] == 2 and mld["status"] == 0
    assert all(np.all(np.isfinite(g[k])) for k in ("cores", "loss", "schmidt", "discarded"))
    derived = tm.derived_constant(n, D, 2)
    assert np.array_equal(g["rank"], mld["rank"])
    for name, scale in (("loss", mld["loss_scale"]), ("schmidt", None), ("discarded", None)):
        assert units(g[name], mld[name], scale) <= hp.measured_constant(units(m64[name], mld[name], scale), derived), name
    ref = cm.psi_of(hp.to_f64(mld["cores"]))[0]
    r64 = float(np.abs(cm.psi_of(hp.to_f64(m64["cores"]))[0] - ref).max() / tm.LD(EPS))
    assert float(np.abs(cm.psi_of(g["cores"])[0] - ref).max() / tm.LD(EPS)) <= hp.measured_constant(r64, derived) + n


def test_status_1_and_status_8():
    c, idx = inputs(6, 5, 200)
    bad = c.copy()
    bad[3, 1, 2, 1] = np.nan
    g = run(bad, idx, None, 0.02, 1)
    assert g["status"] & 1
    assert all(np.all(np.isnan(g[k])) for k in ("cores", "loss", "schmidt", "discarded")) and np.all(g["rank"] == 0)
    g = run(1.01 * c, idx, None, 0.0, 1)                          # un-normalised on entry: the call completes
    assert g["status"] == 8 and all(np.all(np.isfinite(g[k])) for k in ("cores", "loss", "schmidt", "discarded"))
    assert tm.sweep(1.01 * c, idx, lr=0.0, steps=1)["status"] == 8


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_refused_arguments_touch_nothing():
    lib = _ext.lib()
    h = _ext.handle_for(dev())
    size = lib.bornvi_mps_twosite_workspace_bytes
    assert size(h.h, 1, 4, 10) == 0 and size(h.h, 64, 4, 10) == 0 and size(h.h, 4, 0, 10) == 0 and size(h.h, 4, 17, 10) == 0
    assert size(h.h, 4, 4, 0) == 0 and size(h.h, 4, 4, (1 << 20) + 1) == 0
    n, D, B = 5, 4, 70
    need = size(h.h, n, D, B)
    assert need > 0
    c, idx = inputs(n, D, B)
    ct, it = t_(c), t_(idx, torch.int64)
    buf = torch.full((need + 4096,), 7, dtype=torch.uint8, device=dev())
    outs = torch.full((4096,), 7.0, dtype=torch.float64, device=dev())
    ints = torch.full((64,), 7, dtype=torch.int32, device=dev())
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(n_=n, D_=D, B_=B, lr=0.1, steps=2, keep=D, cutoff=0.0, nbytes=need):
        return lib.bornvi_mps_twosite_sweep(h.h, n_, D_, B_, p(ct), p(it), None, C.c_double(lr), steps, keep, C.c_double(cutoff), p(outs),
                                            p(outs, 8192), p(outs, 16384), p(ints), p(ints, 128), p(buf), nbytes, None)
    for kw in (dict(n_=1), dict(n_=64), dict(D_=0, keep=1), dict(D_=17, keep=4), dict(B_=0), dict(B_=(1 << 20) + 1), dict(steps=0), dict(steps=65),
               dict(keep=0), dict(keep=D + 1), dict(lr=-1e-300), dict(lr=float("nan")), dict(lr=float("inf")), dict(cutoff=-1e-300),
               dict(cutoff=1.0), dict(cutoff=float("nan")), dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**kw) == UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert bool((outs == 7.0).all()) and bool((ints == 7).all()) and bool((buf == 7).all())       # nothing was launched
    assert np.array_equal(ct.cpu().numpy(), c) and np.array_equal(it.cpu().numpy(), idx)
    assert call() == 0
    torch.cuda.synchronize()
    assert int(ints[32].item()) == 0


# ---- 7. once at full size ---------------------------------------------------------------------------------------------
def test_full_size():
    """(63, 16, 2^20), lr = 0, one step: the vectors' buffer is 8.4 GB, so a 32-bit offset anywhere shows.  The samples are 1024
    draws from q, each repeated 1024 times (sample b and b + 1024 j are the same state), so that the references cost 1024
    samples: loss[0] against -mean logq of bornvi_mps_score_vjp on the input cores, loss[last] against the same on the output
    cores (with lr = 0 the same state), each within the score call's own bound plus this call's: the psi chain against the
    sample's condition number, and one factorisation's norm-wise error C_bond EPS64 times |l_b| |r_b| / |psi_b|."""
    n, D, B, R = 63, 16, 1 << 20, 1024
    c, base = inputs(n, D, R)
    idx = np.tile(base, B // R)
    ct, it = t_(c), t_(idx, torch.int64)
    loss, schmidt, discarded, rank, status = backend.mps_twosite_sweep(ct, it, None, 0.0, 1)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    loss = loss.cpu().numpy()
    wfull = torch.full((B,), 1.0 / B, dtype=torch.float64, device=dev())
    c_bond = (tm.derived_constant(n, D, 1) - 8) / (2 * (n - 1))
    for j, cores_t in ((0, t_(c)), (len(loss) - 1, ct)):
        backend.mps_environments(cores_t, B)
        lq = backend.mps_score_vjp(cores_t, it, wfull)[1]
        assert bool((lq[:R].repeat(B // R) == lq).all())
        lq = lq[:R].cpu().numpy()
        cores_np = cores_t.cpu().numpy()
        bits = tm.bits_of(base, n)
        ref = sm.conditionals(cores_np, bits)
        env = sm.environments(cores_np)
        kb = hp.to_f64(ref["psi_abs"] / np.abs(ref["psi"]))
        lqb = tk.logq_bound(n, D, kb, float(env["Z_abs"] / env["Z"]), hp.to_f64(ref["logq"]), float(np.log(env["Z"])))
        r = np.zeros((R, D))
        r[:, 0] = 1.0
        for k in range(n, 2, -1):                                 # |r_b| at bond 1, where l_b = e0
            r = np.einsum("bac,bc->ba", cores_np[k - 1][bits[:, k - 1]], r)
        cond = np.sqrt((r * r).sum(axis=1)) / np.abs(hp.to_f64(ref["psi"]))
        bound = EPS * float((lqb + 2 * (n * D + D * D + 4) * kb + 2 * c_bond * cond + np.abs(lq) + 8).mean())
        want = -math.fsum(lq.tolist()) / R
        print(f"loss[{j}] = {loss[j]:.12f}, -mean logq = {want:.12f}: error / bound = {abs(loss[j] - want) / bound:.3f}")
        assert abs(loss[j] - want) <= bound
