"""The circuit engines against the extended-precision reference of circuit_hp.py, per entry: circuit_pass_r3_kernel (8
amplitudes per thread, pivot-normalised records, scale), circuit_pass_fast_kernel and circuit_pass_kernel (16 amplitudes),
build_gates_kernel, the fused-dot last pass, shift_dot_kernel and the adjoint walk.  Every bound is derived in circuit_hp's
docstring from the kernels' operation chains; a correct kernel stays at or below a ratio of 1, and every test prints its
worst ratio beside the constant.  No global maximum appears in an assertion.

Every case runs under both values of reg_wires.  Shapes are the smallest at which a path changes: fewer wires than register
wires (n = 1, 2, 3), tiles too small for the compact tables (n = 5; from 2^6 they build), single-pass plans (8 ... 13),
forced multi-pass plans through tile_bits, the first default multi-pass size, read_map 0 and 1 at the multi-pass shapes, a
batch of several tiles per workgroup, and the deep plan whose fused-gate count is past what the pivot-normalised kernel's
scale can hold in fp64 (plan.hpp: R3_MAX_FUSED).  References are computed once per case and shared."""
import numpy as np
import pytest
import torch

import circuit_hp as ch
from hp_reference import LD, to_f64
from oracle import circuit as oc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ch.unavailable() is not None, reason=str(ch.unavailable()))]

SINGLE = [(1, 1, 0), (2, 2, 0), (3, 2, 0), (5, 2, 0), (6, 2, 0), (8, 2, 0), (10, 2, 0), (12, 2, 0), (13, 2, 0)]
FORCED = [(9, 3, 6), (12, 2, 9), (14, 3, 11)]
LARGE_FAMILIES = ("uniform", "init", "mixed", "tie")          # n >= 14: a reference costs 0.3 s


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(params=[3, 4], ids=["r3", "r4"])
def be(dev, request):
    from tensornetworks_amd import backend
    defaults = {k: backend.get_option(dev, k) for k in ("reg_wires", "read_map")}
    backend.set_option(dev, "reg_wires", request.param)
    yield backend
    backend.set_option(dev, "tile_bits", 13)
    backend.set_option(dev, "tile_bits_multi", 0)
    for k, v in defaults.items():
        backend.set_option(dev, k, v)


def first_multi_pass_size(ansatz, L=2):
    """Smallest n whose default plan of this ansatz has more than one pass under either pass kernel (read off the planner)."""
    from tensornetworks_amd import _ext
    for n in range(1, 20):
        if any(int(_ext.plan_words(_ext.ANSATZ_IDS[ansatz], n, L, f)[3]) > 1 for f in (_ext.R3, 0)):
            return n
    raise AssertionError("no multi-pass plan below n = 20")


def configure(be, dev, kb, read_map):
    """Sets the tile and the read map; -> the flags the planner's describe calls take for the same plan."""
    be.set_option(dev, "tile_bits", kb if kb else 13)
    be.set_option(dev, "read_map", read_map)
    return kb | (0x100 if read_map else 0)


def constants(be, dev, ansatz, n, L, flags, state=False):
    """Constants of the kernel that runs this plan: the 8-amplitude one under reg_wires = 3 where the plan is eligible
    (bornvi_plan_compact_describe), else a 16-amplitude one; state plans always take the latter."""
    from tensornetworks_amd import _ext
    r3 = (not state and be.get_option(dev, "reg_wires") == 3
          and _ext.plan_compact_words(_ext.ANSATZ_IDS[ansatz], n, L, flags)[0] is not None)
    C = ch.plan_constants(ansatz, n, L, "r3" if r3 else "r4", flags)
    C["engine"] = "r3" if r3 else "r4"
    return C


def families_for(n):
    return ch.FAMILIES + ("all_half_pi",) if n < 14 else LARGE_FAMILIES


def thetas_of(ansatz, n, L):
    P = oc.num_params(ansatz, n, L)
    return np.stack([ch.angles(f, P, seed=n, ansatz=ansatz) for f in families_for(n)])


def finite(x, what):
    """The device output as a NumPy array, after asserting that every entry of it is finite."""
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert np.isfinite(x).all(), f"{what}: {int((~np.isfinite(x)).sum())} non-finite entries"
    return x


def report(what, C, worst):
    tail = ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
    print(f"{what} [{C['engine']}, {C['n_passes']} pass(es), {C['n_fused']} fused gates, C_psi {C['C_psi']:.0f}, C_q {C['C_q']:.0f}] "
          f"worst ratio of 1: {tail}")


def check_probs(be, dev, ansatz, n, L, kb, read_map, repeat=1):
    flags = configure(be, dev, kb, read_map)
    C = constants(be, dev, ansatz, n, L, flags)
    ths = thetas_of(ansatz, n, L)
    q = finite(be.circuit_probs(ansatz, n, L, torch.from_numpy(np.tile(ths, (repeat, 1))).to(dev)), "circuit_probs")
    worst = {}
    for b, fam in enumerate(families_for(n)):
        ref = ch.cached_reference(ansatz, n, L, ths[b])
        worst[fam] = ch.fold(ch.worst_ratio(ch.q_ratio(q[b], ref, C["C_psi"], C["C_q"])), ch.sum_ratio(q[b], ref, C["C_psi"], C["C_q"]))
    report(f"circuit_probs {ansatz} n={n} L={L} tile_bits={kb} read_map={read_map}", C, worst)
    assert ch.fold(*worst.values()) <= 1.0, worst
    return q, ths


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb", SINGLE)
def test_probs_single_pass(be, dev, ansatz, n, L, kb):
    check_probs(be, dev, ansatz, n, L, kb, 1 if be.get_option(dev, "reg_wires") == 3 else 0)


@pytest.mark.parametrize("read_map", [0, 1])
@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb", FORCED + [(None, 2, 0)])
def test_probs_multi_pass(be, dev, ansatz, n, L, kb, read_map):
    """(n = None: the first default multi-pass size.)"""
    n = first_multi_pass_size(ansatz, L) if n is None else n
    check_probs(be, dev, ansatz, n, L, kb, read_map)


def test_probs_several_tiles_per_workgroup(be, dev):
    """1024 circuits of 8 tiles each (n = 12, 2^9 tiles): more tiles than the persistent grids have workgroups.  Every
    copy of a circuit gives the same bits, whichever workgroup and trip computes it."""
    ansatz, n, L = "hardware_efficient", 12, 2
    q, ths = check_probs(be, dev, ansatz, n, L, 9, 1, repeat=128)
    R = len(ths)
    assert q.shape[0] == 128 * R
    for r in range(1, 128):
        assert np.array_equal(q[r * R:(r + 1) * R].view(np.int64), q[:R].view(np.int64)), r


# ------------------------------------------------------------------------------------------------ states
@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb", [(1, 1, 0), (2, 2, 0), (3, 2, 0), (5, 2, 0), (6, 2, 0), (8, 2, 0), (10, 2, 0), (13, 2, 0), (9, 3, 6),
                                    (12, 2, 9), (14, 3, 11), (None, 2, 0)])
def test_states_per_entry(be, dev, ansatz, n, L, kb):
    """paramshift_states (base row, pi-shifted rows of the first, a middle and the last parameter) and adjoint_state:
    real and imaginary part of every amplitude; no global phase is removed."""
    n = first_multi_pass_size(ansatz, L) if n is None else n
    flags = configure(be, dev, kb, 1 if be.get_option(dev, "reg_wires") == 3 else 0)
    C = constants(be, dev, ansatz, n, L, flags, state=True)
    A = ch.adjoint_constants(ansatz, n, L)
    P = oc.num_params(ansatz, n, L)
    worst = {}
    for fam in families_for(n):
        theta = ch.angles(fam, P, seed=n, ansatz=ansatz)
        th = torch.from_numpy(theta).to(dev)
        rows = [(None, be.paramshift_states(ansatz, n, L, th, 0, 0, include_base=True)[0])]
        for p in sorted({0, P // 2, P - 1}):
            rows.append((p, be.paramshift_states(ansatz, n, L, th, p, p + 1, include_base=False)[0]))
        r = 0.0
        for p, got in rows:
            ref = ch.cached_reference(ansatz, n, L, theta if p is None else ch.shifted(theta, p, np.pi))
            r = ch.fold(r, ch.worst_ratio(ch.amp_ratio(finite(torch.view_as_real(got), "paramshift_states").view(np.complex128)[:, 0], ref, C["C_psi"])))
        state, probs = be.adjoint_state(ansatz, n, L, th)
        ref = ch.cached_reference(ansatz, n, L, theta)
        ra = ch.fold(ch.worst_ratio(ch.amp_ratio(finite(torch.view_as_real(state), "adjoint_state").view(np.complex128)[:, 0], ref, A["C_psi"])),
                     ch.worst_ratio(ch.q_ratio(finite(probs, "adjoint_state probs"), ref, A["C_psi"], A["C_q"])))
        worst[fam + "/states"] = r
        worst[fam + "/adjoint"] = ra
    report(f"states {ansatz} n={n} L={L} tile_bits={kb} (adjoint C_psi {A['C_psi']:.0f})", C, worst)
    assert ch.fold(*worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ shifted rows, gradients
@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb", [(2, 2, 0), (6, 2, 0), (10, 2, 0), (9, 3, 6), (12, 2, 9), (14, 3, 11)])
def test_paramshift_rows_per_entry(be, dev, ansatz, n, L, kb):
    """paramshift_probs: the (+, -) rows of the first, a middle and the last parameter."""
    flags = configure(be, dev, kb, 1 if be.get_option(dev, "reg_wires") == 3 else 0)
    C = constants(be, dev, ansatz, n, L, flags)
    P = oc.num_params(ansatz, n, L)
    worst = {}
    for fam in families_for(n):
        theta = ch.angles(fam, P, seed=n, ansatz=ansatz)
        th = torch.from_numpy(theta).to(dev)
        r = 0.0
        for p in sorted({0, P // 2, P - 1}):
            got = finite(be.paramshift_probs(ansatz, n, L, th, p, p + 1, include_base=False), "paramshift_probs")
            for row, s in ((0, np.pi / 2), (1, -np.pi / 2)):
                ref = ch.cached_reference(ansatz, n, L, ch.shifted(theta, p, s))
                r = ch.fold(r, ch.worst_ratio(ch.q_ratio(got[row], ref, C["C_psi"], C["C_q"])))
        worst[fam] = r
    report(f"paramshift_probs {ansatz} n={n} L={L} tile_bits={kb}", C, worst)
    assert ch.fold(*worst.values()) <= 1.0, worst


def weights(n, seed):
    """dL/dq of mixed scale: normal entries times 1, 1e-3 or 1e-6."""
    rng = np.random.default_rng([seed, n, 41])
    return rng.standard_normal(1 << n) * rng.choice([1.0, 1e-3, 1e-6], 1 << n)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L,kb,stride", [(3, 2, 0, 1), (8, 2, 0, 1), (8, 2, 0, 5), (9, 3, 6, 5), (12, 2, 9, 7)])
def test_paramshift_grad_per_parameter(be, dev, ansatz, n, L, kb, stride):
    """paramshift_grad (stored rows, then bornvi_ksd_grad_finish) over the full range (stride 1) or a strided share."""
    flags = configure(be, dev, kb, 1 if be.get_option(dev, "reg_wires") == 3 else 0)
    C = constants(be, dev, ansatz, n, L, flags)
    P = oc.num_params(ansatz, n, L)
    w = weights(n, 1)
    worst = {}
    for fam in ch.FAMILIES:
        theta = ch.angles(fam, P, seed=n, ansatz=ansatz)
        g = finite(be.paramshift_grad(ansatz, n, L, torch.from_numpy(theta).to(dev), torch.from_numpy(w).to(dev), 1 if stride > 1 else 0, P,
                                      p_stride=stride), "paramshift_grad")
        params = range(1 if stride > 1 else 0, P, stride)
        ref, allowed = ch.grad_reference(ansatz, n, L, theta, w, params, C["C_psi"], C["C_q"], ch.c_dot_rows(n))
        worst[fam] = ch.worst_ratio(ch.allowed_ratio(g, ref, allowed))
    report(f"paramshift_grad {ansatz} n={n} L={L} tile_bits={kb} stride={stride} ({len(params)} parameters, C_dot {ch.c_dot_rows(n):.0f})", C, worst)
    assert ch.fold(*worst.values()) <= 1.0, worst


@pytest.mark.parametrize("read_map", [0, 1])
def test_fused_dot_per_parameter(dev, read_map):
    """paramshift_dot_begin / _finish at n = 14, L = 3, 2^11 tiles (three passes; the 8-amplitude kernel only): q of the base
    circuit per entry, and the gradient of every 11th parameter from parameter 2 on -- 12 of the 126, whose 24 shifted
    long-double references take about 8 s of host time (once: both read maps share them)."""
    from tensornetworks_amd import backend as be
    ansatz, n, L, kb, stride = "hardware_efficient", 14, 3, 11, 11
    saved = {k: be.get_option(dev, k) for k in ("reg_wires", "read_map", "prefix_share")}
    try:
        be.set_option(dev, "reg_wires", 3)
        be.set_option(dev, "prefix_share", 0)
        flags = configure(be, dev, kb, read_map)
        C = constants(be, dev, ansatz, n, L, flags)
        P = oc.num_params(ansatz, n, L)
        params = range(2, P, stride)
        assert C["engine"] == "r3" and len(params) == 12 and be.paramshift_dot_supported(ansatz, n, L, dev, len(params))
        theta, w = ch.angles("init", P, seed=n), weights(n, 2)
        q, token = be.paramshift_dot_begin(ansatz, n, L, torch.from_numpy(theta).to(dev), 2, P, p_stride=stride)
        _, g = be.paramshift_dot_finish(token, torch.from_numpy(w).to(dev))
        base = ch.cached_reference(ansatz, n, L, theta)
        rq = ch.worst_ratio(ch.q_ratio(finite(q, "fused dot q"), base, C["C_psi"], C["C_q"]))
        C_dot = ch.c_dot_fused(n, kb)
        ref, allowed = ch.grad_reference(ansatz, n, L, theta, w, params, C["C_psi"], C["C_q"], C_dot)
        rg = ch.worst_ratio(ch.allowed_ratio(finite(g, "fused dot gradient"), ref, allowed))
        report(f"fused dot {ansatz} n={n} L={L} tile_bits={kb} read_map={read_map} (12 parameters, C_dot {C_dot:.0f})", C, {"q": rq, "grad": rg})
        assert ch.fold(rq, rg) <= 1.0
    finally:
        be.set_option(dev, "tile_bits", 13)
        for k, v in saved.items():
            be.set_option(dev, k, v)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L", [(1, 2), (3, 2), (8, 2), (11, 2)])
def test_adjoint_vjp_per_parameter(dev, ansatz, n, L):
    """bornvi_adjoint_vjp against the adjoint walk in long double (circuit_hp.adjoint_gradient: unlike the parameter-shift
    difference it does not cancel, so it resolves the gradients far below eps sum |w| q that the envelope arm bounds), under
    the two-armed bound of the backward walk (circuit_hp.adjoint_vjp_allowed).  That reference is tied to the independent
    definition of the gradient on the host: test_circuit_precision_host.py asserts, per parameter, that it agrees with the
    long-double parameter-shift difference to that difference's own derived error."""
    from tensornetworks_amd import backend as be
    P = oc.num_params(ansatz, n, L)
    w = weights(n, 3)
    worst = {}
    for fam in ch.FAMILIES:
        theta = ch.angles(fam, P, seed=n, ansatz=ansatz)
        th = torch.from_numpy(theta).to(dev)
        state, _ = be.adjoint_state(ansatz, n, L, th, want_probs=False)
        g = finite(be.adjoint_vjp(ansatz, n, L, th, state, torch.from_numpy(w).to(dev)), "adjoint_vjp")
        ref = ch.adjoint_gradient(ansatz, n, L, theta, w)
        worst[fam] = ch.worst_ratio(ch.allowed_ratio(g, ref, ch.adjoint_vjp_allowed(ansatz, n, L, theta, w)))
    A = ch.adjoint_constants(ansatz, n, L)
    print(f"adjoint_vjp {ansatz} n={n} L={L} [C_f {A['C_psi']:.0f}] worst ratio of 1: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert ch.fold(*worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ bitwise
@pytest.mark.parametrize("n,L,kb", [(3, 2, 0), (10, 2, 0), (12, 2, 9)])
def test_second_call_and_unaligned_views_are_bitwise_equal(be, dev, n, L, kb):
    """The same inputs give the same bits on a second call, and from a contiguous view that starts 8 bytes into a larger
    buffer (not 16-byte aligned): circuit_probs, paramshift_probs, paramshift_grad, paramshift_states."""
    ansatz = "hardware_efficient"
    configure(be, dev, kb, 1 if be.get_option(dev, "reg_wires") == 3 else 0)
    P = oc.num_params(ansatz, n, L)
    theta = torch.from_numpy(ch.angles("mixed", P, seed=n)).to(dev)
    w = torch.from_numpy(weights(n, 4)).to(dev)
    odd_t = torch.zeros(P + 3, dtype=torch.float64, device=dev)[1:P + 1].copy_(theta)
    odd_w = torch.zeros((1 << n) + 3, dtype=torch.float64, device=dev)[1:(1 << n) + 1].copy_(w)
    assert odd_t.data_ptr() % 16 == 8 and odd_w.data_ptr() % 16 == 8 and odd_t.is_contiguous()
    calls = {
        "circuit_probs": lambda t, v: be.circuit_probs(ansatz, n, L, t.view(1, P)),
        "paramshift_probs": lambda t, v: be.paramshift_probs(ansatz, n, L, t, 0, min(P, 4)),
        "paramshift_grad": lambda t, v: be.paramshift_grad(ansatz, n, L, t, v, 0, P),
        "paramshift_states": lambda t, v: torch.view_as_real(be.paramshift_states(ansatz, n, L, t, 0, min(P, 4))),
    }
    for name, f in calls.items():
        first = f(theta, w).clone()
        assert torch.equal(first.view(torch.int64), f(theta, w).view(torch.int64)), name + ": second call"
        assert torch.equal(first.view(torch.int64), f(odd_t, odd_w).view(torch.int64)), name + ": unaligned view"


# ------------------------------------------------------------------------------------------------ the deep plan
DEEP = ("hardware_efficient", 9, 125, 8)


def test_deep_plan_is_multi_pass_and_past_the_scale_range():
    """No GPU: the plan the 8-amplitude kernel would be given has more than 1074 fused gates (2^-1074 is fp64's smallest
    subnormal and |p|^2 can be 1/2 per gate), and bornvi_plan_compact_describe now refuses it."""
    from tensornetworks_amd import _ext
    ansatz, n, L, kb = DEEP
    W = _ext.plan_words(_ext.ANSATZ_IDS[ansatz], n, L, kb | _ext.R3)
    assert int(W[3]) > 1 and int(W[4]) > 1074, (int(W[3]), int(W[4]))
    assert _ext.plan_compact_words(_ext.ANSATZ_IDS[ansatz], n, L, kb)[0] is None


NEAR_LIMIT = ("hardware_efficient", 9, 111, 8)          # 999 fused gates: the deepest such plan the 8-amplitude kernel still runs


@pytest.mark.parametrize("family", ["all_half_pi", "tie"])
@pytest.mark.parametrize("case", [DEEP, NEAR_LIMIT], ids=["past", "below"])
def test_deep_plan_probs(be, dev, case, family):
    """hardware_efficient, n = 9, 2^8 tiles.  L = 125: 1125 fused gates.  With every angle pi/2 each |p|^2 is 1/2: under
    the pivot-normalised kernel scale = 2^-1125 would underflow to 0 and |x|^2 overflow (q = inf * 0 = nan).  reg_wires = 4
    is the control; under reg_wires = 3 the plan is past R3_MAX_FUSED and runs on the 16-amplitude kernel too.  L = 111:
    999 fused gates, just inside the limit: under reg_wires = 3 the 8-amplitude kernel runs it with scale down to 2^-999
    and |x|^2 up to 2^999, and its q is finite and inside the same bounds."""
    ansatz, n, L, kb = case
    flags = configure(be, dev, kb, 1 if be.get_option(dev, "reg_wires") == 3 else 0)
    C = constants(be, dev, ansatz, n, L, flags)
    past = case == DEEP
    assert C["n_passes"] > 1 and (C["n_fused"] > 1074 if past else ch.r3_max_fused() - 9 < C["n_fused"] <= ch.r3_max_fused())
    assert C["engine"] == ("r3" if be.get_option(dev, "reg_wires") == 3 and not past else "r4")
    theta = ch.angles(family, oc.num_params(ansatz, n, L), seed=n, ansatz=ansatz)
    q = finite(be.circuit_probs(ansatz, n, L, torch.from_numpy(theta[None]).to(dev)), "deep plan q")[0]
    ref = ch.cached_reference(ansatz, n, L, theta)
    bound = to_f64(ch.q_allowed(ref, C["C_psi"], C["C_q"]))
    r = ch.fold(ch.worst_ratio(ch.q_ratio(q, ref, C["C_psi"], C["C_q"])), ch.sum_ratio(q, ref, C["C_psi"], C["C_q"]))
    report(f"deep plan L={L} {family} (largest allowed |dq| {bound.max():.3g})", C, {"q": r})
    assert bound.max() < 1e-10 and r <= 1.0


KERNEL_CHOICE = [("hardware_efficient", 5, 2, 0), ("hardware_efficient", 6, 2, 0), ("all_to_all", 12, 2, 9), ("basic", 14, 3, 11),
                 NEAR_LIMIT, DEEP]


@pytest.mark.parametrize("ansatz,n,L,kb", KERNEL_CHOICE)
def test_get_plan_runs_the_kernel_the_describe_call_names(dev, ansatz, n, L, kb):
    """What get_plan launched, seen from outside: where a plan is not eligible for the 8-amplitude kernel, reg_wires = 3
    falls back to the very plan reg_wires = 4 runs, so the two settings give the same bits; where it is eligible the
    pivot-normalised records round differently and some bits differ.  bornvi_plan_compact_describe must predict which --
    the constants of every other test in this file are chosen by it."""
    from tensornetworks_amd import _ext, backend as be
    saved = {k: be.get_option(dev, k) for k in ("reg_wires", "read_map")}
    try:
        flags = configure(be, dev, kb, 1)
        eligible = _ext.plan_compact_words(_ext.ANSATZ_IDS[ansatz], n, L, flags)[0] is not None
        th = torch.from_numpy(ch.angles("uniform", oc.num_params(ansatz, n, L), seed=n)[None]).to(dev)
        q = {}
        for r in (3, 4):
            be.set_option(dev, "reg_wires", r)
            q[r] = finite(be.circuit_probs(ansatz, n, L, th), "circuit_probs").view(np.int64)
        same = bool(np.array_equal(q[3], q[4]))
        print(f"{ansatz} n={n} L={L} tile_bits={kb}: describe says eligible={eligible}; reg_wires 3 and 4 bitwise equal: {same}")
        assert same == (not eligible)
    finally:
        be.set_option(dev, "tile_bits", 13)
        for k, v in saved.items():
            be.set_option(dev, k, v)


def test_the_fused_dot_follows_the_depth_limit(dev):
    """On the device, get_plan's choice shows through paramshift_dot_supported (true only for multi-pass plans of the
    8-amplitude kernel): n = 16 with the default tile at L = 6 (96 fused gates) and at L = 70 (1120)."""
    from tensornetworks_amd import _ext, backend as be
    he = _ext.ANSATZ_IDS["hardware_efficient"]
    saved = {k: be.get_option(dev, k) for k in ("reg_wires", "read_map", "prefix_share")}
    try:
        be.set_option(dev, "reg_wires", 3)
        be.set_option(dev, "read_map", 0)
        be.set_option(dev, "prefix_share", 0)
        for L, want in ((6, True), (70, False)):
            assert (_ext.plan_compact_words(he, 16, L, 0)[0] is not None) == want
            assert be.paramshift_dot_supported("hardware_efficient", 16, L, dev, 4) == want, L
    finally:
        for k, v in saved.items():
            be.set_option(dev, k, v)
