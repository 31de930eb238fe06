"""The circuit engines' per-entry bounds (circuit_hp.py), checked where no GPU is needed:

* the long-double reference agrees with an independent mpmath walk at n <= 5;
* the fp64 oracle (oracle.circuit.simulate) and a plain float64 mirror of the pivot-normalised recipe of
  circuit_pass_r3_kernel (records, exchange flag, scale = prod |p|^2) lie inside the bounds for every angle family and
  every shape test_gpu_circuit_precision.py uses up to n = 12 -- the worst ratio is printed per family;
* seeded mutants of the mirror leave the bounds by a wide, printed margin; for each it is stated whether the older
  check of test_gpu_circuit.py / test_gpu_r3.py (rtol 1e-10, atol 1e-14 on q; rtol 1e-9, atol 1e-12 max |g| on gradients)
  would have caught it.  The small-entry and the small-gradient mutants are ones it misses;
* every place that answers "does the 8-amplitude kernel run this plan" applies the same depth limit.
"""
import numpy as np
import pytest

import circuit_hp as ch
from hp_reference import EPS64, LD, to_f64
from oracle import circuit as oc

pytestmark = pytest.mark.skipif(ch.unavailable() is not None, reason=str(ch.unavailable()))

HOST_SHAPES = [(1, 1), (1, 2), (2, 2), (3, 2), (5, 2), (6, 2), (8, 2), (9, 3), (10, 2), (11, 2), (12, 2)]
LD_EPS = float(np.finfo(LD).eps)


# ------------------------------------------------------------------------------------------------ reference vs mpmath
def mp_walk(gates, n, theta):
    mp = ch._mp()
    N = 1 << n
    v = [mp.mpc(0)] * N
    v[0] = mp.mpc(1)
    for kind, wires, p in gates:
        if kind in ch.KIND_NAMES:
            if kind == "H":
                h = 1 / mp.sqrt(2)
                U = [[h, h], [h, -h]]
            else:
                x = mp.mpf(float(theta[p])) / 2
                c, s = mp.cos(x), mp.sin(x)
                U = {"RX": [[c, -1j * s], [-1j * s, c]], "RY": [[c, -s], [s, c]], "RZ": [[c - 1j * s, 0], [0, c + 1j * s]]}[kind]
            bit = 1 << (n - 1 - wires[0])
            for i in range(N):
                if not i & bit:
                    a, b = v[i], v[i | bit]
                    v[i], v[i | bit] = U[0][0] * a + U[0][1] * b, U[1][0] * a + U[1][1] * b
        else:
            ca, cb = 1 << (n - 1 - wires[0]), 1 << (n - 1 - wires[1])
            if kind == "CNOT":
                v = [v[i ^ (cb if i & ca else 0)] for i in range(N)]
            else:
                v = [-v[i] if (i & ca and i & cb) else v[i] for i in range(N)]
    return v


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
@pytest.mark.parametrize("n,L", [(1, 1), (3, 2), (5, 2)])
def test_reference_against_mpmath(ansatz, n, L):
    """|psi_LD - psi_mp| <= 6 G 2^-63 psi_abs per entry, G elementary gates: in long double a gate is its rounded entries
    (1) and a chain of 3 (product, sum, sum), times sqrt 2, below 6 per gate."""
    mp = ch._mp()
    worst = 0.0
    for fam in ch.FAMILIES:
        theta = ch.angles(fam, oc.num_params(ansatz, n, L), seed=3)
        ref = ch.reference(ansatz, n, L, theta)
        gates = oc.gate_list(ansatz, n, L)
        G = sum(k in ch.KIND_NAMES for k, _, _ in gates)
        for z, want in enumerate(mp_walk(gates, n, theta)):
            got = mp.mpc(mp.mpf(str(ref["psi"][z].real)), mp.mpf(str(ref["psi"][z].imag)))
            allowed = 6 * G * LD_EPS * float(ref["psi_abs"][z])
            err = float(abs(got - want))
            assert allowed > 0 or err == 0
            worst = max(worst, err / allowed if allowed > 0 else 0.0)
            assert float(ref["psi_abs"][z]) >= float(abs(want)) * (1 - 1e-15)
    print(f"{ansatz} n={n} L={L}: long double against mpmath-40, worst ratio {worst:.3g} of 6 G LD-eps psi_abs")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ oracle and mirror
def case_angles(ansatz, n, L):
    P = oc.num_params(ansatz, n, L)
    fams = [(f, ch.angles(f, P, seed=n, ansatz=ansatz)) for f in ch.FAMILIES]
    return fams + [("all_half_pi", ch.angles("all_half_pi", P)), ("peaked", ch.peaked_angles(ansatz, n, L))]


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
def test_oracle_and_mirror_lie_inside_the_bounds(ansatz):
    worst = {}
    for n, L in HOST_SHAPES:
        Co, Cm = ch.oracle_constants(ansatz, n, L), ch.mirror_constants(ansatz, n, L)
        gates = oc.gate_list(ansatz, n, L)
        for fam, theta in case_angles(ansatz, n, L):
            ref = ch.cached_reference(ansatz, n, L, theta)
            psi = oc.simulate(gates, n, theta)
            r = {"oracle psi": ch.worst_ratio(ch.amp_ratio(psi, ref, Co["C_psi"])),
                 "oracle q": ch.worst_ratio(ch.q_ratio(psi.real ** 2 + psi.imag ** 2, ref, Co["C_psi"], Co["C_q"])),
                 "mirror q": ch.worst_ratio(ch.q_ratio(ch.mirror_r3(ansatz, n, L, theta), ref, Cm["C_psi"], Cm["C_q"])),
                 "mirror sum q": ch.sum_ratio(ch.mirror_r3(ansatz, n, L, theta), ref, Cm["C_psi"], Cm["C_q"])}
            for k, v in r.items():                       # (worst_ratio and sum_ratio give inf for NaN)
                if v >= worst.get((fam, k), (-1.0,))[0]:
                    worst[(fam, k)] = (float(v), n, L, Cm["C_psi"] if "mirror" in k else Co["C_psi"])
    for (fam, k), (v, n, L, C) in sorted(worst.items()):
        print(f"{ansatz} {fam:12s} {k:13s} worst ratio {v:.3g} of 1 at n={n} L={L} (C_psi {C:.0f})")
    assert all(v[0] <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v[0] <= 1.0}


def test_small_entries_are_what_the_older_tolerance_cannot_see():
    """With the trainers' initial angles and the basic ansatz a large share of q (45 % at n = 14, L = 2) is below atol = 1e-14."""
    theta = ch.angles("init", oc.num_params("basic", 14, 2))
    q = to_f64(ch.cached_reference("basic", 14, 2, theta)["q"])
    share = float((q < 1e-14).mean())
    print(f"basic n=14 L=2 init: {100 * share:.1f} % of the entries of q are below 1e-14 (smallest {q.min():.3g})")
    assert share > 0.25


# ------------------------------------------------------------------------------------------------ mutants
def old_q_check(q, ansatz, n, L, theta):
    return bool(np.allclose(q, oc.probs(ansatz, n, L, theta), rtol=1e-10, atol=1e-14))


def q_mutant(name, ansatz, n, L, theta, arg=None):
    """(worst q ratio, worst amplitude ratio, does the older check accept it) of one mutant of the mirror."""
    ref = ch.cached_reference(ansatz, n, L, theta)
    C = ch.mirror_constants(ansatz, n, L)

    def ratios(mutant):
        q, psi = ch.mirror_r3(ansatz, n, L, theta, mutant=mutant, arg=arg, want_psi=True)
        return ch.worst_ratio(ch.q_ratio(q, ref, C["C_psi"], C["C_q"])), ch.worst_ratio(ch.amp_ratio(psi, ref, C["C_psi_state"])), q
    cq, ca, _ = ratios(None)
    rq, ra, q = ratios(name)
    old = old_q_check(q, ansatz, n, L, theta)
    print(f"mutant {name:13s} {ansatz} n={n} L={L}: worst ratio of 1: q {rq:.3g}, amplitudes {ra:.3g} (clean mirror {cq:.3g}, {ca:.3g}); "
          f"the rtol 1e-10 / atol 1e-14 check on q {'MISSES it' if old else 'catches it'}")
    assert cq <= 1.0 and ca <= 1.0
    return rq, ra, old


def test_mutant_float32_hadamard():
    rq, ra, _ = q_mutant("h32", "hardware_efficient", 6, 2, ch.angles("uniform", 36))
    assert rq > 1e3 and ra > 1e3


def test_mutant_float32_sincos():
    rq, ra, _ = q_mutant("sincos32", "hardware_efficient", 6, 2, ch.angles("uniform", 36), arg=4)
    assert rq > 1e3 and ra > 1e3


def test_mutant_sin_from_cos():
    """sin = sqrt(1 - cos^2) loses a tiny angle altogether: q's small entries become 0, which atol = 1e-14 accepts."""
    rq, ra, old = q_mutant("sin_from_cos", "basic", 6, 2, ch.angles("tiny", 24))
    assert rq > 1e3 and ra > 1e3 and old


def test_mutant_cz_sign_on_a_small_entry():
    """The first CZ of the first layer leaves unsigned the largest of its entries with |x|^2 < 1e-14.  The amplitudes show
    it by four orders.  q shows it only through the next layer's mixing (angles 1e-4), so its margin is thin: a sign on a
    small entry is a defect of the phase-coherent outputs first."""
    ansatz, n, L = "hardware_efficient", 6, 2
    theta = ch.peaked_angles(ansatz, n, L)
    rq, ra, old = q_mutant("cz_drop", ansatz, n, L, theta, arg=0)
    print(f"    (entry {ch.LAST_CZ_DROP[0]}, |x|^2 = {ch.LAST_CZ_DROP[1]:.3g} at the gate)")
    assert ra > 1e3 and rq > 1.0 and old


def test_mutant_pivot_left_out_of_scale():
    rq, _, _ = q_mutant("scale_drop", "all_to_all", 6, 2, ch.angles("uniform", 36), arg=2)
    assert rq > 1e3


def test_mutant_exchange_flag_ignored_at_a_tie():
    """basic, three layers: the states that meet the later ties are generic (a tie on |0>, or on a basis state as behind
    the Hadamards of the other ansaetze with RY = pi/2, gives two equal moduli, and q cannot tell them apart)."""
    ansatz, n, L = "basic", 6, 3
    theta = ch.angles("tie", 36, ansatz=ansatz)
    piv = ch.mirror_pivots(ansatz, n, L, theta)
    ties = [i for i, (m0, m1) in enumerate(piv) if m1 > m0 and m1 - m0 <= 4 * EPS64]
    near = [(m0, m1) for m0, m1 in piv if abs(m1 - m0) <= 4 * EPS64]
    sides = sum(m1 > m0 for m0, m1 in near), sum(m1 == m0 for m0, m1 in near), sum(m1 < m0 for m0, m1 in near)
    print(f"tie family: {len(near)} of {len(piv)} pivots within 4 eps: |u10|^2 above / equal to / below |u00|^2: {sides}")
    assert ties and ties[-1] >= 2 * n and min(sides) > 0
    rq, ra, _ = q_mutant("tie_ignore", ansatz, n, L, theta, arg=ties[-1])
    assert rq > 1e3 and ra > 1e3


def small_gradient_case():
    """basic, n = 4, L = 1 (a product state, then CNOTs): wire 0's RY is 1e-9, wire 1's 1e-4, and w is zero unless wire 0
    reads 1 -- so the gradient of wire 1's RY is about 1e-14 of the largest (wire 0's own), with little cancellation."""
    ansatz, n, L = "basic", 4, 1
    theta = np.array([1.3e-9, 0.4, 0.9e-4, -0.7, 0.8, 0.3, -1.1, 0.6])
    rng = np.random.default_rng(5)
    z = np.arange(1 << n)
    src = z
    for kind, wires, _ in oc.gate_list(ansatz, n, L):        # outcome z of the circuit reads the product state at src[z]
        if kind == "CNOT":
            src = src[ch._cnot_src(n, wires[0], wires[1])]
    w = (0.5 + rng.random(1 << n)) * ((src >> (n - 1)) & 1)
    return ansatz, n, L, theta, w, 2                          # parameter 2: wire 1's RY


def mirror_grad(ansatz, n, L, theta, w, wrong_sign_at=None):
    g = np.zeros(theta.size)
    for p in range(theta.size):
        qp = ch.mirror_r3(ansatz, n, L, ch.shifted(theta, p, np.pi / 2))
        qm = ch.mirror_r3(ansatz, n, L, ch.shifted(theta, p, np.pi / 2 if p == wrong_sign_at else -np.pi / 2))
        g[p] = 0.5 * (np.dot(w, qp) - np.dot(w, qm))
    return g


def test_mutant_shift_sign_on_a_small_gradient():
    ansatz, n, L, theta, w, p = small_gradient_case()
    C = ch.mirror_constants(ansatz, n, L)
    ref, allowed = ch.grad_reference(ansatz, n, L, theta, w, range(theta.size), C["C_psi"], C["C_q"], C_dot=(1 << n) + 2)
    share = float(abs(ref[p]) / np.abs(ref).max())
    assert 0 < share < 1e-6, share
    clean = ch.allowed_ratio(mirror_grad(ansatz, n, L, theta, w), ref, allowed)
    g = mirror_grad(ansatz, n, L, theta, w, wrong_sign_at=p)
    ratio = ch.allowed_ratio(g, ref, allowed)
    g_oracle = oc.paramshift_vjp(ansatz, n, L, theta, w)
    # (the older check at this parameter alone: at parameter 0 the fp64 oracle's own cancellation noise exceeds it)
    old = bool(abs(g[p] - g_oracle[p]) <= 1e-9 * abs(g_oracle[p]) + 1e-12 * np.abs(g_oracle).max())
    print(f"mutant shift_sign    {ansatz} n={n} L={L} parameter {p}: |g_p| / max |g| = {share:.3g}; ratio {ratio[p]:.3g} of 1 "
          f"(clean mirror, worst parameter {clean.max():.3g}); the rtol 1e-9 / atol 1e-12 max |g| check "
          f"{'MISSES it' if old else 'catches it'}")
    assert clean.max() <= 1.0 and ratio[p] > 1e3 and old


PI_2_GAP = 6.2e-17          # pi/2 - float64(pi/2) = 6.123e-17, rounded up


def shift_rule_gap_allowed(ansatz, n, L, theta, w, p):
    """How far 1/2 sum w (q+ - q-), evaluated in long double at the angles the device forms (one float64 addition of the
    float64 pi/2), may lie from the derivative d/dtheta_p sum w q.  F(t) = sum w q(theta_p = t) is A + R cos(t - t0), so
    with exact shifts the rule is exact; the formed shifts are off by at most d = PI_2_GAP + eps/2 (|theta_p| + pi/2) each,
    and |F'| <= R everywhere, R^2 = F'(theta_p)^2 + (F(theta_p) - A)^2, A = (F+ + F-) / 2: the rule is off by at most d R
    (the second order, d^2 R / 2, is below 1e-32 R).  To that add the long-double errors of the three references, by the
    bounds of this module with long double's eps: 6 per elementary gate on the amplitudes (test_reference_against_mpmath),
    3 on q, 2^n + 2 on each plain sum.  -> (allowed, R)."""
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    G = sum(k in ch.KIND_NAMES for k, _, _ in oc.gate_list(ansatz, n, L))
    scale = LD_EPS / EPS64
    C_psi, C_q, C_sum = 6 * G * scale, 3 * scale, ((1 << n) + 2) * scale
    refs = [ch.cached_reference(ansatz, n, L, t) for t in (theta, ch.shifted(theta, p, np.pi / 2), ch.shifted(theta, p, -np.pi / 2))]
    F = [(wl * r["q"]).sum() for r in refs]
    errs = [(np.abs(wl) * ch.q_allowed(r, C_psi, C_q)).sum() + LD(EPS64 * C_sum) * (np.abs(wl) * r["q"]).sum() for r in refs]
    g, A = (F[1] - F[2]) / 2, (F[1] + F[2]) / 2
    R = np.sqrt(g * g + (F[0] - A) ** 2) + errs[0] + errs[1] + errs[2]
    d = LD(PI_2_GAP) + LD(EPS64 / 2) * (abs(LD(theta[p])) + LD(np.pi / 2))
    return d * R * (1 + LD(1e-6)) + (errs[1] + errs[2]) / 2, R


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
def test_adjoint_walk_reference_and_bound(ansatz):
    """The reference of bornvi_adjoint_vjp is the adjoint walk in long double (circuit_hp.adjoint_gradient): it does not
    cancel, so it resolves gradients far below eps sum |w| q, where the parameter-shift difference cannot referee.  It is
    the same algorithm as the kernel's, so it is tied here to the independent definition of the gradient: per parameter it
    agrees with the long-double parameter-shift difference to within that difference's derived error
    (shift_rule_gap_allowed) plus its own long-double error.  A convention error in the walk (a generator's sign, a wrong
    Pauli, the order of the un-computation) shows as a gap of the size of the gradient itself.  Then a complex128
    restatement of the walk lies inside circuit_hp.adjoint_vjp_allowed around it."""
    worst, worst_gap = {}, (0.0, None)
    for n, L in [(1, 2), (3, 2), (8, 2)]:
        P = oc.num_params(ansatz, n, L)
        w = np.random.default_rng([n, 41]).standard_normal(1 << n) * np.random.default_rng([n, 42]).choice([1.0, 1e-3, 1e-6], 1 << n)
        for fam in ch.FAMILIES:
            theta = ch.angles(fam, P, seed=n, ansatz=ansatz)
            g = ch.adjoint_gradient(ansatz, n, L, theta, w)
            ps, _ = ch.grad_reference(ansatz, n, L, theta, w, range(P), 0.0, 0.0, 0.0)
            own = ch.adjoint_vjp_allowed(ansatz, n, L, theta, w) * LD(2 * LD_EPS / EPS64)
            for p in range(P):
                allowed, R = shift_rule_gap_allowed(ansatz, n, L, theta, w, p)
                gap = float(abs(ps[p] - g[p]) / (allowed + own[p])) if allowed + own[p] > 0 else (0.0 if ps[p] == g[p] else np.inf)
                if not gap <= worst_gap[0]:
                    worst_gap = (gap, f"n={n} {fam} parameter {p}: |gap| {float(abs(ps[p] - g[p])):.3g}, allowed {float(allowed + own[p]):.3g}, R {float(R):.3g}")
            r = ch.worst_ratio(ch.allowed_ratio(ch.adjoint_gradient(ansatz, n, L, theta, w, fp64=True), g, ch.adjoint_vjp_allowed(ansatz, n, L, theta, w)))
            worst[fam] = ch.fold(worst.get(fam, 0.0), r)
    print(f"{ansatz}: complex128 adjoint walk, worst ratio of 1 per family: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + f"; adjoint walk against parameter shift, worst gap / allowed {worst_gap[0]:.3g} ({worst_gap[1]})")
    assert ch.fold(*worst.values()) <= 1.0, worst
    assert worst_gap[0] <= 1.0, worst_gap


@pytest.mark.parametrize("L,inside", [(111, True), (125, False)])
def test_deep_shapes_on_the_host(L, inside):
    """hardware_efficient, n = 9, every angle pi/2 (each fused gate's |p|^2 is 1/2 from the second layer on).  The fp64
    oracle lies inside the bounds at both depths.  The float64 mirror of the pivot-normalised recipe does so at L = 111
    (999 fused gates, inside R3_MAX_FUSED: scale about 2^-990) and shows the defect at L = 125 (1125): scale underflows
    to 0, |x|^2 overflows, q is not finite -- what circuit_pass_r3_kernel returned for this plan before the limit."""
    ansatz, n = "hardware_efficient", 9
    theta = ch.angles("all_half_pi", oc.num_params(ansatz, n, L))
    ref = ch.cached_reference(ansatz, n, L, theta)
    Co, Cm = ch.oracle_constants(ansatz, n, L), ch.mirror_constants(ansatz, n, L)
    assert (Cm["n_fused"] <= R3_MAX_FUSED) == inside
    psi = oc.simulate(oc.gate_list(ansatz, n, L), n, theta)
    ro = ch.fold(ch.worst_ratio(ch.amp_ratio(psi, ref, Co["C_psi"])), ch.worst_ratio(ch.q_ratio(psi.real ** 2 + psi.imag ** 2, ref, Co["C_psi"], Co["C_q"])))
    with np.errstate(all="ignore"):
        q = ch.mirror_r3(ansatz, n, L, theta)
    rm = ch.worst_ratio(ch.q_ratio(q, ref, Cm["C_psi"], Cm["C_q"]))
    print(f"hardware_efficient n=9 L={L} all-pi/2 ({Cm['n_fused']} fused gates): oracle worst ratio {ro:.3g}; mirror: "
          f"{int(np.isfinite(q).sum())} of {q.size} entries finite, worst ratio {rm:.3g}")
    assert ro <= 1.0
    assert (np.isfinite(q).all() and rm <= 1.0) if inside else (not np.isfinite(q).all() and rm == np.inf)


@pytest.mark.parametrize("ansatz", oc.ANSATZ_TYPES)
def test_tie_family_puts_pivots_within_one_ulp_on_either_side(ansatz):
    """Of the fused gates of the tie family (n = 8, L = 4) some have |u10|^2 above |u00|^2 by at most one ulp (2^-53, the
    spacing of float64 in [1/2, 1)), some as much below, some exactly equal: the exchange flag hangs on the last bit."""
    piv = ch.mirror_pivots(ansatz, 8, 4, ch.angles("tie", oc.num_params(ansatz, 8, 4), seed=8, ansatz=ansatz))
    ulp = 2.0 ** -53
    near = [(m0, m1) for m0, m1 in piv if abs(m1 - m0) <= ulp]
    sides = sum(m1 > m0 for m0, m1 in near), sum(m1 == m0 for m0, m1 in near), sum(m1 < m0 for m0, m1 in near)
    print(f"{ansatz} tie family: {len(near)} of {len(piv)} pivots within one ulp: |u10|^2 above / equal to / below |u00|^2: {sides}")
    assert min(sides) > 0, sides


# ------------------------------------------------------------------------------------------------ the depth limit
R3_MAX_FUSED = ch.r3_max_fused()        # read off csrc/plan.hpp


def test_every_answer_to_does_the_8_amplitude_kernel_run_this_plan_agrees():
    """bornvi_plan_compact_describe (what the describe tools and bench.py report) refuses exactly the plans past the depth
    limit among otherwise identical ones; get_plan and the fused dot take the same helper (plan.hpp: r3_plan_eligible), which
    test_gpu_circuit_precision.py observes on the device through paramshift_dot_supported."""
    from tensornetworks_amd import _ext
    he = _ext.ANSATZ_IDS["hardware_efficient"]
    for n, kb, L_in, L_out in [(9, 8, 111, 112), (9, 8, 111, 125), (16, 0, 62, 63), (16, 0, 62, 70)]:
        for L, eligible in ((L_in, True), (L_out, False)):
            W = _ext.plan_words(he, n, L, kb | _ext.R3)
            nf, passes = int(W[4]), int(W[3])
            words, _ = _ext.plan_compact_words(he, n, L, kb)
            print(f"hardware_efficient n={n} L={L} tile_bits={kb}: {passes} passes, {nf} fused gates, 8-amplitude kernel: {words is not None}")
            assert passes > 1 and (nf <= R3_MAX_FUSED) == eligible and (words is not None) == eligible
    # the two cases of the issue: eligible before the limit existed (multi-pass, > 1074 fused gates), refused now
    for n, L, kb in [(9, 125, 8), (16, 70, 0)]:
        assert int(_ext.plan_words(he, n, L, kb | _ext.R3)[4]) > 1074
    # every plan of the benchmark and of the existing tests keeps its kernel: a few hundred fused gates at most
    for ansatz, n, L in [("hardware_efficient", 16, 6), ("hardware_efficient", 20, 8), ("all_to_all", 14, 3), ("basic", 12, 4)]:
        nf = int(_ext.plan_words(_ext.ANSATZ_IDS[ansatz], n, L, _ext.R3)[4])
        assert nf <= 200 and _ext.plan_compact_words(_ext.ANSATZ_IDS[ansatz], n, L, 0)[0] is not None, (ansatz, n, L, nf)
