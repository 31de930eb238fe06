"""Extended-precision reference of the circuit engines and their per-entry error bounds: circuit_pass_r3_kernel,
circuit_pass_fast_kernel / circuit_pass_kernel, build_gates_kernel with its pivot normalisation, gate_scale_kernel, the
fused-dot last pass, shift_dot_kernel and the adjoint walk (kernels_circuit.hip, kernels_circuit8.hip,
kernels_adjoint.hip).  Test infrastructure, shared by test_circuit_precision_host.py (CPU) and
test_gpu_circuit_precision.py (MI355X); not under test.

Reference.  ``reference`` walks oracle.circuit.gate_list gate by gate in x87 long double (hp_reference.LD) with the
oracle's wire and bit conventions (wire 0 = most significant bit).  cos and sin of theta / 2 come from mpmath: the float64
angle is converted exactly, evaluated at 40 digits and rounded once to long double, so no libm argument reduction is
involved.  A shifted row takes its angle as the device forms it: one float64 addition of +-pi/2 (or pi).  Beside psi and
q = |psi|^2 it returns the envelope psi_abs: the same walk from |e_0| with every matrix entry replaced by its modulus
(every subtraction an addition; CNOT and CZ are permutations).

Bounds (first order in EPS64 = 2^-52; every rounding counts as one whole unit although a correctly rounded operation errs
by half of one; nothing is fitted).  All counts below bound the MODULUS of a complex error; a complex x complex product
whose real and imaginary parts each carry k roundings errs by at most sqrt(2) k eps |a| |b|.
    amplitudes  |psi_hat_z - psi_z| <= E_z = EPS64 C_psi min(psi_abs_z, sqrt 2),  real and imaginary part each.
        Envelope arm: the local error of fused gate j is at most c_g eps (|M_k| ... |M_1|) |psi_{j-1}| (M_e its elementary
        gates) and travels on through moduli.  Norm arm: the same error has 2-norm at most sqrt 2 c_g eps, because the
        modulus matrix of a 2 x 2 unitary has norm at most sqrt 2, and later unitaries keep that norm.
    C_psi = sum of c_g over the fused gates of the PLAN (read off bornvi_plan_describe), c_g = c_build + c_apply:
        c_build   sincos: 2 units per rotation (the HIP math API documents 1 to 2 ulp for sin, cos and sincos in double
                  over the full range; 2 is taken), 1 for the rounded constant of H; then one 2 x 2 complex product per
                  further elementary gate (the first meets the identity and is exact): each entry is 4 real products and
                  3 sums, a chain of 4, times sqrt 2:            c_build = sum trig + 4 sqrt 2 (ne - 1)
        r3        the record: |p|^2 (3), the quotients of 1 / p (1): 4, relative; an entry times 1 / p: product and
                  sum, 2 sqrt 2.  The 12-instruction application: z1 = C x0 + D x1 is a product and three fmas, a chain
                  of 4, times sqrt 2 (z0 has two).  The error of the pivot itself cancels: the probabilities are multiplied
                  back by the |p|^2 the record holds.                  c_apply = 4 + 2 sqrt 2 + 4 sqrt 2
        r4        op_u1: 4 products and 3 sums per component, a chain of 4: c_apply = 4 sqrt 2 (both 16-amplitude kernels)
        adjoint   apply_1q per ELEMENTARY gate: sincos (2) and two products and a sum (2 sqrt 2); H: its constant, a
                  sum and a product, 3 sqrt 2.
    probabilities  |q_hat_z - q_z| <= (|psi_z| + E_z)^2 - |psi_z|^2 + EPS64 C_q q_z.  The quadratic term is the whole
        bound where an amplitude vanishes by cancellation.  C_q = 3 (two squares and their sum); r3 adds the product
        with scale (1) and scale's own chain: n_fused values |p|^2 of 3 roundings each, n_fused lane products and the 63
        products of the butterfly: 4 n_fused + 64.
    gradients  1/2 sum |w_z| (b+_z + b-_z) + EPS64 C_dot 1/2 sum |w_z| (q+_z + q-_z), b the q bound of the shifted rows.
        C_dot, stored rows (shift_dot_kernel): difference, product, pair sum (3), ceil(2^n / 2048) accumulations, 6
        butterfly levels, 16 wave sums, the scale (1).  Fused dot: square, two fmas (3), 8 accumulations, 6 levels, the
        waves of a tile, the scale (1), the tiles of a row, the final difference (1).
    adjoint_vjp  g_k = sum Im <lambda_k| P |phi_k> from states the backward walk un-computes with U^+.  With C_f the
        forward sum of c over all elementary gates and C_b(k) the same over the gates after k,
            |d phi_k| <= eps (C_f + C_b(k)) B_k,   |d lambda_k| <= eps (C_f + 1 + C_b(k)) Lam_k,
        B_k and Lam_k the backward modulus walks of psi_abs and |w| psi_abs (|U|^T |U| v >= v for v >= 0, so these also
        dominate |phi_k| and |lambda_k|).  Envelope arm: eps (2 C_f + 2 C_b + 1 + C_chain) sum Lam_k (|P| B_k); norm arm
        (|| lambda || <= max |w|): eps max |w| (sqrt 2 (2 C_f + 2 C_b + 1) + C_chain).  The smaller holds.
        Its reference is the adjoint walk itself in long double (adjoint_gradient): the parameter-shift difference
        1/2 sum w (q+ - q-) cancels to about eps sum |w| q and is only the derivative to about eps (the device's shift is
        the float64 pi/2 added in float64), so it cannot referee the gradients below that which the envelope arm bounds.
        test_circuit_precision_host.py ties the walk to that independent definition: per parameter the two agree within
        the difference's derived error.
"""
import functools

import numpy as np

import hp_reference as hp
from hp_reference import EPS64, LD, to_f64
from oracle import circuit as oc

CLD = np.clongdouble
SQRT2 = 1.4142135623730951            # sqrt 2 rounded up
TRIG_UNITS = 2.0
KIND_NAMES = ("H", "RX", "RY", "RZ")
Q_FLOOR_LOG2 = -900                   # the input families keep the smallest non-zero q above 2^-900 (asserted)


def unavailable():
    if hp.HAVE_LONGDOUBLE:
        return None
    return f"long double unavailable (np.longdouble eps {np.finfo(LD).eps:.3g})"


# ------------------------------------------------------------------------------------------------ trigonometry
@functools.lru_cache(maxsize=None)
def _mp():
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.dps = 40
    return ctx


@functools.lru_cache(maxsize=1 << 16)
def trig_half(t):
    """(cos(t / 2), sin(t / 2)) of the float64 t as long doubles, through mpmath at 40 digits."""
    mp = _mp()
    x = mp.mpf(float(t)) / 2                       # float -> mpf and the halving are exact
    return LD(mp.nstr(mp.cos(x), 30)), LD(mp.nstr(mp.sin(x), 30))


def matrix_ld(kind, t=None):
    """2 x 2 complex long double matrix of an elementary gate (oracle.circuit.matrix_1q's definitions)."""
    m = np.zeros((2, 2), dtype=CLD)
    if kind == "H":
        h = LD(1) / np.sqrt(LD(2))
        m.real[:] = [[h, h], [h, -h]]
        return m
    c, s = trig_half(float(t))
    if kind == "RX":
        m.real[:] = [[c, 0], [0, c]]
        m.imag[:] = [[0, -s], [-s, 0]]
    elif kind == "RY":
        m.real[:] = [[c, -s], [s, c]]
    elif kind == "RZ":
        m.real[:] = [[c, 0], [0, c]]
        m.imag[:] = [[-s, 0], [0, s]]
    else:
        raise ValueError(kind)
    return m


# ------------------------------------------------------------------------------------------------ the walk
def _apply_1q(v, U, n, w):
    x = v.reshape(1 << w, 2, 1 << (n - 1 - w))
    a, b = x[:, 0, :], x[:, 1, :]
    out = np.empty_like(x)
    out[:, 0, :] = U[0, 0] * a + U[0, 1] * b
    out[:, 1, :] = U[1, 0] * a + U[1, 1] * b
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def _cnot_src(n, c, t):
    i = np.arange(1 << n)
    return i ^ (((i >> (n - 1 - c)) & 1) << (n - 1 - t))


@functools.lru_cache(maxsize=None)
def _cz_mask(n, a, b):
    i = np.arange(1 << n)
    return (((i >> (n - 1 - a)) & (i >> (n - 1 - b))) & 1).astype(bool)


def walk(gates, n, theta, envelope=False, v0=None, dtype=None):
    """The state (envelope=False) or its modulus envelope after `gates`, long double, flat, wire 0 = MSB."""
    if v0 is None:
        v = np.zeros(1 << n, dtype=LD if envelope else CLD)
        v[0] = 1
    else:
        v = v0.copy()
    for kind, wires, p in gates:
        if kind in KIND_NAMES:
            U = matrix_ld(kind, None if p is None else theta[p])
            v = _apply_1q(v, np.abs(U) if envelope else U, n, wires[0])
        elif kind == "CNOT":
            v = v[_cnot_src(n, wires[0], wires[1])]
        elif kind == "CZ":
            if not envelope:
                v = np.where(_cz_mask(n, wires[0], wires[1]), -v, v)
        else:
            raise ValueError(kind)
    return v


def reference(ansatz, n, layers, theta):
    """{'psi', 'q', 'psi_abs'} of one circuit in long double; theta float64 exactly as the device receives it."""
    theta = np.asarray(theta, dtype=np.float64)
    g = oc.gate_list(ansatz, n, layers)
    psi = walk(g, n, theta)
    q = psi.real * psi.real + psi.imag * psi.imag
    assert not (q > 0).any() or q[q > 0].min() > LD(2) ** Q_FLOOR_LOG2, "a non-zero q below 2^-900: the bounds carry no underflow floor"
    return {"psi": psi, "q": q, "psi_abs": walk(g, n, theta, envelope=True)}


def shifted(theta, p, shift):
    """theta with one float64 addition at p: what build_gates_kernel forms."""
    t = np.array(theta, dtype=np.float64)
    t[p] = t[p] + shift
    return t


# ------------------------------------------------------------------------------------------------ constants
def fused_table(ansatz, n, layers, flags=0):
    """[(wire, [kind names])] of the plan's fused gates, and the plan's pass count (bornvi_plan_describe; host only)."""
    from tensornetworks_amd import _ext
    W = _ext.plan_words(_ext.ANSATZ_IDS[ansatz] if isinstance(ansatz, str) else ansatz, n, layers, flags)
    nf, off = int(W[4]), int(W[6])
    table = []
    for f in range(nf):
        fw = W[off + 10 * f: off + 10 * (f + 1)]
        table.append((int(fw[0]), [KIND_NAMES[int(fw[2 + 2 * e])] for e in range(int(fw[1]))]))
    return table, int(W[3])


def c_build(kinds):
    return sum(1.0 if k == "H" else TRIG_UNITS for k in kinds) + 4 * SQRT2 * (len(kinds) - 1)


def c_gate(kinds, engine):
    """engine 'r3' (circuit_pass_r3_kernel, records) or 'r4' (op_u1 of circuit_pass_fast_kernel / circuit_pass_kernel)."""
    return c_build(kinds) + (4 + 2 * SQRT2 + 4 * SQRT2 if engine == "r3" else 4 * SQRT2)


def plan_constants(ansatz, n, layers, engine, flags=0):
    """{'C_psi', 'C_q', 'n_fused', 'n_passes'} of the plan the library runs under this engine and tile setting."""
    from tensornetworks_amd import _ext
    table, passes = fused_table(ansatz, n, layers, flags | (_ext.R3 if engine == "r3" else 0))
    nf = len(table)
    return {"C_psi": float(sum(c_gate(k, engine) for _, k in table)), "C_q": float(3 + (1 + 4 * nf + 64 if engine == "r3" else 0)),
            "n_fused": nf, "n_passes": passes}


def c_adjoint(kind):
    return 3 * SQRT2 if kind == "H" else TRIG_UNITS + 2 * SQRT2


def adjoint_constants(ansatz, n, layers):
    g = [k for k, _, _ in oc.gate_list(ansatz, n, layers) if k in KIND_NAMES]
    return {"C_psi": float(sum(c_adjoint(k) for k in g)), "C_q": 3.0}


def c_dot_rows(n):
    return float(3 + -(-(1 << n) // 2048) + 6 + 16 + 1)


def c_dot_fused(n, k):
    return float(3 + 8 + 6 + max(1, (1 << (k - 3)) // 64) + 1 + (1 << (n - k)) + 1)


# ------------------------------------------------------------------------------------------------ bounds and ratios
def worst_ratio(r):
    """The worst entry of a ratio array as a float; NaN (a NaN or inf * 0 output) counts as the worst: inf."""
    return hp.worst(r)[0]


def fold(*values):
    """Largest of some worst ratios, NaN counting as inf (Python's max and numpy's would drop or pass it)."""
    v = np.asarray([float(x) for x in values], dtype=np.float64)
    return float(np.where(np.isnan(v), np.inf, v).max()) if v.size else 0.0


def r3_max_fused():
    """R3_MAX_FUSED as csrc/plan.hpp states it."""
    import os
    import re
    hdr = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tensornetworks_amd", "csrc", "plan.hpp")
    return int(re.search(r"constexpr int R3_MAX_FUSED = (\d+);", open(hdr).read()).group(1))


def amp_allowed(ref, C_psi):
    return LD(EPS64 * C_psi) * np.minimum(ref["psi_abs"], LD(SQRT2))


def q_allowed(ref, C_psi, C_q):
    E = amp_allowed(ref, C_psi)
    a = np.abs(ref["psi"])
    return (2 * a + E) * E + LD(EPS64 * C_q) * ref["q"]


def allowed_ratio(got, ref, allowed):
    """|got - ref| / allowed per entry (allowed == 0: only got == ref passes), through hp.ratio."""
    return hp.ratio(got, ref, np.asarray(allowed, dtype=LD) / LD(EPS64))


def amp_ratio(got, ref, C_psi):
    """Per entry, the larger of the real and the imaginary part's ratio."""
    got = np.asarray(got, dtype=np.complex128)
    E = amp_allowed(ref, C_psi)
    return np.maximum(allowed_ratio(got.real, ref["psi"].real, E), allowed_ratio(got.imag, ref["psi"].imag, E))


def q_ratio(got, ref, C_psi, C_q):
    return allowed_ratio(got, ref["q"], q_allowed(ref, C_psi, C_q))


def sum_ratio(got, ref, C_psi, C_q):
    """sum q: the entries added in long double on the host, against the reference's sum; allowed: the sum of the bounds."""
    s = np.asarray(got, dtype=np.float64).astype(LD).sum()
    return fold(to_f64(np.abs(s - ref["q"].sum()) / q_allowed(ref, C_psi, C_q).sum()))


@functools.lru_cache(maxsize=512)
def _cached_reference(ansatz, n, layers, key):
    ref = reference(ansatz, n, layers, np.frombuffer(key, dtype=np.float64))
    for a in ref.values():
        a.setflags(write=False)
    return ref


def cached_reference(ansatz, n, layers, theta):
    """reference(), computed once per process for each angle vector and shared read-only."""
    return _cached_reference(ansatz, n, layers, np.ascontiguousarray(theta, dtype=np.float64).tobytes())


def grad_reference(ansatz, n, layers, theta, w, params, C_psi, C_q, C_dot):
    """(g*, allowed) per parameter of `params`: g = 1/2 sum w (q+ - q-) in long double from shifted references."""
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    g, allowed = [], []
    for p in params:
        rp = cached_reference(ansatz, n, layers, shifted(theta, p, np.pi / 2))
        rm = cached_reference(ansatz, n, layers, shifted(theta, p, -np.pi / 2))
        g.append(((wl * rp["q"]).sum() - (wl * rm["q"]).sum()) / 2)
        b = q_allowed(rp, C_psi, C_q) + q_allowed(rm, C_psi, C_q)
        allowed.append((np.abs(wl) * b).sum() / 2 + LD(EPS64 * C_dot) * (np.abs(wl) * (rp["q"] + rm["q"])).sum() / 2)
    return np.array(g, dtype=LD), np.array(allowed, dtype=LD)


def adjoint_gradient(ansatz, n, layers, theta, w, fp64=False):
    """g_k = Im <lambda_k| P_k |phi_k> by the adjoint walk itself, in long double (the reference of bornvi_adjoint_vjp:
    unlike 1/2 sum w (q+ - q-) it does not cancel, so it resolves gradients far below eps sum |w| q) or, fp64=True, in
    complex128 with the oracle's matrices (a host mirror of the kernel's route)."""
    theta = np.asarray(theta, dtype=np.float64)
    gates = oc.gate_list(ansatz, n, layers)
    mat = (lambda k, p: oc.matrix_1q(k, None if p is None else theta[p])) if fp64 else \
        (lambda k, p: matrix_ld(k, None if p is None else theta[p]))
    if fp64:
        phi = oc.simulate(gates, n, theta)
        lam = np.asarray(w, dtype=np.float64) * phi
    else:
        phi = walk(gates, n, theta)
        lam = np.asarray(w, dtype=np.float64).astype(LD) * phi
    g = np.zeros(theta.size, dtype=np.float64 if fp64 else LD)
    for kind, wires, p in reversed(gates):
        if kind in KIND_NAMES:
            if p is not None:
                x = phi.reshape(1 << wires[0], 2, -1)
                if kind == "RZ":
                    v = np.stack([x[:, 0, :], -x[:, 1, :]], axis=1)
                elif kind == "RX":
                    v = x[:, ::-1, :]
                else:                                # Y |phi>: (-i phi_1, i phi_0)
                    v = np.stack([-1j * x[:, 1, :], 1j * x[:, 0, :]], axis=1)
                t = np.conj(lam) * v.reshape(-1)
                g[p] = t.imag.sum()
            Ud = np.conj(mat(kind, p)).T
            phi, lam = _apply_1q(phi, Ud, n, wires[0]), _apply_1q(lam, Ud, n, wires[0])
        elif kind == "CNOT":
            src = _cnot_src(n, wires[0], wires[1])
            phi, lam = phi[src], lam[src]
        else:
            m = _cz_mask(n, wires[0], wires[1])
            phi, lam = np.where(m, -phi, phi), np.where(m, -lam, lam)
    return g


def adjoint_grid(n):
    npairs = 1 << max(n - 1, 0)
    return max(1, min(2048, -(-npairs // 256))), npairs


def adjoint_vjp_allowed(ansatz, n, layers, theta, w):
    """Allowed error per parameter of bornvi_adjoint_vjp (module docstring: adjoint_vjp)."""
    theta = np.asarray(theta, dtype=np.float64)
    gates = oc.gate_list(ansatz, n, layers)
    wl = np.abs(np.asarray(w, dtype=np.float64).astype(LD))
    C_f = adjoint_constants(ansatz, n, layers)["C_psi"]
    nwg, npairs = adjoint_grid(n)
    C_chain = 3 + -(-npairs // (nwg * 256)) + 6 + 4 + nwg
    B = walk(gates, n, theta, envelope=True)
    Lam = wl * B
    wmax = wl.max()
    out = np.zeros(theta.size, dtype=LD)
    C_b = 0.0
    for kind, wires, p in reversed(gates):
        if kind in KIND_NAMES:
            if p is not None:
                x = B.reshape(1 << wires[0], 2, -1)
                PB = B if kind == "RZ" else x[:, ::-1, :].reshape(-1)
                env = LD(EPS64 * (2 * C_f + 2 * C_b + 1 + C_chain)) * (Lam * PB).sum()
                norm = LD(EPS64) * wmax * LD(SQRT2 * (2 * C_f + 2 * C_b + 1) + C_chain)
                out[p] = min(env, norm)
            Ua = np.abs(matrix_ld(kind, None if p is None else theta[p])).T
            B, Lam = _apply_1q(B, Ua, n, wires[0]), _apply_1q(Lam, Ua, n, wires[0])
            C_b += c_adjoint(kind)
        elif kind == "CNOT":                         # its own inverse
            src = _cnot_src(n, wires[0], wires[1])
            B, Lam = B[src], Lam[src]
    return out


# ------------------------------------------------------------------------------------------------ angle families
FAMILIES = ("uniform", "init", "tiny", "mixed", "quarter", "tie", "large")


def tie_angles(rng, P, ansatz):
    """RY = pi/2 makes |u00|^2 = |u10|^2 = 1/2 of a fused RZ RY RX (or RZ RY) whatever the other angles are; in float64 the
    two squared moduli then differ by a few ulps either way or not at all, and so does the record's exchange flag.  RY is
    pi/2, its lower or its upper neighbour; RX and RZ are uniform, so the states are generic."""
    t = rng.uniform(-np.pi, np.pi, P)
    ry = np.arange(P) % 2 == 0 if ansatz == "basic" else np.arange(P) % 3 == 1
    k = rng.integers(0, 3, P)
    half = np.where(k == 1, np.nextafter(np.pi / 2, 0.0), np.where(k == 2, np.nextafter(np.pi / 2, 4.0), np.pi / 2))
    return np.where(ry, half, t)


def angles(family, P, seed=0, ansatz="hardware_efficient"):
    """float64 [P] of one family ('tie' needs the ansatz: where the RY angles sit).  'all_half_pi': every angle pi/2, the
    all-tie vector and the deep case's second one."""
    rng = np.random.default_rng([seed, FAMILIES.index(family) if family in FAMILIES else 99, P])
    if family == "uniform":
        return rng.uniform(-np.pi, np.pi, P)
    if family == "init":                         # as bench.py draws it: float32 0.1 randn
        return (0.1 * rng.standard_normal(P)).astype(np.float32).astype(np.float64)
    if family == "tiny":
        t = 1e-9 * rng.standard_normal(P)
        t[::5] = 0.0
        t[2::7] = -0.0
        return t
    if family == "mixed":
        return rng.standard_normal(P) * rng.choice([1e-9, 1e-3, 1.0], P)
    if family == "quarter":
        return rng.integers(-4, 5, P) * (np.pi / 2)
    if family == "tie":
        return tie_angles(rng, P, ansatz)
    if family == "large":
        t = rng.uniform(-np.pi, np.pi, P)
        big = rng.random(P) < 0.1
        big[0] = True
        return np.where(big, np.sign(t) * 10.0 ** rng.uniform(3, 6, P), t)
    if family == "all_half_pi":
        return np.full(P, np.pi / 2)
    raise ValueError(family)


# ------------------------------------------------------------------------------------------------ float64 mirror
def fuse(gates):
    """The gate list with runs of one-qubit gates on a wire fused (at most 4), as the planner fuses them: a wire's pending
    gates are emitted when an entangler touches it, when a fifth arrives, or at the end.  -> [('U', wire, [(kind, p)]) |
    ('CNOT' | 'CZ', wires, None)]."""
    out, pending = [], {}
    for kind, wires, p in gates:
        if kind in KIND_NAMES:
            lst = pending.setdefault(wires[0], [])
            if len(lst) == 4:
                out.append(("U", wires[0], pending.pop(wires[0])))
                lst = pending.setdefault(wires[0], [])
            lst.append((kind, p))
        else:
            for w in wires:
                if w in pending:
                    out.append(("U", w, pending.pop(w)))
            out.append((kind, wires, None))
    for w in sorted(pending):
        out.append(("U", w, pending[w]))
    return out


def mirror_matrix(elems, theta, mutant=None, arg=None):
    """Fused 2 x 2 matrix of the mirror: elementary matrices from float64 cos / sin, multiplied in order (float64)."""
    U = np.eye(2, dtype=np.complex128)
    for k, p in elems:
        if k == "H":
            h = float(np.float32(0.70710678118654752440)) if mutant == "h32" else 0.70710678118654752440
            M = np.array([[h, h], [h, -h]], dtype=np.complex128)
        else:
            t = theta[p] / 2.0
            c, s = float(np.cos(t)), float(np.sin(t))
            if mutant == "sincos32" and p == arg:
                c, s = float(np.cos(np.float32(t))), float(np.sin(np.float32(t)))
            if mutant == "sin_from_cos":
                s = float(np.copysign(np.sqrt(max(0.0, 1.0 - c * c)), s))
            M = {"RX": [[c, -1j * s], [-1j * s, c]], "RY": [[c, -s], [s, c]], "RZ": [[c - 1j * s, 0], [0, c + 1j * s]]}[k]
            M = np.array(M, dtype=np.complex128)
        U = M @ U
    return U


LAST_CZ_DROP = [None, None]      # (entry, its |x|^2 at the gate) the last cz_drop mutant left unsigned


def mirror_r3(ansatz, n, layers, theta, mutant=None, arg=None, want_psi=False):
    """Plain float64 restatement of the pivot-normalised recipe (build_gates_kernel's record, the 12-instruction pair
    update, the exchange flag, scale = prod |p|^2) in gate-list order: -> q, or (q, psi = x prod p) with want_psi.
    mutant: one seeded defect (test_circuit_precision_host.MUTANTS); arg selects where."""
    theta = np.asarray(theta, dtype=np.float64)
    N = 1 << n
    x = np.zeros(N, dtype=np.complex128)
    x[0] = 1.0
    scale, prod_p = 1.0, 1.0 + 0.0j
    nu = ncz = 0
    for kind, wires, elems in fuse(oc.gate_list(ansatz, n, layers)):
        if kind == "CNOT":
            x = x[_cnot_src(n, wires[0], wires[1])]
            continue
        if kind == "CZ":
            m = _cz_mask(n, wires[0], wires[1]).copy()
            if mutant == "cz_drop" and ncz == arg:          # the signed entry of largest modulus with |x|^2 < 1e-14
                small = np.where(m & (np.abs(x) ** 2 < 1e-14), np.abs(x), -1.0)
                assert small.max() > 0
                m[int(np.argmax(small))] = False
                LAST_CZ_DROP[:] = [int(np.argmax(small)), float(small.max() ** 2)]
            x = np.where(m, -x, x)
            ncz += 1
            continue
        U = mirror_matrix(elems, theta, mutant, arg)
        m0 = U[0, 0].real ** 2 + U[0, 0].imag ** 2
        m1 = U[1, 0].real ** 2 + U[1, 0].imag ** 2
        sw = bool(m1 > m0)
        piv, pm = (U[1, 0], m1) if sw else (U[0, 0], m0)
        inv = complex(piv.real / pm, -piv.imag / pm)
        r0, r1 = (U[1], U[0]) if sw else (U[0], U[1])
        B, C, D = r0[1] * inv, r1[0] * inv, r1[1] * inv
        v = x.reshape(1 << wires, 2, -1)
        a, b = v[:, 0, :], v[:, 1, :]
        z0, z1 = a + B * b, C * a + D * b
        if sw and not (mutant == "tie_ignore" and nu == arg):
            z0, z1 = z1, z0
        x = np.stack([z0, z1], axis=1).reshape(-1)
        if not (mutant == "scale_drop" and nu == arg):
            scale *= pm
        prod_p *= piv
        nu += 1
    q = (x.real * x.real + x.imag * x.imag) * scale
    return (q, x * prod_p) if want_psi else q


def mirror_pivots(ansatz, n, layers, theta):
    """(m0, m1) = (|u00|^2, |u10|^2) in float64 of every fused gate of the mirror, in its order."""
    theta = np.asarray(theta, dtype=np.float64)
    out = []
    for kind, wires, elems in fuse(oc.gate_list(ansatz, n, layers)):
        if kind != "U":
            continue
        U = mirror_matrix(elems, theta)
        out.append((U[0, 0].real ** 2 + U[0, 0].imag ** 2, U[1, 0].real ** 2 + U[1, 0].imag ** 2))
    return out


def mirror_constants(ansatz, n, layers):
    """C_psi and C_q of mirror_r3 (its own fusion, the r3 counts; scale is one sequential product: 4 per gate).  C_psi_state
    is for its psi = x prod p: the complex product of the pivots adds 2 sqrt 2 per gate and one final product."""
    fused = [e for k, _, e in fuse(oc.gate_list(ansatz, n, layers)) if k == "U"]
    return {"C_psi": float(sum(c_gate([k for k, _ in e], "r3") for e in fused)), "C_q": float(4 + 4 * len(fused)), "n_fused": len(fused),
            "C_psi_state": float(sum(c_gate([k for k, _ in e], "r3") for e in fused) + 2 * SQRT2 * (len(fused) + 1))}


def oracle_constants(ansatz, n, layers):
    """oc.simulate applies elementary gates one by one: trig (2; H: its constant and the division, 2) and a chain of 4."""
    g = [k for k, _, _ in oc.gate_list(ansatz, n, layers) if k in KIND_NAMES]
    return {"C_psi": float(sum(TRIG_UNITS + 4 * SQRT2 + (2 * SQRT2 if k == "RZ" else 0) for k in g)), "C_q": 3.0}


def peaked_angles(ansatz, n, layers, seed=0):
    """A peaked state out of an ansatz that starts with Hadamards: the first layer's RY = -pi/2 + 1e-4 randn takes |+> back
    to about |0> (by cancellation: the envelope stays flat), every other angle is 1e-4 randn.  'basic' has no H: 1e-4 randn."""
    rng = np.random.default_rng([seed, 77, n, layers])
    t = 1e-4 * rng.standard_normal(oc.num_params(ansatz, n, layers))
    if ansatz != "basic":
        t[1:3 * n:3] -= np.pi / 2
    return t
