"""Exact sparse statevector simulation of the ansatz circuits (test infrastructure only).

A dense CPU simulation stops being practical near n = 24; this one is exact at any n as long as the state keeps few
non-zero amplitudes.  The state is a pair of arrays ``idx`` (int64 basis indices, wire 0 = MSB, as everywhere in the
project) and ``amp`` (complex128).  The gate order is ``oracle.circuit.gate_list``'s and the gate matrices are
``oracle.circuit.matrix_1q``'s.

Runs of one-qubit gates on a wire are multiplied into one pending 2x2 matrix, flushed when a CNOT or CZ touches the
wire and at the end.  A flushed matrix whose off-diagonal (or diagonal) entries are below MONOMIAL_TOL in magnitude only
permutes indices and sets phases; any other matrix splits every index in two, and equal indices are merged.  CNOT is an
index XOR, CZ a sign.

``sparse_theta`` draws angles that keep the support at most 2^g for g "generic" rotations: with every other one-qubit
gate monomial (RX = 0 and RY = pi/2 in layer 0 of hardware_efficient / all_to_all, where RY(pi/2) H = X; RX, RY in
{0, pi} elsewhere; RZ anything) only the generic ones split the state.
"""
import numpy as np

from .circuit import gate_list, matrix_1q, num_params

MONOMIAL_TOL = 1e-15


def _flush(idx, amp, U, n, w):
    bit = n - 1 - w
    mask = np.int64(1) << bit
    b = (idx >> bit) & 1
    if abs(U[0, 1]) < MONOMIAL_TOL and abs(U[1, 0]) < MONOMIAL_TOL:
        return idx, amp * np.where(b == 1, U[1, 1], U[0, 0])
    if abs(U[0, 0]) < MONOMIAL_TOL and abs(U[1, 1]) < MONOMIAL_TOL:
        # |b> -> U[1-b, b] |1-b>
        return idx ^ mask, amp * np.where(b == 1, U[0, 1], U[1, 0])
    # |b> -> U[0, b] |0> + U[1, b] |1>
    i0, i1 = idx & ~mask, idx | mask
    a0 = amp * np.where(b == 1, U[0, 1], U[0, 0])
    a1 = amp * np.where(b == 1, U[1, 1], U[1, 0])
    u, inv = np.unique(np.concatenate([i0, i1]), return_inverse=True)
    a = np.concatenate([a0, a1])
    merged = np.bincount(inv, weights=a.real, minlength=u.size) + 1j * np.bincount(inv, weights=a.imag, minlength=u.size)
    return u, merged


def state_sparse(ansatz_type, n, layers, theta):
    """-> (idx int64 [m], amp complex128 [m]) sorted by idx: the non-zero amplitudes of the circuit's state."""
    theta = np.asarray(theta, dtype=np.float64)
    if theta.size != num_params(ansatz_type, n, layers):
        raise ValueError("theta has the wrong length")
    idx = np.zeros(1, dtype=np.int64)
    amp = np.ones(1, dtype=np.complex128)
    pending = [None] * n

    def flush(w):
        nonlocal idx, amp
        if pending[w] is not None:
            idx, amp = _flush(idx, amp, pending[w], n, w)
            pending[w] = None

    for kind, wires, p in gate_list(ansatz_type, n, layers):
        if kind in ("H", "RX", "RY", "RZ"):
            w = wires[0]
            U = matrix_1q(kind, None if p is None else theta[p])
            pending[w] = U if pending[w] is None else U @ pending[w]
        elif kind == "CNOT":
            c, t = wires
            flush(c)
            flush(t)
            idx = idx ^ (((idx >> (n - 1 - c)) & 1) << (n - 1 - t))
        elif kind == "CZ":
            a, b = wires
            flush(a)
            flush(b)
            both = ((idx >> (n - 1 - a)) & (idx >> (n - 1 - b)) & 1) == 1
            amp = np.where(both, -amp, amp)
        else:
            raise ValueError(kind)
    for w in range(n):
        flush(w)
    order = np.argsort(idx, kind="stable")
    return idx[order], amp[order]


def probs_sparse(ansatz_type, n, layers, theta):
    """-> (idx int64 [m], p float64 [m]) sorted by idx; every outcome not in idx has probability exactly 0."""
    idx, amp = state_sparse(ansatz_type, n, layers, theta)
    return idx, amp.real ** 2 + amp.imag ** 2


def param_kinds(ansatz_type, n, layers):
    """-> list of (kind, wire, layer) per parameter, in parameter order."""
    out = []
    per_layer = num_params(ansatz_type, n, 1)
    for kind, wires, p in gate_list(ansatz_type, n, layers):
        if p is not None:
            out.append((kind, wires[0], p // per_layer))
    return out


def sparse_theta(ansatz_type, n, layers, rng, g=6, wires=None):
    """Angles that keep the state's support at most 2^g (module docstring) -> (theta [P], generic parameter indices).

    The g generic rotations get uniform random angles; they sit on wires 0, 1, n/2, n-2, n-1 and then random wires
    (or on `wires`), in layers chosen round-robin, so that the entangling gates carry their superpositions into high and
    low index bits alike."""
    kinds = param_kinds(ansatz_type, n, layers)
    P = len(kinds)
    theta = np.zeros(P)
    two_layer0 = ansatz_type in ("hardware_efficient", "all_to_all")
    for p, (kind, w, layer) in enumerate(kinds):
        if kind == "RZ":
            theta[p] = rng.uniform(0.0, 2.0 * np.pi)
        elif two_layer0 and layer == 0:
            theta[p] = np.pi / 2 if kind == "RY" else 0.0
        else:
            theta[p] = np.pi * rng.integers(0, 2)
    if layers == 0 or g == 0:
        return theta, []
    if wires is None:
        base = [0, 1, n // 2, n - 2, n - 1] if n >= 4 else list(range(n))
        wires = []
        for w in base + list(rng.permutation(n)):
            if w not in wires:
                wires.append(int(w))
    wires = list(wires)[:g]
    generic = []
    rot_kinds = ("RX", "RY") if ansatz_type != "basic" else ("RY",)
    for j, w in enumerate(wires):
        layer = j % layers
        kind = rot_kinds[j % len(rot_kinds)]
        p = next(i for i, k in enumerate(kinds) if k == (kind, w, layer))
        theta[p] = rng.uniform(0.0, 2.0 * np.pi)
        generic.append(p)
    return theta, generic


def shifted_thetas(theta, params, shift=np.pi / 2):
    """-> list of (theta + shift e_p, theta - shift e_p) for p in params: the two circuits of the parameter-shift rule."""
    theta = np.asarray(theta, dtype=np.float64)
    out = []
    for p in params:
        tp = theta.copy(); tp[p] += shift
        tm = theta.copy(); tm[p] -= shift
        out.append((tp, tm))
    return out


def paramshift_sparse(ansatz_type, n, layers, theta, params):
    """-> list of ((idx+, p+), (idx-, p-)) per parameter: sparse probabilities of the +-pi/2-shifted circuits."""
    return [(probs_sparse(ansatz_type, n, layers, tp), probs_sparse(ansatz_type, n, layers, tm))
            for tp, tm in shifted_thetas(theta, params)]
