"""Tensor-level wrappers over the bornvi C ABI (include/bornvi.h).

PyTorch owns every buffer (inputs, outputs, workspaces) and the stream; this module only checks
shapes / dtypes / devices and passes raw pointers.  Everything here needs an MI355X: tensors must
live on a 'cuda' (PyTorch-ROCm) device.  There is no CPU path.
"""
import ctypes as C
import math
import os
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _ext
from ._ext import ANSATZ_IDS, BornviError

_workspaces = {}

# Cap for the circuit workspace (bytes); larger batches are processed in chunks by the library.
WORKSPACE_CAP = int(os.environ.get("BORNVI_WORKSPACE_CAP", str(48 << 30)))


def compute_device(preferred=None):
    """The GPU this process computes on: `preferred` if it is a cuda device, else cuda:LOCAL_RANK / current."""
    if preferred is not None:
        d = torch.device(preferred)
        if d.type == "cuda":
            return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
    if not torch.cuda.is_available():
        raise BornviError("no MI355X visible: the bornvi backend has no CPU fallback "
                          "(torch.cuda.is_available() is False)")
    return torch.device("cuda", torch.cuda.current_device())


def ansatz_id(ansatz_type):
    """quantum_born_machine.py:31-38/:113: any string other than the two named ones selects 'basic'."""
    return ANSATZ_IDS.get(ansatz_type, ANSATZ_IDS["basic"])


def num_params(ansatz_type, n, layers):
    return _ext.lib().bornvi_num_params(ansatz_id(ansatz_type), n, layers)


def _ws_key(dev, tag):
    return (dev.index, tag, int(torch.cuda.current_stream(dev).cuda_stream))


def _ws(dev, nbytes, tag="main"):
    """Cached workspace, one per (device, purpose, STREAM): a buffer is only ever used on the stream it was allocated
    on, so the caching allocator's stream-ordered reuse stays valid when a workspace is re-grown (the graphed step
    warms up and captures on a side stream, and the probes launch on several streams)."""
    key = _ws_key(dev, tag)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        _workspaces[key] = None
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        _workspaces[key] = buf
    return buf


def fresh_workspace(dev, nbytes):
    """A new device buffer that can be installed as a workspace (set_workspace)."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def set_workspace(dev, tag, buf):
    """Makes `buf` the cached workspace `tag` of the current stream (the trainer places the symmetric contraction's
    workspace by measurement: SteinOperator._place_gram)."""
    _workspaces[_ws_key(dev, tag)] = buf


def release_workspaces():
    _workspaces.clear()


def _chk(t, dtype, dev, name, numel=None):
    """dtype / device / contiguity and (the C ABI sees raw pointers only) the element count the kernels will index."""
    if t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise BornviError(f"{name}: expected contiguous {dtype} on {dev}, got {t.dtype} on {t.device}")
    if numel is not None and t.numel() != int(numel):
        raise BornviError(f"{name}: expected {int(numel)} elements, got {t.numel()} (shape {tuple(t.shape)})")


def _out(t, dtype, dev, name, shape):
    """The optional output `t`, checked for the element count of `shape` (an int or a tuple), or a new tensor of that shape."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    _chk(t, dtype, dev, name, math.prod(shape) if isinstance(shape, tuple) else shape)      # not np.prod: 3 us a call
    return t


def _seed_word(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise BornviError(f"seed must be an integer, got {seed!r}")
    return int(seed) & ((1 << 64) - 1)


def _sample_count(B):
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not 1 <= int(B) <= MPS_SAMPLED_MAX_BATCH:
        raise BornviError(f"number of samples: 1 ... 2^24 per call, got {B!r}")
    return int(B)


def _evidence_args(mask, value, dev, count=None):
    """Checks a list of evidences (mask, value int64 [Q], 1 <= Q <= 2^16), or with `count` one of exactly that many -> Q."""
    if count is not None:
        if not torch.is_tensor(mask) or not torch.is_tensor(value):
            raise BornviError(f"mask, value: expected two [{count}] int64 tensors")
    else:
        if not torch.is_tensor(mask) or not torch.is_tensor(value) or mask.dim() != 1 or mask.shape != value.shape:
            raise BornviError("mask, value: expected two [Q] int64 tensors")
        count = int(mask.numel())
        if not 1 <= count <= MPS_QUERY_MAX_QUERIES:
            raise BornviError(f"number of queries: 1 ... 2^16 per call, got {count}")
    _chk(mask, torch.int64, dev, "mask", count)
    _chk(value, torch.int64, dev, "value", count)
    return count


# Largest n of the circuit engines (circuits, parameter shift, fused dot, adjoint) and of the matrix-free Stein mat-vec:
# the planner's tile and workgroup indices are 16 bits and its tiles hold at most 2^13 amplitudes (include/bornvi.h).
CIRCUIT_MAX_N = _ext.LIMITS["BORNVI_CIRCUIT_MAX_N"]


def _chk_n(n, lo=1, hi=30):
    if not (isinstance(n, (int, np.integer)) and lo <= int(n) <= hi):
        raise BornviError(f"number of qubits / latent variables out of range: {n!r} (accepted: {lo} ... {hi})")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


_size_cache = {}


def _cached_size(h, name, *args):
    key = (h.device_index, name) + args
    v = _size_cache.get(key)
    if v is None:
        v = _size_cache[key] = h.size(name, *args)
    return v


def clip_cast_grad(grad64, max_norm):
    """float64 gradient -> (float32 gradient clipped like clip_grad_norm_, its float32 total norm [0-dim])."""
    dev = grad64.device
    h = _ext.handle_for(dev)
    _chk(grad64, torch.float64, dev, "grad64")
    g32 = torch.empty(grad64.shape, dtype=torch.float32, device=dev)
    norm = torch.empty((), dtype=torch.float32, device=dev)
    h.call("bornvi_clip_cast_grad", grad64.numel(), _ptr(grad64), float(max_norm), _ptr(g32), _ptr(norm),
           _ext.stream_ptr(dev))
    return g32, norm


def clip_cast_grad_guard(grad64, max_norm, loss, out=None, found_out=None):
    """clip_cast_grad plus the NaN/Inf guard of the loss as a device flag: -> (g32, norm [0-dim], found_inf [0-dim]
    float32, 1.0 when loss [1] float64 is NaN or +-Inf), one launch.  out / found_out: destinations to write into
    (theta.grad and the optimiser's found_inf tensor in a captured step: two copy nodes fewer per replay)."""
    dev = grad64.device
    h = _ext.handle_for(dev)
    _chk(grad64, torch.float64, dev, "grad64")
    _chk(loss, torch.float64, dev, "loss")
    if out is not None:
        _chk(out, torch.float32, dev, "out", grad64.numel())
    if found_out is not None:
        _chk(found_out, torch.float32, dev, "found_out", 1)
    g32 = out if out is not None else torch.empty(grad64.shape, dtype=torch.float32, device=dev)
    norm = torch.empty((), dtype=torch.float32, device=dev)
    found = found_out if found_out is not None else torch.empty((), dtype=torch.float32, device=dev)
    h.call("bornvi_clip_cast_grad_guard", grad64.numel(), _ptr(grad64), float(max_norm), _ptr(loss), _ptr(g32), _ptr(norm),
           _ptr(found), _ext.stream_ptr(dev))
    return g32, norm, found


def clip_adam_step(grad64, max_norm, loss, theta, grad32, theta64, exp_avg, exp_avg_sq, counters, lr_table, beta1, beta2,
                   eps, norm_out=None, loss_history=None, norm_history=None):
    """clip_cast_grad_guard + the Adam update of float32 theta + the float64 copy of the new theta, one launch
    (bornvi_clip_adam_step).  All tensors on the GPU and updated in place; -> the gradient's float32 norm [0-dim]."""
    dev = grad64.device
    h = _ext.handle_for(dev)
    P = grad64.numel()
    _chk(grad64, torch.float64, dev, "grad64")
    _chk(loss, torch.float64, dev, "loss")
    for t, dt, nm in ((theta, torch.float32, "theta"), (grad32, torch.float32, "grad32"), (theta64, torch.float64, "theta64"),
                      (exp_avg, torch.float32, "exp_avg"), (exp_avg_sq, torch.float32, "exp_avg_sq")):
        _chk(t, dt, dev, nm, P)
    _chk(counters, torch.int32, dev, "counters", 2)
    _chk(lr_table, torch.float64, dev, "lr_table")
    norm = norm_out if norm_out is not None else torch.empty((), dtype=torch.float32, device=dev)
    _chk(norm, torch.float32, dev, "norm_out", 1)
    if loss_history is not None:
        _chk(loss_history, torch.float64, dev, "loss_history", lr_table.numel())
    if norm_history is not None:
        _chk(norm_history, torch.float32, dev, "norm_history", lr_table.numel())
    h.call("bornvi_clip_adam_step", P, _ptr(grad64), float(max_norm), _ptr(loss), _ptr(theta), _ptr(grad32), _ptr(theta64),
           _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(counters), _ptr(lr_table), lr_table.numel(), float(beta1), float(beta2),
           float(eps), _ptr(norm), _ptr(loss_history) if loss_history is not None else None,
           _ptr(norm_history) if norm_history is not None else None, _ext.stream_ptr(dev))
    return norm


def set_option(dev, name, value):
    _size_cache.clear()
    h = _ext.handle_for(dev)
    h.call("bornvi_set_option", name.encode(), int(value))


def get_option(dev, name):
    """Current value of a planner / engine option of this device's handle (bornvi_get_option)."""
    v = C.c_longlong(0)
    _ext.handle_for(dev).call("bornvi_get_option", name.encode(), C.byref(v))
    return int(v.value)


def set_engine_option(dev, name, value):
    """Options that do not change plans or workspace sizes (e.g. "batched_quadform"): no cache invalidation."""
    _ext.handle_for(dev).call("bornvi_set_option", name.encode(), int(value))


_ROCTX = os.environ.get("BORNVI_ROCTX", "0") == "1"


class EventSpan:
    """`with` block that records a (start, end) torch.cuda.Event pair on the current stream -- the
    stream every bornvi kernel of the block is launched on -- when timers are enabled."""

    def __init__(self, timers, name):
        self.timers, self.name = timers, name

    def __enter__(self):
        if _ROCTX:                       # BORNVI_ROCTX=1: named ranges for rocprofv3 --marker-trace / roctx consumers
            torch.cuda.nvtx.range_push(f"bornvi:{self.name}")
        if self.timers is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if _ROCTX:
            torch.cuda.nvtx.range_pop()
        if self.timers is not None:
            self.ev[1].record()
            self.timers.setdefault(self.name, []).append(self.ev)
        return False


# ---- circuits -------------------------------------------------------------------------------------
def circuit_probs(ansatz_type, n, layers, thetas):
    """thetas float64 [B, P] on a cuda device -> probs float64 [B, 2^n]."""
    _chk_n(n, 1, CIRCUIT_MAX_N)
    dev = thetas.device
    h = _ext.handle_for(dev)
    aid = ansatz_id(ansatz_type)
    P = num_params(ansatz_type, n, layers)
    if thetas.dim() != 2 or thetas.shape[1] != P:
        raise BornviError(f"thetas must be [batch, {P}]")
    _chk(thetas, torch.float64, dev, "thetas")
    B = thetas.shape[0]
    probs = torch.empty((B, 1 << n), dtype=torch.float64, device=dev)
    need = h.size("bornvi_circuit_workspace_bytes", aid, n, layers, B)
    ws = _ws(dev, min(need, max(WORKSPACE_CAP, h.size("bornvi_circuit_workspace_bytes", aid, n, layers, 1))))
    h.call("bornvi_circuit_probs", aid, n, layers, B, _ptr(thetas), _ptr(probs), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return probs


def paramshift_probs(ansatz_type, n, layers, theta, p_begin, p_end, include_base=True, out=None, ws_tag="main",
                     p_stride=1):
    """theta float64 [P] -> probs [(1 if include_base) + 2 count, 2^n]: optional base row, then (+p, -p) rows for
    p = p_begin, p_begin + p_stride, ... < p_end (count of them; p_stride = 1: the range [p_begin, p_end))."""
    _chk_n(n, 1, CIRCUIT_MAX_N)
    dev = theta.device
    h = _ext.handle_for(dev)
    aid = ansatz_id(ansatz_type)
    _chk(theta, torch.float64, dev, "theta", num_params(ansatz_type, n, layers))
    count = len(range(p_begin, p_end, p_stride))
    B = (1 if include_base else 0) + 2 * count
    if out is None:
        out = torch.empty((B, 1 << n), dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out")
        if out.numel() != B << n:
            raise BornviError("out has the wrong size")
    if B == 0:
        return out
    need = _cached_size(h, "bornvi_circuit_workspace_bytes", aid, n, layers, B)
    ws = _ws(dev, min(need, max(WORKSPACE_CAP, _cached_size(h, "bornvi_circuit_workspace_bytes", aid, n, layers, 1))), ws_tag)
    h.call("bornvi_paramshift_probs_strided", aid, n, layers, _ptr(theta), int(p_begin), int(count), int(p_stride),
           1 if include_base else 0, _ptr(out), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out


def paramshift_dot_supported(ansatz_type, n, layers, dev, count):
    """True when the fused path exists for this plan (multi-pass plan of the 8-amplitude kernel, no prefix sharing) and
    its workspace -- every shifted state at once, no chunks -- fits WORKSPACE_CAP; else the caller takes the chunked
    path (paramshift_probs)."""
    h = _ext.handle_for(dev)
    key = (id(h), "dot_supported", ansatz_id(ansatz_type), int(n), int(layers), int(count))
    if key not in _size_cache:       # (a size of 0 is the library's "not available": no error)
        _size_cache[key] = int(_ext.lib().bornvi_paramshift_dot_workspace_bytes(h.h, ansatz_id(ansatz_type), int(n), int(layers), int(count)))
    return 0 < _size_cache[key] <= WORKSPACE_CAP    # (the cap is read on every call: it may change after the size was cached)


def paramshift_dot_begin(ansatz_type, n, layers, theta, p_begin, p_end, p_stride=1):
    """First half of a parameter-shift step with the dot product fused into the last circuit pass: runs the base circuit
    and the shifted circuits of p = p_begin, p_begin + p_stride, ... < p_end up to their last pass, and the base circuit
    to the end.  Returns (q [2^n], token); give the token to paramshift_dot_finish once y = K_p q is known."""
    _chk_n(n, 1, CIRCUIT_MAX_N)
    dev = theta.device
    h = _ext.handle_for(dev)
    aid = ansatz_id(ansatz_type)
    _chk(theta, torch.float64, dev, "theta", num_params(ansatz_type, n, layers))
    count = len(range(p_begin, p_end, p_stride))
    need = int(_cached_size(h, "bornvi_paramshift_dot_workspace_bytes", aid, n, layers, count))
    if need == 0:
        raise BornviError("the fused parameter-shift dot is not available for this plan (see paramshift_dot_supported)")
    ws = _ws(dev, need, "dot")
    q = torch.empty(1 << n, dtype=torch.float64, device=dev)
    h.call("bornvi_paramshift_dot_begin", aid, n, layers, _ptr(theta), int(p_begin), int(count), int(p_stride), _ptr(q), _ptr(ws),
           ws.numel(), _ext.stream_ptr(dev))
    return q, (aid, int(n), int(layers), count, ws)


def paramshift_dot_finish(token, w, ksd2=None):
    """Second half: the shifted circuits' last pass with the weights w [2^n] -> (loss [1] or None, grad [count]);
    ksd2 [1] given: grad carries the factor 1 / (2 sqrt(max(ksd2, 1e-12))) and loss = sqrt(max(ksd2, 1e-12)); else 1/2."""
    aid, n, layers, count, ws = token
    dev = w.device
    h = _ext.handle_for(dev)
    _chk(w, torch.float64, dev, "w", 1 << n)
    if ksd2 is not None:
        _chk(ksd2, torch.float64, dev, "ksd2", 1)
    grad = torch.empty(count, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev) if ksd2 is not None else None
    h.call("bornvi_paramshift_dot_finish", aid, n, layers, count, _ptr(w), _ptr(ksd2) if ksd2 is not None else None,
           _ptr(grad) if count else None, _ptr(loss) if loss is not None else None, _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return loss, grad


def paramshift_grad(ansatz_type, n, layers, theta, dLdq, p_begin, p_end, p_stride=1, shots=None):
    """grad[i] = 1/2 dLdq . (q(theta + pi/2 e_p) - q(theta - pi/2 e_p)) for p = p_begin + i p_stride < p_end, float64.
    shots = (S, seed, epoch tensor): the shifted distributions are replaced by histograms of S draws (shots_histogram)."""
    _chk_n(n, 1, CIRCUIT_MAX_N)
    dev = theta.device
    h = _ext.handle_for(dev)
    aid = ansatz_id(ansatz_type)
    _chk(theta, torch.float64, dev, "theta", num_params(ansatz_type, n, layers))
    _chk(dLdq, torch.float64, dev, "dLdq", 1 << n)
    ns = len(range(p_begin, p_end, p_stride))
    grad = torch.empty(ns, dtype=torch.float64, device=dev)
    if ns == 0:
        return grad
    shifted = paramshift_probs(ansatz_type, n, layers, theta, p_begin, p_end, include_base=False, p_stride=p_stride)
    if shots is not None:
        S, seed, epoch = shots
        shots_histogram(shifted, n, S, seed, epoch, include_base=False, p_begin=p_begin, p_stride=p_stride, out=shifted)
    return shifted_dot(n, shifted, ns, dLdq, out=grad)


def shifted_dot(n, shifted, n_shift, dLdq, out=None):
    """grad[i] = 1/2 dLdq . (shifted[2 i] - shifted[2 i + 1]) over stored (+p, -p) rows [2 n_shift, 2^n], float64: the
    finishing kernel with ksd2 = 1 (loss = 1, scale = 1/2)."""
    dev = dLdq.device
    h = _ext.handle_for(dev)
    _chk_n(n)
    _chk(dLdq, torch.float64, dev, "dLdq", 1 << n)
    grad = out if out is not None else torch.empty(n_shift, dtype=torch.float64, device=dev)
    _chk(grad, torch.float64, dev, "out", n_shift)
    if n_shift == 0:
        return grad
    _chk(shifted, torch.float64, dev, "shifted", (2 * n_shift) << n)
    one = torch.ones(1, dtype=torch.float64, device=dev)
    h.call("bornvi_ksd_grad_finish", n, _ptr(shifted), int(n_shift), _ptr(dLdq), _ptr(one), None, None, _ptr(grad),
           _ext.stream_ptr(dev))
    return grad


def adjoint_state(ansatz_type, n, layers, theta, want_probs=True):
    """OPT-IN adjoint engine, forward walk: theta float64 [P] -> (state complex128 [2^n], probs float64 [2^n] or None)."""
    _chk_n(n, 1, CIRCUIT_MAX_N)
    dev = theta.device
    h = _ext.handle_for(dev)
    aid = ansatz_id(ansatz_type)
    _chk(theta, torch.float64, dev, "theta", num_params(ansatz_type, n, layers))
    state = torch.empty(1 << n, dtype=torch.complex128, device=dev)
    probs = torch.empty(1 << n, dtype=torch.float64, device=dev) if want_probs else None
    ws = _ws(dev, _cached_size(h, "bornvi_adjoint_workspace_bytes", aid, n, layers), "adjoint")
    h.call("bornvi_adjoint_state", aid, n, layers, _ptr(theta), _ptr(state), _ptr(probs) if want_probs else None, _ptr(ws),
           ws.numel(), _ext.stream_ptr(dev))
    return state, probs


def adjoint_vjp(ansatz_type, n, layers, theta, state, dLdq):
    """OPT-IN adjoint engine, backward walk: grad[p] = d/dtheta_p sum_z dLdq[z] q_z(theta), float64 [P] -- the quantity
    paramshift_grad computes with 2P circuits, from one forward state and one backward walk."""
    _chk_n(n, 1, CIRCUIT_MAX_N)
    dev = theta.device
    h = _ext.handle_for(dev)
    aid = ansatz_id(ansatz_type)
    P = num_params(ansatz_type, n, layers)
    _chk(theta, torch.float64, dev, "theta", P)
    _chk(state, torch.complex128, dev, "state", 1 << n)
    _chk(dLdq, torch.float64, dev, "dLdq", 1 << n)
    grad = torch.zeros(P, dtype=torch.float64, device=dev)
    ws = _ws(dev, _cached_size(h, "bornvi_adjoint_workspace_bytes", aid, n, layers), "adjoint")
    h.call("bornvi_adjoint_vjp", aid, n, layers, _ptr(theta), _ptr(state), _ptr(dLdq), _ptr(grad), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return grad


def gate1q_apply(state, n, wire, U):
    """In-place one-qubit gate on state complex128 [B, 2^n] (one HBM round trip)."""
    dev = state.device
    h = _ext.handle_for(dev)
    _chk_n(n, 1, 40)
    _chk(state, torch.complex128, dev, "state")
    if state.numel() % (1 << n):
        raise BornviError("state: element count is not a multiple of 2^n")
    Uh = np.ascontiguousarray(np.asarray(U, dtype=np.complex128).reshape(4)).view(np.float64)
    arr = (C.c_double * 8)(*Uh.tolist())
    h.call("bornvi_gate1q_apply", n, state.numel() >> n, _ptr(state), int(wire), arr, _ext.stream_ptr(dev))
    return state


def cnot_apply(state, n, control, target):
    dev = state.device
    h = _ext.handle_for(dev)
    _chk_n(n, 2, 40)
    _chk(state, torch.complex128, dev, "state")
    if state.numel() % (1 << n):
        raise BornviError("state: element count is not a multiple of 2^n")
    h.call("bornvi_cnot_apply", n, state.numel() >> n, _ptr(state), int(control), int(target), _ext.stream_ptr(dev))
    return state


def born_probs(state, n):
    dev = state.device
    h = _ext.handle_for(dev)
    _chk_n(n, 0, 40)
    _chk(state, torch.complex128, dev, "state")
    if state.numel() % (1 << n):
        raise BornviError("state: element count is not a multiple of 2^n")
    probs = torch.empty(state.shape, dtype=torch.float64, device=dev)
    h.call("bornvi_born_probs", n, state.numel() >> n, _ptr(state), _ptr(probs), _ext.stream_ptr(dev))
    return probs


# ---- classical Born machine (probability table) ------------------------------------------------------------
BORN_TABLE_MAX_ROWS = _ext.LIMITS["BORNVI_BORN_TABLE_MAX_ROWS"]


def _born_table_args(w, mode):
    """(rows, n) of a raw-parameter table w [rows, 2^n]; every argument error is raised here, before any GPU call."""
    if isinstance(mode, bool) or mode not in (0, 1):
        raise BornviError(f"born-table mode must be 0 (softmax) or 1 (|w| / sum |w|), got {mode!r}")
    if not torch.is_tensor(w) or w.dim() != 2:
        raise BornviError(f"w: expected a [rows, 2^n] tensor, got {tuple(w.shape) if torch.is_tensor(w) else type(w)}")
    rows, N = int(w.shape[0]), int(w.shape[1])
    if N < 1 or N & (N - 1):
        raise BornviError(f"w: row length {N} is not a power of two")
    if not 1 <= rows <= BORN_TABLE_MAX_ROWS:
        raise BornviError(f"w: 1 ... {BORN_TABLE_MAX_ROWS} rows per call, got {rows}")
    n = N.bit_length() - 1
    _chk_n(n, 0, 30)
    return rows, n


def born_table_probs(w, mode, want_entropy=True):
    """Classical Born machine forward (bornvi_born_table_probs): raw parameters w float32 [rows, 2^n] on the GPU ->
    (q32 float32 [rows, 2^n], q64 = its exact float64 upcast, H float32 [rows] or None).  mode 0: softmax(w - max w),
    1: |w| / sum |w|; H = -sum q log max(q, 1e-10) over q32."""
    rows, n = _born_table_args(w, mode)
    dev = w.device
    h = _ext.handle_for(dev)
    _chk(w, torch.float32, dev, "w")
    q32 = torch.empty(w.shape, dtype=torch.float32, device=dev)
    q64 = torch.empty(w.shape, dtype=torch.float64, device=dev)
    H = torch.empty(rows, dtype=torch.float32, device=dev) if want_entropy else None
    ws = _ws(dev, _cached_size(h, "bornvi_born_table_workspace_bytes", n, rows), "born_table")
    h.call("bornvi_born_table_probs", n, rows, int(mode), _ptr(w), _ptr(q32), _ptr(q64), _ptr(H) if H is not None else None,
           _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return q32, q64, H


def born_table_vjp(w, q64, mode, y=None, ksd2=None, entropy_weight=0.0, out=None, loss_out=None):
    """Classical Born machine backward (bornvi_born_table_vjp): float32 [rows, 2^n] d/dw of
    sqrt(max(ksd2, 1e-12)) - entropy_weight * H per row.  y float64 [rows, 2^n] = K_p q (None: no KSD term); ksd2 float64
    [rows] (None with y given: y is dL/dq itself); entropy_weight 0: no entropy term.  out: destination (e.g. a
    parameter's .grad); loss_out float64 [rows]: receives sqrt(max(ksd2, 1e-12))."""
    rows, n = _born_table_args(w, mode)
    try:
        lam = float(entropy_weight)
    except (TypeError, ValueError):
        raise BornviError(f"entropy_weight must be a number, got {entropy_weight!r}") from None
    if not np.isfinite(lam):
        raise BornviError(f"entropy_weight must be finite, got {entropy_weight!r}")
    if loss_out is not None and ksd2 is None:
        raise BornviError("loss_out needs ksd2")
    dev = w.device
    h = _ext.handle_for(dev)
    _chk(w, torch.float32, dev, "w")
    _chk(q64, torch.float64, dev, "q64", w.numel())
    if y is not None:
        _chk(y, torch.float64, dev, "y", w.numel())
    if ksd2 is not None:
        _chk(ksd2, torch.float64, dev, "ksd2", rows)
    if loss_out is not None:
        _chk(loss_out, torch.float64, dev, "loss_out", rows)
    if out is None:
        out = torch.empty(w.shape, dtype=torch.float32, device=dev)
    else:
        _chk(out, torch.float32, dev, "out", w.numel())
    ws = _ws(dev, _cached_size(h, "bornvi_born_table_workspace_bytes", n, rows), "born_table")
    h.call("bornvi_born_table_vjp", n, rows, int(mode), _ptr(w), _ptr(q64), _ptr(y) if y is not None else None,
           _ptr(ksd2) if ksd2 is not None else None, lam, _ptr(out), _ptr(loss_out) if loss_out is not None else None,
           _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out


REINFORCE_MAX_BATCH = _ext.LIMITS["BORNVI_REINFORCE_MAX_BATCH"]


def reinforce_step(idx, logit, log_p, q32, baseline, first, baseline_decay, entropy_coef=0.01, q_floor=1e-10, out=None,
                   loss_out=None, found_out=None):
    """REINFORCE step of the table family (bornvi_reinforce_step): idx int64 [B] sampled outcomes, logit float32 [B]
    classifier logits of the samples, log_p float32 [2^n] = log p(x_obs | z), q32 float32 [2^n] the Born probabilities,
    baseline float64 [1] running baseline (updated in place: the first call's mean reward, then the exponential average)
    -> (dLdq float64 [2^n] = d loss_q / d q, the y of born_table_vjp(ksd2=None); loss float32 [1]; found_inf float32 [1],
    1.0 when the loss is NaN or +-Inf).  out / loss_out / found_out: destinations to write into."""
    dev = q32.device
    h = _ext.handle_for(dev)
    N = int(q32.numel())
    if N < 2 or N & (N - 1):
        raise BornviError(f"q32: {N} entries is not 2^n with n >= 1")
    n = N.bit_length() - 1
    _chk_n(n)
    B = int(idx.numel())
    if not 1 <= B <= REINFORCE_MAX_BATCH:
        raise BornviError(f"idx: 1 ... 2^24 samples per call, got {B}")
    for name, v in (("baseline_decay", baseline_decay), ("entropy_coef", entropy_coef), ("q_floor", q_floor)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise BornviError(f"{name} must be a finite number, got {v!r}")
    if q_floor < 0:
        raise BornviError(f"q_floor must not be negative, got {q_floor!r}")
    _chk(idx, torch.int64, dev, "idx")
    _chk(logit, torch.float32, dev, "logit", B)
    _chk(log_p, torch.float32, dev, "log_p", N)
    _chk(q32, torch.float32, dev, "q32")
    _chk(baseline, torch.float64, dev, "baseline", 1)
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", N)
    if loss_out is None:
        loss_out = torch.empty(1, dtype=torch.float32, device=dev)
    else:
        _chk(loss_out, torch.float32, dev, "loss_out", 1)
    if found_out is None:
        found_out = torch.empty(1, dtype=torch.float32, device=dev)
    else:
        _chk(found_out, torch.float32, dev, "found_out", 1)
    ws = _ws(dev, _cached_size(h, "bornvi_reinforce_workspace_bytes", n, B), "reinforce")
    h.call("bornvi_reinforce_step", n, B, _ptr(idx), _ptr(logit), _ptr(log_p), _ptr(q32), _ptr(baseline), 1 if first else 0,
           float(baseline_decay), float(entropy_coef), float(q_floor), _ptr(out), _ptr(loss_out), _ptr(found_out),
           _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out, loss_out, found_out


# ---- exact ELBO ---------------------------------------------------------------------------------------
ELBO_MAX_ROWS = _ext.LIMITS["BORNVI_ELBO_MAX_ROWS"]


def elbo_weights(q, log_p, q_floor=1e-10, want_w=True, want_entropy=True, out=None):
    """Exact ELBO of Born distributions against a log-joint table (bornvi_elbo_weights): q float64 [rows, 2^n] (or
    [2^n]) on the GPU, log_p float64 [2^n] = log p(x, z), finite -> (neg_elbo [rows] = sum q (l - log_p), entropy [rows]
    = -sum q l or None, w [rows, 2^n] = l - log_p + [q >= q_floor] = d neg_elbo / d q or None), l = log max(q, q_floor).
    out: destination of w (same element count as q).  Every argument error is raised here, before any GPU call."""
    if not torch.is_tensor(q) or not torch.is_tensor(log_p) or q.dim() not in (1, 2) or log_p.dim() != 1:
        raise BornviError("elbo_weights: q must be a [rows, 2^n] or [2^n] tensor and log_p a [2^n] tensor")
    N = int(log_p.numel())
    if N < 2 or N & (N - 1):
        raise BornviError(f"log_p: {N} entries is not 2^n with n >= 1")
    n = N.bit_length() - 1
    _chk_n(n)
    if q.shape[-1] != N:
        raise BornviError(f"q: rows of {int(q.shape[-1])} entries against a log_p of {N}")
    rows = int(q.numel()) // N
    if not 1 <= rows <= ELBO_MAX_ROWS:
        raise BornviError(f"q: 1 ... {ELBO_MAX_ROWS} rows per call, got {rows}")
    if isinstance(q_floor, bool) or not isinstance(q_floor, (int, float, np.integer, np.floating)) \
            or not np.isfinite(q_floor) or not q_floor > 0:
        raise BornviError(f"q_floor must be a positive finite number, got {q_floor!r}")
    if out is not None and not want_w:
        raise BornviError("elbo_weights: out is the destination of w, which want_w=False leaves out")
    dev = q.device
    h = _ext.handle_for(dev)
    _chk(q, torch.float64, dev, "q")
    _chk(log_p, torch.float64, dev, "log_p")
    w = None
    if want_w:
        w = out if out is not None else torch.empty(q.shape, dtype=torch.float64, device=dev)
        _chk(w, torch.float64, dev, "out", q.numel())
    neg_elbo = torch.empty(rows, dtype=torch.float64, device=dev)
    entropy = torch.empty(rows, dtype=torch.float64, device=dev) if want_entropy else None
    ws = _ws(dev, _cached_size(h, "bornvi_elbo_workspace_bytes", n, rows), "elbo")
    h.call("bornvi_elbo_weights", n, rows, _ptr(q), _ptr(log_p), float(q_floor), _ptr(w) if w is not None else None,
           _ptr(neg_elbo), _ptr(entropy) if entropy is not None else None, _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return neg_elbo, entropy, w


# ---- MMD with a Hamming-distance kernel (include/bornvi_mmd.h) --------------------------------------------------
MMD_TILE_BITS = _ext.MMD_LIMITS["BORNVI_MMD_TILE_BITS"]
MMD_HIGH_BITS = _ext.MMD_LIMITS["BORNVI_MMD_HIGH_BITS"]
MMD_MAX_SCALES = _ext.MMD_LIMITS["BORNVI_MMD_MAX_SCALES"]
HAMMING_PAIRS_MAX_A = _ext.MMD_LIMITS["BORNVI_HAMMING_PAIRS_MAX_A"]
HAMMING_PAIRS_MAX_B = _ext.MMD_LIMITS["BORNVI_HAMMING_PAIRS_MAX_B"]


def mmd_passes(n):
    """Tile passes of mmd_weights with w at n variables (bornvi_mmd_passes: 1, 3 or 5; host only, no GPU needed)."""
    _chk_n(n)
    return int(_ext.lib().bornvi_mmd_passes(int(n)))


def mmd_weights(q, target, lam, want_w=True, out=None):
    """Squared MMD of q against target under the kernel whose Walsh-Hadamard spectrum is lam (bornvi_mmd_weights): q float64
    [2^n] on the GPU, target float64 [2^n] or None (zeros), lam float64 [n + 1] -> (loss [1] = d^T K d with d = q - target,
    w [2^n] = 2 K d or None).  out: destination of w.  Every argument error is raised here, before any GPU call."""
    if not torch.is_tensor(q) or not torch.is_tensor(lam) or q.dim() != 1 or lam.dim() != 1:
        raise BornviError("mmd_weights: q must be a [2^n] tensor and lam a [n + 1] tensor")
    N = int(q.numel())
    if N < 2 or N & (N - 1):
        raise BornviError(f"q: {N} entries is not 2^n with n >= 1")
    n = N.bit_length() - 1
    _chk_n(n)
    if int(lam.numel()) != n + 1:
        raise BornviError(f"lam: expected {n + 1} entries (n = {n}), got {int(lam.numel())}")
    if target is not None and (not torch.is_tensor(target) or target.dim() != 1):
        raise BornviError("mmd_weights: target must be a [2^n] tensor or None")
    if out is not None and not want_w:
        raise BornviError("mmd_weights: out is the destination of w, which want_w=False leaves out")
    dev = q.device
    h = _ext.handle_for(dev)
    _chk(q, torch.float64, dev, "q")
    _chk(lam, torch.float64, dev, "lam")
    if target is not None:
        _chk(target, torch.float64, dev, "target", N)
    w = None
    if want_w:
        w = out if out is not None else torch.empty(N, dtype=torch.float64, device=dev)
        _chk(w, torch.float64, dev, "out", N)
    for name, t in (("q", q), ("target", target), ("out", w)):
        if t is not None and t.data_ptr() % 16:
            raise BornviError(f"{name}: the storage must be 16-byte aligned")
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    ws = _ws(dev, _cached_size(h, "bornvi_mmd_workspace_bytes", n), "mmd")
    h.call("bornvi_mmd_weights", n, _ptr(q), _ptr(target) if target is not None else None, _ptr(lam), _ptr(loss),
           _ptr(w) if w is not None else None, _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return loss, w


def hamming_pairs_rowsum(za, zb, kappa, skip_same_index=False, want_counts=False):
    """Row sums of a Hamming-distance kernel between two lists of states (bornvi_hamming_pairs_rowsum): za int64 [A], zb int64
    [B], kappa float64 [n + 1] -> (r float64 [A], r_a = sum_j kappa[popcount(za_a xor zb_j)], without j = a when
    skip_same_index; total float64 [1] = sum_a r_a; counts int32 [A, n + 1] or None).  1 <= A <= 2^17, 1 <= B <= 2^20; the
    states' bits at or above n must be 0.  Every argument error is raised here, before any GPU call."""
    if not torch.is_tensor(kappa) or kappa.dim() != 1 or not 2 <= int(kappa.numel()) <= MPS_SAMPLED_MAX_N + 1:
        raise BornviError("kappa: expected a [n + 1] float64 tensor, 1 <= n <= 63")
    n = int(kappa.numel()) - 1
    if not torch.is_tensor(za) or za.dim() != 1 or not 1 <= int(za.numel()) <= HAMMING_PAIRS_MAX_A:
        raise BornviError("za: expected a [A] int64 tensor, 1 <= A <= 2^17")
    if not torch.is_tensor(zb) or zb.dim() != 1 or not 1 <= int(zb.numel()) <= HAMMING_PAIRS_MAX_B:
        raise BornviError("zb: expected a [B] int64 tensor, 1 <= B <= 2^20")
    dev = za.device
    h = _ext.handle_for(dev)
    A, B = int(za.numel()), int(zb.numel())
    _chk(za, torch.int64, dev, "za")
    _chk(zb, torch.int64, dev, "zb")
    _chk(kappa, torch.float64, dev, "kappa")
    r = torch.empty(A, dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    counts = torch.empty((A, n + 1), dtype=torch.int32, device=dev) if want_counts else None
    ws = _ws(dev, _cached_size(h, "bornvi_hamming_pairs_workspace_bytes", n, A, B), f"hamming_pairs_{n}_{A}_{B}")
    h.call("bornvi_hamming_pairs_rowsum", n, A, _ptr(za), B, _ptr(zb), 1 if skip_same_index else 0, _ptr(kappa), _ptr(r), _ptr(total),
           _ptr(counts) if counts is not None else None, _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return r, total, counts


# ---- matrix-product-state Born machine -------------------------------------------------------------------
MPS_MAX_N =_ext.LIMITS["BORNVI_MPS_MAX_N"]
MPS_MAX_BOND = _ext.LIMITS["BORNVI_MPS_MAX_BOND"]


_ENUMERATED = object()


def _mps_args(cores, num_samples=_ENUMERATED):
    """(n, D) of cores [n, 2, D, D] for the enumerated calls (n <= MPS_MAX_N), or (n, D, B) with a sample count for the
    sampled ones (n <= MPS_SAMPLED_MAX_N); every argument error is raised here, before any GPU call."""
    if not torch.is_tensor(cores) or cores.dim() != 4 or cores.shape[1] != 2 or cores.shape[2] != cores.shape[3]:
        raise BornviError(f"cores: expected an [n, 2, D, D] tensor, got {tuple(cores.shape) if torch.is_tensor(cores) else type(cores)}")
    n, D, B = int(cores.shape[0]), int(cores.shape[2]), num_samples
    _chk_n(n, 1, MPS_MAX_N if B is _ENUMERATED else MPS_SAMPLED_MAX_N)
    if not 1 <= D <= MPS_MAX_BOND:
        raise BornviError(f"cores: bond dimension 1 ... {MPS_MAX_BOND}, got {D}")
    if B is _ENUMERATED:
        return n, D
    return n, D, _sample_count(B)


def mps_probs(cores, want_q32=True, want_psi=False):
    """MPS Born machine forward (bornvi_mps_probs): cores float64 [n, 2, D, D] on the GPU -> (q32 float32 [2^n] or None,
    q64 float64 [2^n], psi float64 [2^n] or None, Z float64 [1]).  Leaves the sweep's levels, psi and Z in the cached
    workspace for mps_vjp: call that next, with the same cores, before another mps_probs of this shape on this stream."""
    n, D = _mps_args(cores)
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    N = 1 << n
    q64 = torch.empty(N, dtype=torch.float64, device=dev)
    q32 = torch.empty(N, dtype=torch.float32, device=dev) if want_q32 else None
    psi = torch.empty(N, dtype=torch.float64, device=dev) if want_psi else None
    Z = torch.empty(1, dtype=torch.float64, device=dev)
    ws = _ws(dev, _cached_size(h, "bornvi_mps_workspace_bytes", n, D), "mps")
    h.call("bornvi_mps_probs", n, D, _ptr(cores), _ptr(q64), _ptr(q32) if q32 is not None else None,
           _ptr(psi) if psi is not None else None, _ptr(Z), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return q32, q64, psi, Z


def mps_vjp(cores, g, out=None):
    """MPS Born machine backward (bornvi_mps_vjp): float64 [n, 2, D, D] = dL/dcores from g = dL/dq float64 [2^n], through
    what the last mps_probs(cores) left in the cached workspace.  out: destination (e.g. a parameter's .grad)."""
    n, D = _mps_args(cores)
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    _chk(g, torch.float64, dev, "g", 1 << n)
    if out is None:
        out = torch.empty(cores.shape, dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", cores.numel())
    ws = _ws(dev, _cached_size(h, "bornvi_mps_workspace_bytes", n, D), "mps")
    h.call("bornvi_mps_vjp", n, D, _ptr(cores), _ptr(g), _ptr(out), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out


# ---- sampled MPS Born machine (no 2^n object) -------------------------------------------------------------
MPS_SAMPLED_MAX_N = _ext.LIMITS["BORNVI_MPS_SAMPLED_MAX_N"]
MPS_SAMPLED_MAX_BATCH = _ext.LIMITS["BORNVI_MPS_SAMPLED_MAX_BATCH"]


class _SampledFamily(NamedTuple):
    """What tells the three sampled families' calls apart on the host (the real, the complex-cores and the purified one)."""
    prefix: str          # the entry points are bornvi_<prefix>_environments / _sample / _score_vjp
    args: Callable       # (cores, num_samples) -> the entry points' leading integers (..., B); raises every argument error
    size_query: str      # the workspace size query's symbol, taking those integers
    tag: str             # the workspace tag: the family's prefix and a %d for each of those integers


def _sampled_ws(fam, h, dev, dims):
    """One workspace per family, dims and stream: the environments call leaves the environments in it for the two after it."""
    return _ws(dev, _cached_size(h, fam.size_query, *dims), fam.tag % dims)


def _sampled_environments(fam, cores, num_samples):
    dims = fam.args(cores, num_samples)
    dev = cores.device
    _chk(cores, torch.float64, dev, "cores")
    h = _ext.handle_for(dev)
    log_Z = torch.empty(1, dtype=torch.float64, device=dev)
    ws = _sampled_ws(fam, h, dev, dims)
    h.call(f"bornvi_{fam.prefix}_environments", *dims, _ptr(cores), _ptr(log_Z), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return log_Z


def _sampled_sample(fam, cores, num_samples, seed, epoch, out_idx, second, status, second_dtype=torch.float64,
                    second_name="out_logq", second_cols=None, want_second=True):
    """-> (idx, second, status).  second: the sampler's per-sample output beside idx (logq float64 [B], or with second_cols = 2
    the purified family's aux int64 [B, 2]), filled when given or when want_second, else None and a NULL pointer."""
    dims = fam.args(cores, num_samples)
    B = dims[-1]
    dev = cores.device
    _chk(cores, torch.float64, dev, "cores")
    seed = _seed_word(seed)
    if not torch.is_tensor(epoch):
        raise BornviError("epoch: expected an int64 device tensor [1]")
    _chk(epoch, torch.int64, dev, "epoch", 1)
    h = _ext.handle_for(dev)
    out_idx = _out(out_idx, torch.int64, dev, "out_idx", B)
    if second is not None or want_second:
        second = _out(second, second_dtype, dev, second_name, B if second_cols is None else (B, second_cols))
    status = _out(status, torch.int32, dev, "status", 1)
    ws = _sampled_ws(fam, h, dev, dims)
    h.call(f"bornvi_{fam.prefix}_sample", *dims, _ptr(cores), seed, _ptr(epoch), _ptr(out_idx),
           _ptr(second) if second is not None else None, _ptr(status), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out_idx, second, status


def _sampled_score(fam, cores, idx, w, out, out_logq, status, gradient_optional=False):
    """-> (grad, logq, status).  gradient_optional: out=False asks for logq alone (then w may be None) -> grad None."""
    if not torch.is_tensor(idx) or idx.dim() != 1:
        raise BornviError("idx: expected a [B] int64 tensor")
    dims = fam.args(cores, int(idx.numel()))
    B = dims[-1]
    dev = cores.device
    _chk(cores, torch.float64, dev, "cores")
    _chk(idx, torch.int64, dev, "idx", B)
    want = not (gradient_optional and out is False)
    if want or w is not None:
        if not torch.is_tensor(w):
            raise BornviError("w: expected a [B] float64 tensor")
        _chk(w, torch.float64, dev, "w", B)
    h = _ext.handle_for(dev)
    out = _out(out, torch.float64, dev, "out", tuple(cores.shape)) if want else None
    out_logq = _out(out_logq, torch.float64, dev, "out_logq", B)
    status = _out(status, torch.int32, dev, "status", 1)
    ws = _sampled_ws(fam, h, dev, dims)
    h.call(f"bornvi_{fam.prefix}_score_vjp", *dims, _ptr(cores), _ptr(idx), _ptr(w) if w is not None else None, _ptr(out_logq),
           _ptr(out) if want else None, _ptr(status), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out, out_logq, status


_MPS = _SampledFamily("mps", _mps_args, "bornvi_mps_sample_workspace_bytes", "mps_sampled_%d_%d_%d")


def _mps_sampled_ws(h, dev, n, D, B):
    """The real family's workspace of (n, D, B): the Fisher and Stein calls read the environments mps_environments left in it."""
    return _sampled_ws(_MPS, h, dev, (n, D, B))


def mps_environments(cores, num_samples):
    """Left and right environments of an MPS and log Z (bornvi_mps_environments): cores float64 [n, 2, D, D] on the GPU,
    1 <= n <= 63 -> log Z float64 [1].  The environments stay in the cached workspace of (n, D, num_samples) for
    mps_sample and mps_score_vjp: call those next, with the same cores and sample count, on this stream."""
    return _sampled_environments(_MPS, cores, num_samples)


def mps_sample(cores, num_samples, seed, epoch, out_idx=None, out_logq=None, status=None):
    """Exact ancestral draws from an MPS Born machine (bornvi_mps_sample), after mps_environments(cores, num_samples):
    -> (idx int64 [B] outcome indices, logq float64 [B] = log q(idx), status int32 [1]: 0, or 1 when a sample met
    conditional masses summing to 0 or a non-finite number).  Draw k of sample b is a pure function of (seed, epoch, b, k).
    epoch: an int64 device tensor [1] (read by the kernel: a captured graph sees its value at replay time)."""
    return _sampled_sample(_MPS, cores, num_samples, seed, epoch, out_idx, out_logq, status)


def mps_score_vjp(cores, idx, w, out=None, out_logq=None, status=None):
    """Score-function gradient of an MPS Born machine (bornvi_mps_score_vjp), after mps_environments(cores, len(idx)):
    idx int64 [B] outcome indices in [0, 2^n), w float64 [B] -> (grad float64 [n, 2, D, D] = sum_b w_b grad log q(idx_b),
    logq float64 [B], status int32 [1]: 0, or 2 when some psi(idx_b) is 0 or not finite).  out: destination of grad."""
    return _sampled_score(_MPS, cores, idx, w, out, out_logq, status)


# ---- sampled MPS Born machine with complex cores (kernels_cmps.hip, include/bornvi_cmps.h) ----------
CMPS_MAX_BOND = _ext.CMPS_LIMITS["BORNVI_CMPS_MAX_BOND"]


def _cmps_args(cores, num_samples):
    """(n, D, B) of complex cores float64 [n, 2, D, D, 2] ((re, im) last) and a sample count; every argument error is raised
    here, before any GPU call."""
    if not torch.is_tensor(cores) or cores.dim() != 5 or cores.shape[1] != 2 or cores.shape[2] != cores.shape[3] or cores.shape[4] != 2:
        raise BornviError(f"cores: expected an [n, 2, D, D, 2] tensor (re, im last), got "
                          f"{tuple(cores.shape) if torch.is_tensor(cores) else type(cores)}")
    n, D = int(cores.shape[0]), int(cores.shape[2])
    _chk_n(n, 1, MPS_SAMPLED_MAX_N)
    if not 1 <= D <= CMPS_MAX_BOND:
        raise BornviError(f"cores: complex bond dimension 1 ... {CMPS_MAX_BOND}, got {D}")
    return n, D, _sample_count(num_samples)


_CMPS = _SampledFamily("cmps", _cmps_args, "bornvi_cmps_workspace_bytes", "cmps_%d_%d_%d")


def cmps_environments(cores, num_samples):
    """Left and right environments of a complex MPS and log Z (bornvi_cmps_environments): cores float64 [n, 2, D, D, 2] on the
    GPU, 1 <= n <= 63, 1 <= D <= 16 -> log Z float64 [1].  The environments stay in the cached workspace of (n, D, num_samples)
    for cmps_sample and cmps_score_vjp: call those next, with the same cores and sample count, on this stream."""
    return _sampled_environments(_CMPS, cores, num_samples)


def cmps_sample(cores, num_samples, seed, epoch, out_idx=None, out_logq=None, status=None):
    """Exact ancestral draws from a complex MPS Born machine (bornvi_cmps_sample), after cmps_environments(cores, num_samples):
    -> (idx int64 [B], logq float64 [B], status int32 [1]) as mps_sample; the uniforms are mps_sample's at (seed, epoch, b, k)."""
    return _sampled_sample(_CMPS, cores, num_samples, seed, epoch, out_idx, out_logq, status)


def cmps_score_vjp(cores, idx, w, out=None, out_logq=None, status=None):
    """Score-function gradient of a complex MPS Born machine (bornvi_cmps_score_vjp), after cmps_environments(cores, len(idx)):
    idx int64 [B], w float64 [B] -> (grad float64 [n, 2, D, D, 2] = the gradient of sum_b w_b log q(idx_b) in the real and
    imaginary parts of cores, logq float64 [B], status int32 [1]: 0, or 2 when some psi(idx_b) is 0 or not finite)."""
    return _sampled_score(_CMPS, cores, idx, w, out, out_logq, status)


# ---- sampled MPS Born machine as a locally purified state (kernels_lps.hip, include/bornvi_lps.h) ----
LPS_MAX_BOND = _ext.LPS_LIMITS["BORNVI_LPS_MAX_BOND"]
LPS_MAX_PURIFICATION = _ext.LPS_LIMITS["BORNVI_LPS_MAX_PURIFICATION"]


def _lps_args(cores, num_samples):
    """(n, m, D, B) of purified cores float64 [n, 2, m, D, D] and a sample count; every argument error is raised here, before
    any GPU call."""
    if not torch.is_tensor(cores) or cores.dim() != 5 or cores.shape[1] != 2 or cores.shape[3] != cores.shape[4]:
        raise BornviError(f"cores: expected an [n, 2, m, D, D] tensor, got "
                          f"{tuple(cores.shape) if torch.is_tensor(cores) else type(cores)}")
    n, m, D = int(cores.shape[0]), int(cores.shape[2]), int(cores.shape[3])
    _chk_n(n, 1, MPS_SAMPLED_MAX_N)
    if not 1 <= D <= LPS_MAX_BOND:
        raise BornviError(f"cores: purified bond dimension 1 ... {LPS_MAX_BOND}, got {D}")
    if not 1 <= m <= LPS_MAX_PURIFICATION:
        raise BornviError(f"cores: purification dimension 1 ... {LPS_MAX_PURIFICATION}, got {m}")
    return n, m, D, _sample_count(num_samples)


_LPS = _SampledFamily("lps", _lps_args, "bornvi_lps_workspace_bytes", "lps_%d_%d_%d_%d")


def lps_environments(cores, num_samples):
    """Left and right environments of a locally purified MPS and log Z (bornvi_lps_environments): cores float64
    [n, 2, m, D, D] on the GPU, 1 <= n <= 63, 1 <= D <= 16, 1 <= m <= 4 -> log Z float64 [1].  The environments stay in the
    cached workspace of (n, m, D, num_samples) for lps_sample and lps_score_vjp: call those next, with the same cores and
    sample count, on this stream."""
    return _sampled_environments(_LPS, cores, num_samples)


def lps_sample(cores, num_samples, seed, epoch, out_idx=None, out_aux=None, status=None, want_aux=False):
    """Exact draws from a locally purified MPS (bornvi_lps_sample), after lps_environments(cores, num_samples):
    -> (idx int64 [B], aux int64 [B, 2] or None, status int32 [1]).  The uniforms are mps_sample's at (seed, epoch, b, k).
    aux (want_aux, or an out_aux to fill) holds the purification indices drawn beside the bits, two bits a site; there is
    no logq here (lps_score_vjp with out=False gives it)."""
    return _sampled_sample(_LPS, cores, num_samples, seed, epoch, out_idx, out_aux, status, second_dtype=torch.int64,
                           second_name="out_aux", second_cols=2, want_second=want_aux)


def lps_score_vjp(cores, idx, w=None, out=None, out_logq=None, status=None):
    """log q and the score-function gradient of a locally purified MPS (bornvi_lps_score_vjp), after
    lps_environments(cores, len(idx)): idx int64 [B], w float64 [B] -> (grad float64 [n, 2, m, D, D] = the gradient of
    sum_b w_b log q(idx_b), logq float64 [B], status int32 [1]: 0, or 2 when some T(idx_b) is 0 or not finite).
    out=False (then w may be None): logq only, the same bits, no right sweep and no gradient work -> (None, logq, status)."""
    return _sampled_score(_LPS, cores, idx, w, out, out_logq, status, gradient_optional=True)


# ---- sampled Born machine on a binary tree tensor network (kernels_ttn.hip, include/bornvi_ttn.h) ----
TTN_MAX_BOND = _ext.TTN_LIMITS["BORNVI_TTN_MAX_BOND"]


def ttn_tree_shape(num_latent_vars):
    """(h, L) of the tree over n variables: h = max(1, ceil(log2 n)) levels of nodes, L = 2^h leaf positions."""
    _chk_n(num_latent_vars, 1, MPS_SAMPLED_MAX_N)
    h = max(1, (int(num_latent_vars) - 1).bit_length())
    return h, 1 << h


def _ttn_family(num_latent_vars):
    """The family record of the tree over n variables: the cores [L - 1, D, D, D] do not say n (positions >= n are padding)."""
    if isinstance(num_latent_vars, bool) or not isinstance(num_latent_vars, int):
        raise BornviError(f"num_latent_vars: expected an integer, got {num_latent_vars!r}")
    _, L = ttn_tree_shape(num_latent_vars)

    def args(cores, num_samples):
        if not torch.is_tensor(cores) or cores.dim() != 4 or not cores.shape[1] == cores.shape[2] == cores.shape[3] or cores.shape[0] != L - 1:
            raise BornviError(f"cores: expected an [L - 1, D, D, D] tensor with L = {L} (n = {num_latent_vars}), got "
                              f"{tuple(cores.shape) if torch.is_tensor(cores) else type(cores)}")
        D = int(cores.shape[1])
        if not 2 <= D <= TTN_MAX_BOND:
            raise BornviError(f"cores: tree bond dimension 2 ... {TTN_MAX_BOND}, got {D}")
        return num_latent_vars, D, _sample_count(num_samples)
    return _SampledFamily("ttn", args, "bornvi_ttn_workspace_bytes", "ttn_%d_%d_%d")


def ttn_environments(cores, num_latent_vars, num_samples):
    """Up and down densities of a tree tensor network and log Z (bornvi_ttn_environments): cores float64 [L - 1, D, D, D] on
    the GPU, 1 <= n <= 63, 2 <= D <= 8 -> log Z float64 [1].  The environments stay in the cached workspace of
    (n, D, num_samples) for ttn_sample and ttn_score_vjp: call those next, with the same cores and sample count, on this stream."""
    return _sampled_environments(_ttn_family(num_latent_vars), cores, num_samples)


def ttn_sample(cores, num_latent_vars, num_samples, seed, epoch, out_idx=None, out_logq=None, status=None):
    """Exact depth-first draws from a tree tensor network (bornvi_ttn_sample), after ttn_environments: -> (idx int64 [B],
    logq float64 [B], status int32 [1]) as mps_sample; the uniforms are mps_sample's at (seed, epoch, b, k = position + 1)."""
    return _sampled_sample(_ttn_family(num_latent_vars), cores, num_samples, seed, epoch, out_idx, out_logq, status)


def ttn_score_vjp(cores, num_latent_vars, idx, w=None, out=None, out_logq=None, status=None):
    """log q and the score-function gradient of a tree tensor network (bornvi_ttn_score_vjp), after ttn_environments(cores, n,
    len(idx)): idx int64 [B], w float64 [B] -> (grad float64 [L - 1, D, D, D] = the gradient of sum_b w_b log q(idx_b), exactly
    0.0 in the dead entries, logq float64 [B], status int32 [1]: 0, or 2 when some psi(idx_b) is 0 or not finite).
    out=False (then w may be None): logq only, the same bits, no down sweep and no gradient work -> (None, logq, status)."""
    return _sampled_score(_ttn_family(num_latent_vars), cores, idx, w, out, out_logq, status, gradient_optional=True)


# ---- exact posterior queries of the sampled MPS (kernels_mps_query.hip) ----------------------------------------------
MPS_QUERY_MAX_QUERIES = _ext.LIMITS["BORNVI_MPS_QUERY_MAX_QUERIES"]


def _mps_query_ws(h, dev, n, D, Q):
    return _ws(dev, _cached_size(h, "bornvi_mps_query_workspace_bytes", n, D, Q), f"mps_query_{n}_{D}_{Q}")


def mps_log_marginals(cores, mask, value, out=None, status=None):
    """Log probabilities of partial assignments under an MPS Born machine (bornvi_mps_log_marginals): mask, value int64 [Q]
    on the GPU (a set mask bit clamps tuple position p = bit n - 1 - p to the value's bit), 1 <= Q <= 2^16 ->
    (logm float64 [Q], status int32 [1]: 0, or 1 when some evidence has probability zero (logm -inf) or met a non-finite
    environment (NaN)).  An empty mask gives exactly 0.0, a full one log q of that state.  Needs no mps_environments."""
    n, D, _ = _mps_args(cores, 1)
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    Q = _evidence_args(mask, value, dev)
    out = _out(out, torch.float64, dev, "out", Q)
    status = _out(status, torch.int32, dev, "status", 1)
    ws = _mps_query_ws(h, dev, n, D, Q)
    h.call("bornvi_mps_log_marginals", n, D, Q, _ptr(cores), _ptr(mask), _ptr(value), _ptr(out), _ptr(status), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return out, status


def mps_sample_clamped(cores, num_samples, mask, value, seed, epoch, out_idx=None, out_logq=None, out_logm=None, status=None):
    """Exact draws from q(. | evidence) of an MPS Born machine (bornvi_mps_sample_clamped): mask, value int64 [1] on the
    GPU -> (idx int64 [B], logq float64 [B] = log q(idx | evidence), logm float64 [1] = the evidence's log marginal,
    status int32 [1]: 0, or 1 when a sample died (logq NaN) or the evidence has probability zero).  seed and epoch as
    mps_sample: with an empty mask idx and logq are mps_environments + mps_sample's bit for bit.  Needs no mps_environments."""
    n, D, B = _mps_args(cores, num_samples)
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    seed = _seed_word(seed)
    _chk(epoch, torch.int64, dev, "epoch", 1)
    _evidence_args(mask, value, dev, 1)
    out_idx = _out(out_idx, torch.int64, dev, "out_idx", B)
    out_logq = _out(out_logq, torch.float64, dev, "out_logq", B)
    out_logm = _out(out_logm, torch.float64, dev, "out_logm", 1)
    status = _out(status, torch.int32, dev, "status", 1)
    ws = _mps_query_ws(h, dev, n, D, 1)
    h.call("bornvi_mps_sample_clamped", n, D, B, _ptr(cores), _ptr(mask), _ptr(value), seed, _ptr(epoch),
           _ptr(out_idx), _ptr(out_logq), _ptr(out_logm), _ptr(status), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out_idx, out_logq, out_logm, status


def mps_marginals(cores, want_pairs=False, out_m1=None, out_m2=None):
    """Exact marginals of an MPS Born machine (bornvi_mps_marginals): -> (m1 float64 [n], m1[i] = q(z_i = 1), m2 float64
    [n, n] or None, m2[i, j] = q(z_i = 1, z_j = 1): symmetric bit for bit, its diagonal m1).  Runs its own environment
    sweeps in its own workspace: no mps_environments is needed and none is disturbed."""
    n, D, _ = _mps_args(cores, 1)
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    out_m1 = _out(out_m1, torch.float64, dev, "out_m1", n)
    if want_pairs:
        out_m2 = _out(out_m2, torch.float64, dev, "out_m2", n * n).view(n, n)
    elif out_m2 is not None:
        raise BornviError("out_m2 given without want_pairs")
    ws = _mps_query_ws(h, dev, n, D, 1)
    h.call("bornvi_mps_marginals", n, D, _ptr(cores), _ptr(out_m1), _ptr(out_m2) if want_pairs else None, _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return out_m1, out_m2


# ---- canonical form, bond spectra and truncation (kernels_mps_canon.hip) -----------------------
def mps_canonicalise(cores, bond_dim_out=None, cutoff=0.0):
    """Canonical form of an MPS Born machine (bornvi_mps_canonicalise): cores float64 [n, 2, D, D] on the GPU, 1 <= n <= 63 ->
    (cores_out float64 [n, 2, D_out, D_out]: psi_out = psi / sqrt(Z) up to what is cut, sites 2 .. n right-canonical;
    schmidt float64 [n - 1, D]: the Schmidt values of every bond, descending, sum of squares 1; discarded float64 [n - 1]:
    the sum of the dropped squares; rank int32 [n - 1]: the values kept; log_norm float64 [1] = log Z of the input; status
    int32 [1]: 0, 1 (non-finite input or Z: cores_out NaN) or 4 (a factorisation did not converge)).  bond_dim_out (default
    D): the D_out largest values of a bond stay; then more go from the small end while the dropped squares sum to <= cutoff."""
    n, D, _ = _mps_args(cores, 1)
    Do = D if bond_dim_out is None else bond_dim_out
    if isinstance(Do, bool) or not isinstance(Do, (int, np.integer)) or not 1 <= int(Do) <= D:
        raise BornviError(f"bond_dim_out must be an integer in 1 ... {D} (the cores' bond dimension), got {bond_dim_out!r}")
    Do = int(Do)
    _chk_positive(cutoff, "cutoff", allow_zero=True)
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    out = torch.empty(n, 2, Do, Do, dtype=torch.float64, device=dev)
    schmidt = torch.empty(n - 1, D, dtype=torch.float64, device=dev)
    discarded = torch.empty(n - 1, dtype=torch.float64, device=dev)
    rank = torch.empty(n - 1, dtype=torch.int32, device=dev)
    log_norm = torch.empty(1, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _ws(dev, _cached_size(h, "bornvi_mps_canon_workspace_bytes", n, D), f"mps_canon_{n}_{D}")
    h.call("bornvi_mps_canonicalise", n, D, Do, float(cutoff), _ptr(cores), _ptr(out), _ptr(schmidt) if n > 1 else None,
           _ptr(discarded) if n > 1 else None, _ptr(rank) if n > 1 else None, _ptr(log_norm), _ptr(status), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return out, schmidt, discarded, rank, log_norm, status


# ---- two-site sweeps of the sampled MPS (kernels_mps_twosite.hip, include/bornvi_twosite.h) --------
MPS_TWOSITE_MAX_BOND = _ext.TWOSITE_LIMITS["BORNVI_MPS_TWOSITE_MAX_BOND"]
MPS_TWOSITE_MAX_BATCH = _ext.TWOSITE_LIMITS["BORNVI_MPS_TWOSITE_MAX_BATCH"]
MPS_TWOSITE_MAX_STEPS = _ext.TWOSITE_LIMITS["BORNVI_MPS_TWOSITE_MAX_STEPS"]


def mps_twosite_args(cores, idx, w, lr, steps, bond_dim_keep, cutoff):
    """(n, D, B, D_keep) of a two-site sweep's arguments; every argument error is raised here, before any GPU call."""
    if not torch.is_tensor(idx) or idx.dim() != 1:
        raise BornviError("idx: expected a [B] int64 tensor")
    n, D, _ = _mps_args(cores, 1)
    if n < 2:
        raise BornviError("a two-site sweep needs at least two sites (n >= 2)")
    if D > MPS_TWOSITE_MAX_BOND:
        raise BornviError(f"two-site sweeps: bond dimension 1 ... {MPS_TWOSITE_MAX_BOND}, got {D}")
    B = int(idx.numel())
    if not 1 <= B <= MPS_TWOSITE_MAX_BATCH:
        raise BornviError(f"number of samples: 1 ... 2^20 per two-site sweep, got {B}")
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= int(steps) <= MPS_TWOSITE_MAX_STEPS:
        raise BornviError(f"steps must be an integer in 1 ... {MPS_TWOSITE_MAX_STEPS}, got {steps!r}")
    Dk = D if bond_dim_keep is None else bond_dim_keep
    if isinstance(Dk, bool) or not isinstance(Dk, (int, np.integer)) or not 1 <= int(Dk) <= D:
        raise BornviError(f"bond_dim_keep must be an integer in 1 ... {D} (the cores' bond dimension), got {bond_dim_keep!r}")
    _chk_positive(lr, "lr", allow_zero=True)
    _chk_positive(cutoff, "cutoff", allow_zero=True)
    if not cutoff < 1:
        raise BornviError(f"cutoff must be < 1, got {cutoff!r}")
    dev = cores.device
    _chk(cores, torch.float64, dev, "cores")
    _chk(idx, torch.int64, dev, "idx", B)
    if w is not None:
        if not torch.is_tensor(w):
            raise BornviError("w: expected None or a [B] float64 tensor")
        _chk(w, torch.float64, dev, "w", B)
    return n, D, B, int(Dk)


def mps_twosite_sweep(cores, idx, w=None, lr=0.05, steps=5, bond_dim_keep=None, cutoff=0.0):
    """One round trip of two-site updates over the bonds of a sampled MPS (bornvi_mps_twosite_sweep): cores float64
    [n, 2, D, D] on the GPU in canonical form (what mps_canonicalise returns; 2 <= n <= 63, D <= 16), REPLACED IN PLACE;
    idx int64 [B] samples, w float64 [B] weights or None for 1 / B each -> (loss float64 [2 (n - 1)]: the merged tensor's
    loss after the last descent step of every bond visited; schmidt float64 [n - 1, D]: the kept values of every bond over
    their norm, descending, then 0.0; discarded float64 [n - 1]; rank int32 [n - 1]; status int32 [1]: a sum of 1 (non-finite
    cores or norm: outputs NaN), 2 (some psi of a sample was 0 or not finite: left out at that bond), 4 (a factorisation did
    not converge), 8 (the cores were not canonical on entry)).  bond_dim_keep (default D) and cutoff cut every bond as
    mps_canonicalise does."""
    n, D, B, Dk = mps_twosite_args(cores, idx, w, lr, steps, bond_dim_keep, cutoff)
    dev = cores.device
    h = _ext.handle_for(dev)
    loss = torch.empty(2 * (n - 1), dtype=torch.float64, device=dev)
    schmidt = torch.empty(n - 1, D, dtype=torch.float64, device=dev)
    discarded = torch.empty(n - 1, dtype=torch.float64, device=dev)
    rank = torch.empty(n - 1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _ws(dev, _cached_size(h, "bornvi_mps_twosite_workspace_bytes", n, D, B), f"mps_twosite_{n}_{D}_{B}")
    h.call("bornvi_mps_twosite_sweep", n, D, B, _ptr(cores), _ptr(idx), _ptr(w) if w is not None else None, float(lr), int(steps),
           Dk, float(cutoff), _ptr(loss), _ptr(schmidt), _ptr(discarded), _ptr(rank), _ptr(status), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return loss, schmidt, discarded, rank, status


def bn_descriptor(packed, dev):
    """(device arrays, BnDesc) of bayesian_network.pack_network's dict; the arrays must outlive every call that uses the
    descriptor.  A network with a summed-out node is refused by bn_logjoint_samples, not here."""
    t = {k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in packed.items()}
    desc = _ext.BnDesc(int(t["role"].numel()), int(t["parents"].shape[1]), t["role"].data_ptr(),
                       t["n_parents"].data_ptr(), t["parents"].data_ptr(), t["cpt_off"].data_ptr(), t["cpt"].data_ptr())
    return t, desc


def bn_logjoint_samples(desc, n, idx, p_floor=1e-30, out=None):
    """Log joint of sampled latent states (bornvi_bn_logjoint_samples): desc from bn_descriptor, idx int64 [B] on the GPU
    -> logp float64 [B], logp_b = sum over the nodes of log max(CPT factor, p_floor).  Every factor is floored, where
    ElboObjective floors the product; the two agree whenever no factor is below p_floor and the product is >= p_floor."""
    _chk_n(n, 1, MPS_SAMPLED_MAX_N)
    _chk_positive(p_floor, "p_floor")
    if not torch.is_tensor(idx) or idx.dim() != 1 or not 1 <= int(idx.numel()) <= MPS_SAMPLED_MAX_BATCH:
        raise BornviError("idx: expected a [B] int64 tensor, 1 <= B <= 2^24")
    dev = idx.device
    h = _ext.handle_for(dev)
    B = int(idx.numel())
    _chk(idx, torch.int64, dev, "idx")
    out = _out(out, torch.float64, dev, "out", B)
    h.call("bornvi_bn_logjoint_samples", C.byref(desc), int(n), B, _ptr(idx), float(p_floor), _ptr(out), _ext.stream_ptr(dev))
    return out


# ---- amortised inference: draws from the network, gradient of log-marginals -------------------
def bn_sample(desc, n, num_samples, seed, epoch, out_idx=None, out_logp=None, status=None):
    """Exact ancestral draws from the network (bornvi_bn_sample): desc from bn_descriptor of
    bayesian_network.pack_network_for_sampling's dict, epoch an int64 device tensor [1] -> (idx int64 [B]: the kept nodes'
    bits, tuple position p at bit n - 1 - p, logp float64 [B] = log p of the whole draw, dropped nodes included, status
    int32 [1]: 0, or 1 when a sample met a CPT row whose sum is not positive and finite).  A draw is a pure function of
    (network, seed, epoch, b)."""
    _chk_n(n, 1, MPS_SAMPLED_MAX_N)
    B = _sample_count(num_samples)
    seed = _seed_word(seed)
    if not torch.is_tensor(epoch):
        raise BornviError("epoch: expected an int64 device tensor [1]")
    dev = epoch.device
    h = _ext.handle_for(dev)
    _chk(epoch, torch.int64, dev, "epoch", 1)
    out_idx = _out(out_idx, torch.int64, dev, "out_idx", B)
    out_logp = _out(out_logp, torch.float64, dev, "out_logp", B)
    status = _out(status, torch.int32, dev, "status", 1)
    h.call("bornvi_bn_sample", C.byref(desc), int(n), B, seed, _ptr(epoch), _ptr(out_idx), _ptr(out_logp),
           _ptr(status), _ext.stream_ptr(dev))
    return out_idx, out_logp, status


def mps_log_marginals_vjp_groups(Q):
    """The workgroups that take queries in mps_log_marginals_vjp = the partials per gradient entry: a function of Q only."""
    G = C.c_int(0)
    if _ext.lib().bornvi_mps_log_marginals_vjp_geometry(int(Q), C.byref(G)) != 0:
        raise BornviError(f"number of queries: 1 ... 2^16 per call, got {Q}")
    return int(G.value)


def mps_log_marginals_vjp(cores, mask, value, c, out=None, out_logm=None, status=None):
    """Gradient of weighted log-marginals of an MPS Born machine (bornvi_mps_log_marginals_vjp): mask, value int64 [Q] as
    for mps_log_marginals, c float64 [Q] -> (grad float64 [n, 2, D, D] = sum_j c_j grad log q(evidence_j), logm float64
    [Q]: mps_log_marginals' bits, status int32 [1]: 0, or 1 when some evidence is impossible or met a non-finite
    environment; such an evidence contributes nothing).  Needs no mps_environments."""
    n, D, _ = _mps_args(cores, 1)
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    Q = _evidence_args(mask, value, dev)
    _chk(c, torch.float64, dev, "c", Q)
    out = _out(out, torch.float64, dev, "out", tuple(cores.shape))
    out_logm = _out(out_logm, torch.float64, dev, "out_logm", Q)
    status = _out(status, torch.int32, dev, "status", 1)
    ws = _ws(dev, _cached_size(h, "bornvi_mps_log_marginals_vjp_workspace_bytes", n, D, Q), f"mps_logm_vjp_{n}_{D}_{Q}")
    h.call("bornvi_mps_log_marginals_vjp", n, D, Q, _ptr(cores), _ptr(mask), _ptr(value), _ptr(c), _ptr(out), _ptr(out_logm),
           _ptr(status), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out, out_logm, status


# ---- sampled KSD: scores of p at sampled states, pairwise Stein kernel row sums -----------------------------
STEIN_PAIRS_MAX_BATCH = _ext.LIMITS["BORNVI_STEIN_PAIRS_MAX_B"]


def bn_score_samples(desc, n, idx, p_floor=1e-30, out=None, want_logp=False):
    """Stein score of p at sampled latent states (bornvi_bn_score_samples): desc from bn_descriptor, idx int64 [B] on the
    GPU -> S float64 [B, n], S[b, i] = 1 - prod_v max(f_v(flip_i z_b), p_floor) / max(f_v(z_b), p_floor) over node i's own
    factor and its children's; with want_logp (S, logp [B]), logp bit-equal to bn_logjoint_samples.  Every factor is
    floored; there is no zero row where p(x, z) < 1e-12 (score_from_packed has that rule; at n = 60 every joint is below it)."""
    _chk_n(n, 1, MPS_SAMPLED_MAX_N)
    _chk_positive(p_floor, "p_floor")
    if not torch.is_tensor(idx) or idx.dim() != 1 or not 1 <= int(idx.numel()) <= MPS_SAMPLED_MAX_BATCH:
        raise BornviError("idx: expected a [B] int64 tensor, 1 <= B <= 2^24")
    dev = idx.device
    h = _ext.handle_for(dev)
    B = int(idx.numel())
    _chk(idx, torch.int64, dev, "idx")
    out = _out(out, torch.float64, dev, "out", (B, int(n)))
    logp = torch.empty(B, dtype=torch.float64, device=dev) if want_logp else None
    h.call("bornvi_bn_score_samples", C.byref(desc), int(n), B, _ptr(idx), float(p_floor), _ptr(out),
           _ptr(logp) if logp is not None else None, _ext.stream_ptr(dev))
    return (out, logp) if want_logp else out


def stein_pairs_geometry(B):
    """(32-column tiles per column range, number of column ranges G) of stein_pairs_rowsum for B samples: a function of B
    only; a row sum is G partials added in order, each a chain over its range's tiles (host only, no GPU needed)."""
    per, G = C.c_int(0), C.c_int(0)
    if _ext.lib().bornvi_stein_pairs_geometry(int(B), C.byref(per), C.byref(G)) != 0:
        raise BornviError(f"stein_pairs_geometry: 2 <= B <= 2^17, got {B!r}")
    return per.value, G.value


def stein_pairs_rowsum(idx, S, n, length_scale=1.0, out=None, total=None):
    """Row sums of the pairwise Stein kernel of B samples (bornvi_stein_pairs_rowsum): idx int64 [B], S float64 [B, n] the
    samples' score rows -> (r float64 [B], r_b = sum over b' != b BY SAMPLE INDEX of k_p(z_b, z_b'), total float64 [1] =
    sum_b r_b).  2 <= B <= 2^17, n * length_scale >= 1.  The workspace is cached per (n, B)."""
    _chk_n(n, 1, MPS_SAMPLED_MAX_N)
    _chk_positive(length_scale, "length_scale")
    if not float(int(n)) * float(length_scale) >= 1.0:
        raise BornviError(f"stein_pairs_rowsum: n * length_scale >= 1 is required (the Gram form loses accuracy below it), "
                          f"got {int(n)} * {length_scale!r}")
    if not torch.is_tensor(idx) or idx.dim() != 1 or not 2 <= int(idx.numel()) <= STEIN_PAIRS_MAX_BATCH:
        raise BornviError("idx: expected a [B] int64 tensor, 2 <= B <= 2^17")
    dev = idx.device
    h = _ext.handle_for(dev)
    n, B = int(n), int(idx.numel())
    _chk(idx, torch.int64, dev, "idx")
    _chk(S, torch.float64, dev, "S", B * n)
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", B)
    if total is None:
        total = torch.empty(1, dtype=torch.float64, device=dev)
    else:
        _chk(total, torch.float64, dev, "total", 1)
    ws = _ws(dev, _cached_size(h, "bornvi_stein_pairs_workspace_bytes", n, B), f"stein_pairs_{n}_{B}")
    h.call("bornvi_stein_pairs_rowsum", n, B, float(length_scale), _ptr(idx), _ptr(S), _ptr(out), _ptr(total), _ptr(ws),
           ws.numel(), _ext.stream_ptr(dev))
    return out, total


# ---- natural gradient ---------------------------------------------------------------------------------
FISHER_MAX_PARAMS = _ext.LIMITS["BORNVI_FISHER_MAX_PARAMS"]


def _chk_positive(v, name, allow_zero=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) \
            or not (v >= 0 if allow_zero else v > 0):
        raise BornviError(f"{name} must be a finite number {'>= 0' if allow_zero else '> 0'}, got {v!r}")


def fisher_gram(shifted, q, q_floor=1e-10, out=None):
    """Classical Fisher matrix of a Born distribution from stored parameter-shift rows (bornvi_fisher_gram): shifted
    float64 [2 P, 2^n] on the GPU, rows (+p, -p) as paramshift_probs lays them out; q float64 [2^n] -> F float64 [P, P],
    F_ab = sum_z d_a d_b / q_z over the states with q_z >= q_floor, d_a = 1/2 (row_2a - row_2a+1).  F == F.T bitwise; two
    calls are bitwise equal; capturable once the stream's workspace exists."""
    if not torch.is_tensor(shifted) or not torch.is_tensor(q) or shifted.dim() != 2 or q.dim() != 1:
        raise BornviError("fisher_gram: shifted must be a [2 P, 2^n] tensor and q a [2^n] tensor")
    N = int(q.numel())
    if N < 2 or N & (N - 1):
        raise BornviError(f"q: {N} entries is not 2^n with n >= 1")
    n = N.bit_length() - 1
    _chk_n(n)
    if shifted.shape[1] != N or shifted.shape[0] % 2:
        raise BornviError(f"shifted: shape {tuple(shifted.shape)} is not [2 P, {N}]")
    P = int(shifted.shape[0]) // 2
    if not 1 <= P <= FISHER_MAX_PARAMS:
        raise BornviError(f"shifted: 1 ... {FISHER_MAX_PARAMS} parameters per call, got {P}")
    _chk_positive(q_floor, "q_floor")
    dev = q.device
    h = _ext.handle_for(dev)
    _chk(shifted, torch.float64, dev, "shifted")
    _chk(q, torch.float64, dev, "q")
    if out is None:
        out = torch.empty((P, P), dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", P * P)
    ws = _ws(dev, _cached_size(h, "bornvi_fisher_workspace_bytes", n, P), "fisher")
    h.call("bornvi_fisher_gram", n, _ptr(shifted), P, _ptr(q), float(q_floor), _ptr(out), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return out


def spd_solve(A, b, damping=0.0, out=None, info=None):
    """(A + damping I) x = b by Cholesky on the device (bornvi_spd_solve): A float64 [P, P] symmetric (its upper triangle
    is read, A is left untouched), b float64 [P] -> (x float64 [P], info int32 [1]).  info is 0 on success, k + 1 when
    pivot k is non-positive or non-finite, P + 1 when b is not finite, P + 2 when the solution is not finite; in those
    cases x = b.  Bitwise reproducible; capturable once the stream's workspace exists."""
    if not torch.is_tensor(A) or not torch.is_tensor(b) or A.dim() != 2 or A.shape[0] != A.shape[1] or b.dim() != 1:
        raise BornviError("spd_solve: A must be a [P, P] tensor and b a [P] tensor")
    P = int(A.shape[0])
    if not 1 <= P <= FISHER_MAX_PARAMS:
        raise BornviError(f"A: 1 ... {FISHER_MAX_PARAMS} rows, got {P}")
    _chk_positive(damping, "damping", allow_zero=True)
    dev = A.device
    h = _ext.handle_for(dev)
    _chk(A, torch.float64, dev, "A")
    _chk(b, torch.float64, dev, "b", P)
    if out is None:
        out = torch.empty(P, dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", P)
    if info is None:
        info = torch.empty(1, dtype=torch.int32, device=dev)
    else:
        _chk(info, torch.int32, dev, "info", 1)
    ws = _ws(dev, _cached_size(h, "bornvi_spd_solve_workspace_bytes", P), "spd_solve")
    h.call("bornvi_spd_solve", P, _ptr(A), float(damping), _ptr(b), _ptr(out), _ptr(info), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return out, info


def spd_solve_batched(A, b, damping=0.0, out=None, info=None):
    """nb independent systems (A[j] + damping I) x[j] = b[j] in one launch (bornvi_spd_solve_batched): A float64 [nb, P, P],
    b float64 [nb, P] -> (x float64 [nb, P], info int32 [nb]).  System j is bit for bit what spd_solve gives on (A[j], b[j]),
    with its info codes and its rule x[j] = b[j] where info[j] != 0.  Capturable once the stream's workspace exists."""
    if not torch.is_tensor(A) or not torch.is_tensor(b) or A.dim() != 3 or A.shape[1] != A.shape[2] or b.dim() != 2 \
            or b.shape[0] != A.shape[0]:
        raise BornviError("spd_solve_batched: A must be a [nb, P, P] tensor and b a [nb, P] tensor")
    nb, P = int(A.shape[0]), int(A.shape[1])
    if not 1 <= P <= FISHER_MAX_PARAMS:
        raise BornviError(f"A: 1 ... {FISHER_MAX_PARAMS} rows per system, got {P}")
    if not 1 <= nb <= 65535:
        raise BornviError(f"A: 1 ... 65535 systems, got {nb}")
    _chk_positive(damping, "damping", allow_zero=True)
    dev = A.device
    h = _ext.handle_for(dev)
    _chk(A, torch.float64, dev, "A")
    _chk(b, torch.float64, dev, "b", nb * P)
    if out is None:
        out = torch.empty((nb, P), dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", nb * P)
    if info is None:
        info = torch.empty(nb, dtype=torch.int32, device=dev)
    else:
        _chk(info, torch.int32, dev, "info", nb)
    ws = _ws(dev, _cached_size(h, "bornvi_spd_solve_batched_workspace_bytes", P, nb), "spd_solve_batched")
    h.call("bornvi_spd_solve_batched", P, nb, _ptr(A), float(damping), _ptr(b), _ptr(out), _ptr(info), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return out, info


# ---- natural gradient of the sampled MPS Born machine ---------------------------------------------------
SCORE_ROWS_MIN_BATCH = 2


def score_rows_ld(num_samples):
    """Leading dimension of the score rows of B samples: the power of two >= max(B, 64) (what score_fisher_gram takes)."""
    return max(64, 1 << (int(num_samples) - 1).bit_length())


def mps_score_rows(cores, idx, k_begin=0, k_count=None, out=None, status=None):
    """Per-sample score rows of an MPS Born machine (bornvi_mps_score_rows), after mps_environments(cores, len(idx)):
    -> (rows float64 [k_count, 2 D^2, ld], status int32 [1]) for the sites k_begin .. k_begin + k_count - 1 (from 0),
    rows[j, (s D + a) D + c, b] = d log q(idx_b) / d cores[k_begin + j, s, a, c] in centred form (2 [z = s] l r / psi - mu with
    mu its exact mean under q), ld = score_rows_ld(B), the columns B .. ld - 1 exactly 0.0.  status: 0, or 2 when some
    psi(idx_b) is 0 or not finite (that sample's column is all 0.0).  B >= 2."""
    if not torch.is_tensor(idx) or idx.dim() != 1:
        raise BornviError("idx: expected a [B] int64 tensor")
    n, D, B = _mps_args(cores, int(idx.numel()))
    if B < SCORE_ROWS_MIN_BATCH:
        raise BornviError(f"mps_score_rows: at least {SCORE_ROWS_MIN_BATCH} samples, got {B}")
    if k_count is None:
        k_count = n - int(k_begin)
    if isinstance(k_begin, bool) or isinstance(k_count, bool) or not isinstance(k_begin, (int, np.integer)) \
            or not isinstance(k_count, (int, np.integer)) or k_begin < 0 or k_count < 1 or k_begin + k_count > n:
        raise BornviError(f"mps_score_rows: sites {k_begin!r} .. + {k_count!r} are not a range of the {n} sites")
    k_begin, k_count = int(k_begin), int(k_count)
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    _chk(idx, torch.int64, dev, "idx", B)
    ld, R = score_rows_ld(B), 2 * D * D
    out = _out(out, torch.float64, dev, "out", (k_count, R, ld))
    status = _out(status, torch.int32, dev, "status", 1)
    ws = _mps_sampled_ws(h, dev, n, D, B)
    h.call("bornvi_mps_score_rows", n, D, B, _ptr(cores), _ptr(idx), k_begin, k_count, ld, _ptr(out), _ptr(status), _ptr(ws),
           ws.numel(), _ext.stream_ptr(dev))
    return out, status


def score_fisher_workspace_bytes(dev, R, nblocks, ld):
    return _cached_size(_ext.handle_for(dev), "bornvi_score_fisher_workspace_bytes", int(R), int(nblocks), int(ld))


def score_fisher_gram(rows, num_samples, out=None):
    """Sampled Fisher estimate from score rows (bornvi_score_fisher_gram): rows float64 [nblocks, R, ld] (ld a power of two
    >= 64, the columns num_samples .. ld - 1 zero) -> F float64 [nblocks, R, R], F[j] = rows[j] rows[j]^T / num_samples on the
    fp64 matrix cores.  F[j] == F[j].T bitwise; two calls are bitwise equal; an entry's order of summation depends on ld
    only.  1 <= R <= 1024.  Capturable once the stream's workspace exists."""
    if not torch.is_tensor(rows) or rows.dim() != 3:
        raise BornviError("score_fisher_gram: rows must be an [nblocks, R, ld] tensor")
    nblocks, R, ld = (int(v) for v in rows.shape)
    B = num_samples
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not SCORE_ROWS_MIN_BATCH <= int(B) <= ld:
        raise BornviError(f"number of samples: {SCORE_ROWS_MIN_BATCH} ... ld = {ld}, got {B!r}")
    if not 1 <= R <= FISHER_MAX_PARAMS:
        raise BornviError(f"rows: 1 ... {FISHER_MAX_PARAMS} rows per block, got {R}")
    if not 1 <= nblocks <= 65535:
        raise BornviError(f"rows: 1 ... 65535 blocks, got {nblocks}")
    if ld < 64 or ld & (ld - 1) or ld > MPS_SAMPLED_MAX_BATCH:
        raise BornviError(f"rows: the leading dimension must be a power of two in 64 ... 2^24, got {ld}")
    dev = rows.device
    h = _ext.handle_for(dev)
    _chk(rows, torch.float64, dev, "rows")
    if out is None:
        out = torch.empty((nblocks, R, R), dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", nblocks * R * R)
    ws = _ws(dev, _cached_size(h, "bornvi_score_fisher_workspace_bytes", R, nblocks, ld), "score_fisher")
    h.call("bornvi_score_fisher_gram", R, nblocks, int(B), ld, _ptr(rows), _ptr(out), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out


SAMPLE_GRAM_MAX_BATCH = _ext.LIMITS["BORNVI_SAMPLE_GRAM_MAX_BATCH"]           # T is [B, B] and spd_solve factors it


def mps_score_sample_gram_workspace_bytes(dev, n, D, num_samples):
    return _cached_size(_ext.handle_for(dev), "bornvi_mps_score_sample_gram_workspace_bytes", int(n), int(D), int(num_samples))


def mps_score_sample_gram(cores, idx, out=None, status=None):
    """Sample-space Gram of the score rows of an MPS Born machine (bornvi_mps_score_sample_gram), after
    mps_environments(cores, len(idx)): -> (T float64 [B, B], status int32 [1]), T[b, b'] = o_b . o_b' / B with o_b the
    centred score row of sample b (the column b of mps_score_rows), computed from the samples' left and right vectors on
    the fp64 matrix cores without forming a row.  T == T.T bitwise; two calls are bitwise equal.  status: 0, or 2 when some
    psi(idx_b) is 0 or not finite (that sample's row and column are all 0.0).  2 <= B <= 1024."""
    if not torch.is_tensor(idx) or idx.dim() != 1:
        raise BornviError("idx: expected a [B] int64 tensor")
    n, D, B = _mps_args(cores, int(idx.numel()))
    if not SCORE_ROWS_MIN_BATCH <= B <= SAMPLE_GRAM_MAX_BATCH:
        raise BornviError(f"mps_score_sample_gram: {SCORE_ROWS_MIN_BATCH} ... {SAMPLE_GRAM_MAX_BATCH} samples, got {B}")
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    _chk(idx, torch.int64, dev, "idx", B)
    out = _out(out, torch.float64, dev, "out", (B, B))
    status = _out(status, torch.int32, dev, "status", 1)
    env = _mps_sampled_ws(h, dev, n, D, B)
    ws = _ws(dev, _cached_size(h, "bornvi_mps_score_sample_gram_workspace_bytes", n, D, B), f"mps_sample_gram_{n}_{D}_{B}")
    h.call("bornvi_mps_score_sample_gram", n, D, B, _ptr(cores), _ptr(idx), _ptr(out), _ptr(status), _ptr(env), env.numel(),
           _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out, status


# ---- matrix-free natural gradient of the sampled MPS Born machine: O v, and conjugate gradients around a product ----
CG_MAX_PARAMS = _ext.LIMITS["BORNVI_CG_MAX_PARAMS"]
CG_STATE_DOUBLES = _ext.LIMITS["BORNVI_CG_STATE_DOUBLES"]


def mps_score_jvp(cores, idx, v, scale=1.0, out=None, status=None):
    """Per-sample directional derivative of log q of an MPS Born machine (bornvi_mps_score_jvp), after
    mps_environments(cores, len(idx)): v float64 [n, 2, D, D] -> (t float64 [B], status int32 [1]),
    t_b = scale <grad log q(idx_b), v>: the product O v of the centred score rows (mps_score_rows) with v, without forming a
    row; mps_score_vjp is its transpose.  t_b's bits depend on (cores, v, scale, idx_b) only; two calls are bitwise equal.
    status: 0, or 2 when some psi(idx_b) is 0 or not finite (that t_b is 0.0).  B >= 2."""
    if not torch.is_tensor(idx) or idx.dim() != 1:
        raise BornviError("idx: expected a [B] int64 tensor")
    n, D, B = _mps_args(cores, int(idx.numel()))
    if B < SCORE_ROWS_MIN_BATCH:
        raise BornviError(f"mps_score_jvp: at least {SCORE_ROWS_MIN_BATCH} samples, got {B}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not np.isfinite(scale):
        raise BornviError(f"scale must be a finite number, got {scale!r}")
    if not torch.is_tensor(v) or tuple(v.shape) != tuple(cores.shape):
        raise BornviError(f"v: expected a tensor of the cores' shape {tuple(cores.shape)}, got "
                          f"{tuple(v.shape) if torch.is_tensor(v) else type(v)}")
    dev = cores.device
    h = _ext.handle_for(dev)
    _chk(cores, torch.float64, dev, "cores")
    _chk(idx, torch.int64, dev, "idx", B)
    _chk(v, torch.float64, dev, "v", cores.numel())
    out = _out(out, torch.float64, dev, "out", B)
    status = _out(status, torch.int32, dev, "status", 1)
    env = _mps_sampled_ws(h, dev, n, D, B)
    h.call("bornvi_mps_score_jvp", n, D, B, _ptr(cores), _ptr(idx), _ptr(v), float(scale), _ptr(out), _ptr(status), _ptr(env),
           env.numel(), _ext.stream_ptr(dev))
    return out, status


def _cg_vectors(g, named):
    """P and the device of g float64 [P] (any shape, contiguous); every (name, tensor) of `named` must match it."""
    if not torch.is_tensor(g) or g.numel() < 1:
        raise BornviError("cg: g must be a tensor with at least one element")
    P, dev = int(g.numel()), g.device
    if P > CG_MAX_PARAMS:
        raise BornviError(f"cg: 1 ... 2^31 - 1 elements, got {P}")
    _chk(g, torch.float64, dev, "g")
    for name, t in named:
        if not torch.is_tensor(t):
            raise BornviError(f"cg: {name} must be a tensor")
        _chk(t, torch.float64, dev, name, P)
    return P, dev


def cg_init(g, x=None, r=None, p=None, state=None, info=None):
    """Start of conjugate gradients on (F + damping I) x = g (bornvi_cg_init): g float64 [P] (any shape) ->
    (x = 0, r = g, p = g, state float64 [8], info int32 [1]).  state: rr = r^T r, rr0 = g^T g, iterations, done flag, relres,
    fallback flag.  g = 0 sets done; a non-finite g sets done and fallback (info = 1).  x, r, p, state, info: destinations."""
    if torch.is_tensor(g):
        x, r, p = (torch.empty_like(g) if t is None else t for t in (x, r, p))
    P, dev = _cg_vectors(g, (("x", x), ("r", r), ("p", p)))
    if state is None:
        state = torch.empty(CG_STATE_DOUBLES, dtype=torch.float64, device=dev)
    else:
        _chk(state, torch.float64, dev, "state", CG_STATE_DOUBLES)
    if info is None:
        info = torch.empty(1, dtype=torch.int32, device=dev)
    else:
        _chk(info, torch.int32, dev, "info", 1)
    _ext.handle_for(dev).call("bornvi_cg_init", P, _ptr(g), _ptr(x), _ptr(r), _ptr(p), _ptr(state), _ptr(info), _ext.stream_ptr(dev))
    return x, r, p, state, info


def cg_step(Fp, x, r, p, state, damping, rel_tol=0.0):
    """One conjugate-gradient iteration in place (bornvi_cg_step), Fp = F p without the damping: q = Fp + damping p,
    alpha = rr / p^T q, x += alpha p, r -= alpha q, p = r + (rr' / rr) p; done once rr' <= rel_tol^2 rr0.  Writes nothing once
    the done flag of `state` is set; freezes (and, at iteration 0, asks for the fallback) where p^T q is not positive and
    finite.  Returns state."""
    P, dev = _cg_vectors(Fp, (("x", x), ("r", r), ("p", p)))
    _chk_positive(damping, "damping")
    _chk_positive(rel_tol, "rel_tol", allow_zero=True)
    if not torch.is_tensor(state):
        raise BornviError("cg: state must be a tensor")
    _chk(state, torch.float64, dev, "state", CG_STATE_DOUBLES)
    _ext.handle_for(dev).call("bornvi_cg_step", P, float(damping), float(rel_tol), _ptr(Fp), _ptr(x), _ptr(r), _ptr(p), _ptr(state),
                              _ext.stream_ptr(dev))
    return state


def cg_finish(g, x, state, info=None, iters=None, relres=None):
    """End of a conjugate-gradient solve (bornvi_cg_finish) -> (x, info int32 [1], iters int32 [1], relres float64 [1]):
    x = g bit for bit and info = 1 where the fallback flag of `state` is set or x is not finite, else info = 0 (converged
    or not: relres = sqrt(rr / rr0) says).  info, iters, relres: destinations."""
    P, dev = _cg_vectors(g, (("x", x),))
    if not torch.is_tensor(state):
        raise BornviError("cg: state must be a tensor")
    _chk(state, torch.float64, dev, "state", CG_STATE_DOUBLES)
    if info is None:
        info = torch.empty(1, dtype=torch.int32, device=dev)
    else:
        _chk(info, torch.int32, dev, "info", 1)
    if iters is None:
        iters = torch.empty(1, dtype=torch.int32, device=dev)
    else:
        _chk(iters, torch.int32, dev, "iters", 1)
    if relres is None:
        relres = torch.empty(1, dtype=torch.float64, device=dev)
    else:
        _chk(relres, torch.float64, dev, "relres", 1)
    _ext.handle_for(dev).call("bornvi_cg_finish", P, _ptr(g), _ptr(x), _ptr(state), _ptr(info), _ptr(iters), _ptr(relres),
                              _ext.stream_ptr(dev))
    return x, info, iters, relres


def paramshift_states_bytes(n, count, include_base=True):
    """Bytes of the rows paramshift_states writes: 16 (count + base) 2^n."""
    return 16 * (int(count) + (1 if include_base else 0)) << int(n)


def paramshift_states(ansatz_type, n, layers, theta, p_begin, p_end, include_base=True, out=None):
    """theta float64 [P] -> states complex128 [(1 if include_base) + (p_end - p_begin), 2^n]: optional base row
    U(theta)|0..0>, then U(theta + pi e_p)|0..0> for p in [p_begin, p_end), phase-coherent and in canonical order
    (bornvi_paramshift_states; a row equals adjoint_state at the same parameters to rounding).  The circuits run in
    chunks when their workspace would exceed WORKSPACE_CAP.  Capturable after one eager call."""
    _chk_n(n, 1, CIRCUIT_MAX_N)
    dev = theta.device
    h = _ext.handle_for(dev)
    aid = ansatz_id(ansatz_type)
    P = num_params(ansatz_type, n, layers)
    _chk(theta, torch.float64, dev, "theta", P)
    if not 0 <= p_begin <= p_end <= P:
        raise BornviError(f"parameter range [{p_begin}, {p_end}) out of bounds (P = {P})")
    count = int(p_end) - int(p_begin)
    B = (1 if include_base else 0) + count
    if out is None:
        out = torch.empty((B, 1 << n), dtype=torch.complex128, device=dev)
    else:
        _chk(out, torch.complex128, dev, "out", B << n)
    if B == 0:
        return out
    need = _cached_size(h, "bornvi_paramshift_states_workspace_bytes", aid, n, layers, B)
    ws = _ws(dev, min(need, max(WORKSPACE_CAP, _cached_size(h, "bornvi_paramshift_states_workspace_bytes", aid, n, layers, 1))),
             "states")
    h.call("bornvi_paramshift_states", aid, n, layers, _ptr(theta), int(p_begin), count, 1 if include_base else 0, _ptr(out),
           _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out


def qfi_gram(phi, psi, out=None):
    """Quantum Fisher information matrix (bornvi_qfi_gram): phi complex128 [P, 2^n] (the pi-shifted states), psi
    complex128 [2^n] -> Q float64 [P, P], Q_ab = Re<phi_a|phi_b> - Re(conj(c_a) c_b), c_a = <psi|phi_a>: 4 x the
    Fubini-Study metric.  Q == Q.T bitwise; two calls are bitwise equal; capturable once the stream's workspace exists."""
    if not torch.is_tensor(phi) or not torch.is_tensor(psi) or phi.dim() != 2 or psi.dim() != 1:
        raise BornviError("qfi_gram: phi must be a [P, 2^n] tensor and psi a [2^n] tensor")
    N = int(psi.numel())
    if N < 2 or N & (N - 1):
        raise BornviError(f"psi: {N} entries is not 2^n with n >= 1")
    n = N.bit_length() - 1
    _chk_n(n)
    P = int(phi.shape[0])
    if phi.shape[1] != N:
        raise BornviError(f"phi: shape {tuple(phi.shape)} is not [P, {N}]")
    if not 1 <= P <= FISHER_MAX_PARAMS:
        raise BornviError(f"phi: 1 ... {FISHER_MAX_PARAMS} parameters per call, got {P}")
    dev = psi.device
    h = _ext.handle_for(dev)
    _chk(phi, torch.complex128, dev, "phi")
    _chk(psi, torch.complex128, dev, "psi")
    if out is None:
        out = torch.empty((P, P), dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", P * P)
    ws = _ws(dev, _cached_size(h, "bornvi_qfi_workspace_bytes", n, P), "qfi")
    h.call("bornvi_qfi_gram", n, P, _ptr(phi), _ptr(psi), _ptr(out), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out


# ---- finite shots -------------------------------------------------------------------------------------
SHOTS_MAX = _ext.LIMITS["BORNVI_SHOTS_MAX"]


def shots_histogram(probs, n, shots, seed, epoch, include_base=True, p_begin=0, p_stride=1, out=None):
    """Finite-shot measurement of B Born distributions (bornvi_shots_histogram): probs float64 [B, 2^n] on the GPU ->
    frequencies counts / shots [B, 2^n] of `shots` exact multinomial draws per row.  Row r is circuit id 0 (base) if
    include_base and r == 0, else 2p + 1 / 2p + 2 for the (+p, -p) rows of p = p_begin, p_begin + p_stride, ... -- the
    layout of paramshift_probs; the draws are a pure function of (seed, epoch, circuit id, draw index).  epoch: an int64
    device tensor [1] (read by the kernel: a captured graph sees its value at replay time).  out: destination [B, 2^n]
    (may be `probs` itself: in place); default a new tensor."""
    dev = probs.device
    h = _ext.handle_for(dev)
    _chk_n(n)
    if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)) or not (1 <= int(shots) <= SHOTS_MAX):
        raise BornviError(f"shots must be an integer in [1, 2^31 - 1], got {shots!r}")
    if probs.numel() % (1 << n):
        raise BornviError("probs: element count is not a multiple of 2^n")
    _chk(probs, torch.float64, dev, "probs")
    B = probs.numel() >> n
    _chk(epoch, torch.int64, dev, "epoch", 1)
    if out is None:
        out = torch.empty((B, 1 << n), dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", B << n)
        if out.data_ptr() != probs.data_ptr():
            a0, a1 = probs.data_ptr(), probs.data_ptr() + 8 * probs.numel()
            b0, b1 = out.data_ptr(), out.data_ptr() + 8 * out.numel()
            if a0 < b1 and b0 < a1:
                raise BornviError("shots_histogram: out overlaps probs without being the same buffer")
    if B == 0:
        return out
    ws = _ws(dev, _cached_size(h, "bornvi_shots_workspace_bytes", int(n), int(B)), "shots")
    h.call("bornvi_shots_histogram", int(n), int(B), _ptr(probs), _ptr(out), int(shots), int(seed) & ((1 << 64) - 1),
           _ptr(epoch), 1 if include_base else 0, int(p_begin), int(p_stride), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out


# ---- Stein ---------------------------------------------------------------------------------------
def score_from_packed(packed, n, dev):
    """packed: dict from bayesian_network.pack_network -> (S [2^n, n], pxz [2^n]) float64 on dev."""
    h = _ext.handle_for(dev)
    t = {k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in packed.items()}
    desc = _ext.BnDesc(int(t["role"].numel()), int(t["parents"].shape[1]), t["role"].data_ptr(),
                       t["n_parents"].data_ptr(), t["parents"].data_ptr(), t["cpt_off"].data_ptr(),
                       t["cpt"].data_ptr())
    S = torch.empty((1 << n, n), dtype=torch.float64, device=dev)
    pxz = torch.empty(1 << n, dtype=torch.float64, device=dev)
    h.call("bornvi_score_from_cpts", C.byref(desc), n, _ptr(S), _ptr(pxz), _ext.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()   # `t` (descriptor arrays) must outlive the kernel
    return S, pxz


def gram_ld(n):
    """Row pitch (doubles) the library recommends for a dense K_p that the symmetric contraction will stream:
    2^n + 32 for n >= 14 (a power-of-two pitch makes the row streams of a band collide on one HBM channel: n = 16
    2.56 ms padded against 2.62 ... 2.83 ms dense, by allocation), else 2^n."""
    return int(_ext.lib().bornvi_stein_gram_ld(int(n)))


def _chk_matrix(K, rows, N, dev, name):
    """K must be a float64 [rows, N] matrix on dev with unit column stride; returns its row pitch in doubles.  A padded
    matrix is the [:, :N] view of a [rows, ld] buffer (what stein_gram(ld=...) returns)."""
    if K.dtype != torch.float64 or K.device != dev or K.dim() != 2 or tuple(K.shape) != (int(rows), int(N)):
        raise BornviError(f"{name}: expected float64 [{int(rows)}, {int(N)}] on {dev}, got {K.dtype} {tuple(K.shape)} on {K.device}")
    if rows == 0:
        return int(N)
    ld = int(K.stride(0)) if rows > 1 else max(int(K.stride(0)), int(N))
    if K.stride(1) != 1 or ld < N or (ld & 1 and N > 1):
        raise BornviError(f"{name}: rows must be contiguous with an even pitch >= {int(N)} (strides {tuple(K.stride())})")
    return ld


def stein_gram(S, n, length_scale=1.0, rows=None, out=None, ld=None):
    """Dense K_p [2^n, 2^n], or only its rows [rows[0], rows[1]) (one rank's block of a row shard).
    ld: row pitch in doubles (default 2^n: a contiguous matrix; gram_ld(n) for the padded layout the symmetric
    contraction streams best) -- the result is then the [:, :2^n] view of a [rows, ld] buffer.
    out: a [rows, 2^n] float64 destination with unit column stride (e.g. rows of a larger, possibly padded, buffer)."""
    dev = S.device
    h = _ext.handle_for(dev)
    _chk_n(n, 1, 17)
    N = 1 << n
    _chk(S, torch.float64, dev, "S", n << n)
    r0, r1 = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
    if not (0 <= r0 <= r1 <= N):
        raise BornviError("stein_gram: row range out of bounds")
    if out is None:
        ld = N if ld is None else int(ld)
        if ld < N or ld & 1 and N > 1:
            raise BornviError("stein_gram: ld must be even and >= 2^n")
        K = torch.empty((r1 - r0, ld), dtype=torch.float64, device=dev)[:, :N]
    else:
        K = out
    pitch = _chk_matrix(K, r1 - r0, N, dev, "out" if out is not None else "K")
    h.call("bornvi_stein_gram_build_rows_ld", n, float(length_scale), _ptr(S), r0, r1, _ptr(K), pitch, _ext.stream_ptr(dev))
    return K


def sym_pair_shard(n, rank, world_size):
    """Strip pairs [pa, pb) of the symmetric contraction owned by `rank`, and the two row ranges they cover:
    ((pa, pb), (rows_lo_begin, rows_lo_end), (rows_hi_begin, rows_hi_end)).  None when 2^n is too small to cut
    into whole strip pairs for every rank (the row shard is used then)."""
    R = int(_ext.lib().bornvi_stein_sym_strip_rows())
    N = 1 << n
    if N % (2 * R) != 0:
        return None
    ns = N // R
    npairs = ns // 2
    chunk = -(-npairs // world_size)
    pa = min(npairs, rank * chunk)
    pb = min(npairs, pa + chunk)
    return (pa, pb), (pa * R, pb * R), ((ns - pb) * R, (ns - pa) * R)


def stein_quadform_sym_pairs(K_lo, K_hi, pa, pb, q, n, out=None):
    """This GPU's additive share of (K q, q^T K q) from its strip pairs [pa, pb) of the upper triangle:
    returns a [2^n + 1] vector (y_partial followed by ksd2_partial) -- the message of the all-reduce."""
    dev = q.device
    h = _ext.handle_for(dev)
    _chk_n(n, 1, 17)
    N = 1 << n
    _chk(q, torch.float64, dev, "q", N)
    ld = N
    if pb > pa:
        R = int(_ext.lib().bornvi_stein_sym_strip_rows())
        ld = _chk_matrix(K_lo, (pb - pa) * R, N, dev, "K_lo")
        if _chk_matrix(K_hi, (pb - pa) * R, N, dev, "K_hi") != ld:
            raise BornviError("K_lo and K_hi must have the same row pitch")
    if out is None:
        out = torch.empty(N + 1, dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", N + 1)
    ws = _ws(dev, _cached_size(h, "bornvi_stein_quadform_sym_workspace_bytes", n), "qfsym")
    h.call("bornvi_stein_quadform_sym_pairs_ld", n, _ptr(K_lo) if pb > pa else None, _ptr(K_hi) if pb > pa else None,
           ld, int(pa), int(pb), _ptr(q), C.c_void_p(out.data_ptr() + 8 * N), _ptr(out), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return out


def stein_quadform_rows(K_rows, r0, r1, q, n, out=None):
    """K_rows = rows [r0, r1) of K_p; returns a [r1 - r0 + 1] vector: those rows of K q followed by
    the partial sum over them of q_i y_i (the message one rank contributes to the all-gather)."""
    dev = K_rows.device
    h = _ext.handle_for(dev)
    _chk_n(n, 1, 17)
    nr = r1 - r0
    if not (0 <= r0 <= r1 <= (1 << n)):
        raise BornviError("stein_quadform_rows: row range out of bounds")
    _chk(K_rows, torch.float64, dev, "K_rows", nr << n)
    _chk(q, torch.float64, dev, "q", 1 << n)
    if out is None:
        out = torch.empty(nr + 1, dtype=torch.float64, device=dev)
    else:
        _chk(out, torch.float64, dev, "out", nr + 1)
    ws = _ws(dev, _cached_size(h, "bornvi_stein_quadform_workspace_bytes", n, 1), "qf")
    h.call("bornvi_stein_quadform_rows", n, _ptr(K_rows), int(r0), int(r1), _ptr(q), _ptr(out),
           C.c_void_p(out.data_ptr() + 8 * nr), _ptr(ws), ws.numel(), _ext.stream_ptr(dev))
    return out


def stein_kp_pairs(n, length_scale, zi, zj, si, sj):
    dev = si.device
    h = _ext.handle_for(dev)
    for t, dt, nm in ((zi, torch.int64, "zi"), (zj, torch.int64, "zj"), (si, torch.float64, "si"), (sj, torch.float64, "sj")):
        _chk(t, dt, dev, nm)
    M = zi.numel()
    _chk_n(n)
    if zj.numel() != M or si.numel() != M * n or sj.numel() != M * n:
        raise BornviError("stein_kp_pairs: zi, zj must be [M] and si, sj [M, n]")
    out = torch.empty(M, dtype=torch.float64, device=dev)
    h.call("bornvi_stein_kp_pairs", n, float(length_scale), M, _ptr(zi), _ptr(zj), _ptr(si), _ptr(sj), _ptr(out),
           _ext.stream_ptr(dev))
    return out


def stein_quadform(K, Q, n, want_y=True):
    """Q [B, 2^n] (or [2^n]) -> (ksd2 [B], Y [B, 2^n] or None)."""
    dev = K.device
    h = _ext.handle_for(dev)
    _chk_n(n, 1, 17)
    # K: dense [2^n, 2^n], or the [:, :2^n] view of a padded [2^n, ld] buffer (the trainer's K_p, stein_gram(ld=...))
    ld = _chk_matrix(K, 1 << n, 1 << n, dev, "K") if K.dim() == 2 else (_chk(K, torch.float64, dev, "K", 1 << (2 * n)) or (1 << n))
    if Q.numel() % (1 << n):
        raise BornviError("Q: element count is not a multiple of 2^n")
    Q2 = Q.reshape(-1, 1 << n)
    _chk(Q2, torch.float64, dev, "Q")
    B = Q2.shape[0]
    ksd2 = torch.empty(B, dtype=torch.float64, device=dev)
    Y = torch.empty_like(Q2) if want_y else None
    ws = _ws(dev, h.size("bornvi_stein_quadform_workspace_bytes", n, B), "qf")
    h.call("bornvi_stein_quadform_ld", n, _ptr(K), ld, _ptr(Q2), B, _ptr(ksd2), _ptr(Y) if want_y else None, _ptr(ws),
           ws.numel(), _ext.stream_ptr(dev))
    return ksd2, Y


def stein_sym_workspace_bytes(dev, n):
    """Workspace bytes of the symmetric contraction (stein_quadform_sym / _pairs) at this n."""
    return int(_cached_size(_ext.handle_for(dev), "bornvi_stein_quadform_sym_workspace_bytes", int(n)))


def stein_quadform_sym(K, q, n):
    """(ksd2 [1], y = K q [2^n]) for a symmetric K (as built by stein_gram): reads the upper triangle only."""
    dev = K.device
    h = _ext.handle_for(dev)
    _chk_n(n, 1, 17)
    ld = _chk_matrix(K, 1 << n, 1 << n, dev, "K")
    _chk(q, torch.float64, dev, "q", 1 << n)
    y = torch.empty(1 << n, dtype=torch.float64, device=dev)
    ksd2 = torch.empty(1, dtype=torch.float64, device=dev)
    ws = _ws(dev, _cached_size(h, "bornvi_stein_quadform_sym_workspace_bytes", n), "qfsym")
    h.call("bornvi_stein_quadform_sym_ld", n, _ptr(K), ld, _ptr(q), _ptr(ksd2), _ptr(y), _ptr(ws), ws.numel(),
           _ext.stream_ptr(dev))
    return ksd2, y


def stein_matvec_kron(S, q, n, length_scale=1.0):
    """Matrix-free (ksd2 [1], y = K_p q [2^n])."""
    _chk_n(n, 1, CIRCUIT_MAX_N)
    dev = S.device
    h = _ext.handle_for(dev)
    _chk(S, torch.float64, dev, "S", n << n)
    _chk(q, torch.float64, dev, "q", 1 << n)
    y = torch.empty(1 << n, dtype=torch.float64, device=dev)
    ksd2 = torch.empty(1, dtype=torch.float64, device=dev)
    ws = _ws(dev, _cached_size(h, "bornvi_stein_matvec_kron_workspace_bytes", n), "kron")
    h.call("bornvi_stein_matvec_kron", n, float(length_scale), _ptr(S), _ptr(q), _ptr(y), _ptr(ksd2), _ptr(ws),
           ws.numel(), _ext.stream_ptr(dev))
    return ksd2, y


def ksd_grad_finish(n, shifted, n_shift, y, ksd2, want_dldq=False):
    """-> (loss [1], grad [n_shift], dLdq [2^n] or None); see bornvi_ksd_grad_finish."""
    dev = y.device
    h = _ext.handle_for(dev)
    _chk_n(n)
    _chk(y, torch.float64, dev, "y", 1 << n)
    _chk(ksd2, torch.float64, dev, "ksd2", 1)
    if n_shift:
        _chk(shifted, torch.float64, dev, "shifted", (2 * n_shift) << n)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    grad = torch.empty(n_shift, dtype=torch.float64, device=dev)
    dldq = torch.empty(1 << n, dtype=torch.float64, device=dev) if want_dldq else None
    h.call("bornvi_ksd_grad_finish", n, _ptr(shifted) if n_shift else None, int(n_shift), _ptr(y), _ptr(ksd2),
           _ptr(loss), _ptr(dldq) if want_dldq else None, _ptr(grad) if n_shift else None, _ext.stream_ptr(dev))
    return loss, grad, dldq
