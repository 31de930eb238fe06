"""Where a call reads and writes: an arena with guard bands, and the five assertions of an entry point's memory contract.

Every device buffer of a call (inputs, outputs, in/out arguments, workspaces) is carved out of ONE uint8 tensor at an address
the test chooses, with its exact byte size.  Between the buffers and at both ends lie guard bands, each at least as large as the
call's largest buffer and never under 1 MiB, so that an overrun by a whole row, tile or partial block still lands in memory the
test owns and compares.  A band holds GUARD_BYTE (0xA5), except for the MARGIN bytes next to a buffer: those take the run's fill
(run Z 0x00, run F 0xFF, run L what an earlier, larger call of the same entry left), so that a read just outside an input sees
bytes that differ between the runs.  Everything outside the buffers a call may write is compared byte for byte after the call.

A case is a list of Buffers and a function run(mem, addr): `mem` the arena, addr[name] the buffer's address (None for an optional
pointer passed as NULL).  On the GPU an address is a device pointer and run() makes the raw C-ABI calls; the host stand-ins of
tests/test_memory_contract_host.py get offsets into a CPU arena.  check_case() runs the case and raises one of

  ExtentError        1. a byte outside the buffers the call may write changed (guards, margins, a NULL'ed optional output)
  PriorDependence    2. an `out` / `inout` buffer differs between runs Z, L and F, or a documented unwritten part was written
  InputModified      3. an `in` buffer changed
  OptionalChanged    4. passing an optional output as NULL changed another output
  PlacementChanged   5. the same buffers at the least alignment the header allows changed an output

The ROLES table below is the memory contract of include/bornvi.h written down per pointer; check_complete() holds it against the
header, so a new entry point cannot be added without its line here."""
import ctypes as C
import functools
import re

import numpy as np
import torch

GUARD_BYTE = 0xA5
MIN_GUARD = 1 << 20
MARGIN = 4096            # bytes next to every buffer that take the run's fill instead of GUARD_BYTE
FILLS = {"Z": 0x00, "F": 0xFF}
WS_ALIGN = 8             # least alignment of a workspace where the header asks for no more (the library aligns internally; the size queries carry the slack)


class ContractError(AssertionError):
    pass


class ExtentError(ContractError):
    pass


class PriorDependence(ContractError):
    pass


class InputModified(ContractError):
    pass


class OptionalChanged(ContractError):
    pass


class PlacementChanged(ContractError):
    pass


class Buffer:
    """One carved buffer.  role: in | out | inout | workspace.  data: the bytes an in / inout buffer starts from (any numpy array).
    align: the least alignment the header allows (the element size where it states nothing).  optional: the header documents
    "or NULL" for this output.  unwritten: boolean numpy mask over the BYTES of an `out` buffer that the header documents as not
    written (padded columns, rows of sites outside the range, everything once a done flag is set)."""

    def __init__(self, name, role, nbytes=None, data=None, align=8, optional=False, unwritten=None):
        assert role in ("in", "out", "inout", "workspace"), role
        if data is not None:
            data = np.ascontiguousarray(data)
            raw = np.frombuffer(data.tobytes(), dtype=np.uint8)
            nbytes = raw.size if nbytes is None else nbytes
            assert nbytes == raw.size
            self.raw = torch.from_numpy(raw.copy())
        else:
            assert role in ("out", "workspace") and nbytes is not None, (name, role)
            self.raw = None
        assert nbytes > 0, name
        self.name, self.role, self.nbytes, self.align, self.optional = name, role, int(nbytes), int(align), bool(optional)
        self.unwritten, self.alt, self.stated = None, None, False      # stated: the header states this alignment, the library enforces it
        if unwritten is not None:
            m = np.ascontiguousarray(unwritten).astype(bool).reshape(-1)
            assert m.size == self.nbytes and role in ("out", "inout"), name
            self.unwritten = torch.from_numpy(m)


class Case:
    def __init__(self, buffers, run):
        self.buffers, self.run = list(buffers), run
        names = [b.name for b in self.buffers]
        assert len(set(names)) == len(names), names


def _up(v, a):
    return (v + a - 1) // a * a


def guard_bytes(buffers):
    """Every band: at least the largest single buffer of the call, never under 1 MiB."""
    return _up(max(MIN_GUARD, max(b.nbytes for b in buffers)) + 2 * MARGIN, 4096)


def layout(buffers, base, least=False):
    """{name: offset} and the arena size.  Buffers sit at 256-byte aligned ADDRESSES (base + offset); with least=True at an address
    that is a multiple of the buffer's `align` and not of twice that."""
    G = guard_bytes(buffers)
    offs, cur = {}, 0
    for b in buffers:
        addr = _up(base + cur + G, 4096)
        if least:
            addr += b.align
            assert addr % b.align == 0 and addr % (2 * b.align) != 0
        offs[b.name] = addr - base
        cur = addr - base + b.nbytes
    return offs, cur + G + 4096


class Arena:
    def __init__(self, nbytes, device):
        self.mem = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.base = self.mem.data_ptr() if self.mem.is_cuda else 0

    def view(self, off, n):
        return self.mem[off:off + n]


def _prepare(arena, case, offs, mode, donor, alt=False):
    """Fill the arena for one run.  Z / F: guards GUARD_BYTE, margins, workspaces and outputs the fill byte.  L: the arena is left
    as the donor call left it; guards are restored, and every workspace and output starts from the first bytes of the donor's buffer
    of the same name (what a cached workspace holds: same start address, a larger call's contents)."""
    mem = arena.mem
    spans = sorted((offs[b.name], b) for b in case.buffers)
    if mode in FILLS:
        mem.fill_(GUARD_BYTE)
        for o, b in spans:
            mem[o - MARGIN:o + b.nbytes + MARGIN] = FILLS[mode]
    else:
        cur = 0
        for o, b in spans:
            mem[cur:o - MARGIN] = GUARD_BYTE
            cur = o + b.nbytes + MARGIN
        mem[cur:] = GUARD_BYTE
        for o, b in spans:
            if b.role in ("out", "workspace") and b.name in donor:
                d = donor[b.name]
                k = min(d.numel(), b.nbytes)
                mem[o:o + k] = d[:k]
    for o, b in spans:
        if b.raw is not None:
            mem[o:o + b.nbytes] = (b.alt if alt and b.alt is not None else b.raw).to(mem.device)


def _sync(mem):
    if mem.is_cuda:
        torch.cuda.synchronize(mem.device)


def run_once(arena, case, mode, donor=None, null=None, least=False, alt=False):
    """One run.  Returns {name: bytes after the call} of the out / inout buffers (unwritten parts zeroed) after assertions 1 and 3
    and the unwritten-part half of 2."""
    offs, size = layout(case.buffers, arena.base, least)
    assert size <= arena.mem.numel()
    _prepare(arena, case, offs, mode, donor or {}, alt)
    before = arena.mem.clone()
    addr = {b.name: (None if b.name == null else arena.base + offs[b.name]) for b in case.buffers}
    case.run(arena.mem, addr)
    _sync(arena.mem)
    diff = arena.mem != before
    outs = {}
    for b in case.buffers:
        o = offs[b.name]
        region = diff[o:o + b.nbytes]
        if b.name == null:
            continue                                     # a NULL'ed output is memory the call must not touch: left to the extent check
        if b.role == "in":
            if bool(region.any()):
                at = int(region.nonzero()[0])
                raise InputModified(f"run {mode}: input '{b.name}' changed at byte {at} of {b.nbytes}")
        elif b.role in ("out", "inout"):
            got = arena.mem[o:o + b.nbytes].clone()
            if b.unwritten is not None:
                m = b.unwritten.to(got.device)
                if bool((region & m).any()):
                    at = int((region & m).nonzero()[0])
                    raise PriorDependence(f"run {mode}: '{b.name}' was written at byte {at}, inside its documented unwritten part")
                got[m] = 0
            outs[b.name] = got
        if b.role != "in":
            region.zero_()
    if bool(diff.any()):
        at = int(diff.nonzero()[0])
        near = min(case.buffers, key=lambda b: min(abs(at - offs[b.name]), abs(at - offs[b.name] - b.nbytes)))
        rel = at - offs[near.name]
        where = f"{-rel} bytes before" if rel < 0 else f"{rel - near.nbytes} bytes past the end of"
        raise ExtentError(f"run {mode}{' (NULL ' + null + ')' if null else ''}{' (least alignment)' if least else ''}: byte at offset "
                          f"{at} changed outside every writable buffer, {where} '{near.name}' ({near.role}, {near.nbytes} bytes)")
    return outs


def _snapshot(arena, case, least=False):
    offs, _ = layout(case.buffers, arena.base, least)
    return {b.name: arena.mem[offs[b.name]:offs[b.name] + b.nbytes].clone() for b in case.buffers if b.role in ("out", "workspace")}


def _compare(ref, got, what, error):
    for name, want in ref.items():
        if name not in got:
            continue
        if not torch.equal(want, got[name]):
            at = int((want != got[name]).nonzero()[0])
            raise error(f"{what}: '{name}' differs at byte {at} of {want.numel()}")


def check_refusal(case, name, device, error):
    """Placement, the other half: the buffer `name`, whose alignment the header states, at an address 8 bytes off.  The call must
    be refused in the argument checks (it raises `error`) and nothing in the arena may change."""
    arena = arena_for([case], device)
    offs, _ = layout(case.buffers, arena.base)
    _prepare(arena, case, offs, "Z", {})
    before = arena.mem.clone()
    addr = {b.name: arena.base + offs[b.name] + (8 if b.name == name else 0) for b in case.buffers}
    try:
        case.run(arena.mem, addr)
    except error:
        _sync(arena.mem)
        diff = arena.mem != before
        for b in case.buffers:           # (calls of the sequence in front of the refused one may have written their own buffers)
            if b.role != "in" and b.name != name:
                diff[offs[b.name]:offs[b.name] + b.nbytes] = False
        if bool(diff.any()):
            raise ExtentError(f"'{name}' 8 bytes off its stated alignment: refused, but byte {int(diff.nonzero()[0])} of the arena changed")
        return
    raise PlacementChanged(f"'{name}' 8 bytes off its stated alignment was not refused")


def arena_for(cases, device):
    need = 0
    for c in cases:
        need = max(need, layout(c.buffers, 0, True)[1] + 4096 * (len(c.buffers) + 2))      # (the base's own alignment is not known yet)
    return Arena(need, device)


def check_case(case, donor_case, device, arena=None):
    """The five assertions for one case; donor_case is a valid call of the same entry (the next larger shape, other input values)
    whose leftovers run L starts from.  Order Z, L, F: the harshest prior contents come last."""
    arena = arena or arena_for([case, donor_case], device)
    z = run_once(arena, case, "Z")
    run_once(arena, donor_case, "Z")
    donor = _snapshot(arena, donor_case)
    l = run_once(arena, case, "L", donor=donor)
    _compare(z, l, "run L against run Z (leftovers of a larger call)", PriorDependence)
    f = run_once(arena, case, "F")
    _compare(z, f, "run F against run Z (0xFF bytes)", PriorDependence)
    for b in case.buffers:
        if b.optional:
            assert b.role == "out", b.name
            o = run_once(arena, case, "Z", null=b.name)
            _compare(z, o, f"'{b.name}' passed as NULL", OptionalChanged)
    if any(b.alt is not None for b in case.buffers):
        a = run_once(arena, case, "Z", alt=True)
        _compare(z, a, "other bytes in the parts of the inputs that are never read", PriorDependence)
    p = run_once(arena, case, "Z", least=True)
    _compare(z, p, "least alignment", PlacementChanged)
    return z


# ---------------------------------------------------------------------------------------------------------------------------
# The contract per pointer.  role[?][@align]: `?` the header documents "or NULL"; @16 the header states 16-byte alignment and the
# library refuses any other address before any launch (otherwise the element size: 16 bytes for complex128).
# "host": a host pointer (the 2 x 2 matrix of gate1q, the network descriptor, whose ARRAYS are
# device inputs).  "out-partial": an output with documented unwritten parts.

ROLES = {
    "bornvi_circuit_probs": dict(thetas="in", probs="out", workspace="workspace@16"),
    "bornvi_paramshift_probs": dict(theta="in", probs="out", workspace="workspace@16"),
    "bornvi_paramshift_probs_strided": dict(theta="in", probs="out", workspace="workspace@16"),
    "bornvi_paramshift_grad": dict(theta="in", dLdq="in", grad="out", workspace="workspace@16"),
    "bornvi_paramshift_dot_begin": dict(theta="in", q_out="out", workspace="workspace@16"),
    "bornvi_paramshift_dot_finish": dict(w="in", ksd2="in?", grad="out", loss_out="out?", workspace="workspace@16"),
    "bornvi_gate1q_apply": dict(state="inout", U="host"),
    "bornvi_cnot_apply": dict(state="inout"),
    "bornvi_born_probs": dict(state="in", probs="out"),
    "bornvi_score_from_cpts": dict(bn="host", S="out", pxz="out?"),
    "bornvi_bn_logjoint_samples": dict(bn="host", idx="in", logp="out"),
    "bornvi_bn_score_samples": dict(bn="host", idx="in", S="out", logp="out?"),
    "bornvi_stein_pairs_rowsum": dict(idx="in", S="in", r="out", total="out", workspace="workspace"),
    "bornvi_stein_gram_build": dict(S="in", K="out@16"),
    "bornvi_stein_gram_build_rows": dict(S="in", K_rows="out@16"),
    "bornvi_stein_gram_build_rows_ld": dict(S="in", K_rows="out-partial@16"),          # columns >= 2^n of a row: never written
    "bornvi_stein_kp_pairs": dict(zi="in", zj="in", si="in", sj="in", out="out"),
    "bornvi_stein_quadform": dict(K="in", Q="in", ksd2="out", Y="out?", workspace="workspace"),
    "bornvi_stein_quadform_ld": dict(K="in", Q="in", ksd2="out", Y="out?", workspace="workspace"),
    "bornvi_stein_quadform_sym": dict(K="in@16", q="in", ksd2="out", y="out", workspace="workspace@16"),
    "bornvi_stein_quadform_sym_ld": dict(K="in@16", q="in", ksd2="out", y="out", workspace="workspace@16"),
    "bornvi_stein_quadform_sym_pairs": dict(K_lo="in@16", K_hi="in@16", q="in", ksd2_partial="out", y_partial="out",
                                            workspace="workspace@16"),
    "bornvi_stein_quadform_sym_pairs_ld": dict(K_lo="in@16", K_hi="in@16", q="in", ksd2_partial="out", y_partial="out",
                                               workspace="workspace@16"),
    "bornvi_stein_quadform_rows": dict(K_rows="in", q="in", y_rows="out?", ksd2_partial="out", workspace="workspace"),
    "bornvi_stein_matvec_kron": dict(S="in", q="in", y="out", ksd2="out", workspace="workspace@16"),
    "bornvi_ksd_grad_finish": dict(shifted="in", y="in", ksd2="in", loss_out="out", dLdq_out="out?", grad="out"),
    "bornvi_shots_histogram": dict(probs="in", freq="out", epoch_dev="in", workspace="workspace"),
    "bornvi_born_table_probs": dict(w="in", q32="out", q64="out", entropy="out?", workspace="workspace"),
    "bornvi_born_table_vjp": dict(w="in", q64="in", y="in?", ksd2="in?", grad="out", loss_out="out?", workspace="workspace"),
    "bornvi_reinforce_step": dict(idx="in", logit="in", log_p="in", q32="in", baseline="inout", dLdq="out", loss="out",
                                  found_inf="out", workspace="workspace"),
    "bornvi_elbo_weights": dict(q="in", log_p="in", w="out?", neg_elbo="out", entropy="out?", workspace="workspace"),
    "bornvi_mps_probs": dict(cores="in", q64="out", q32="out?", psi="out?", Z_out="out", workspace="workspace"),
    "bornvi_mps_vjp": dict(cores="in", g="in", grad_cores="out", workspace="workspace"),
    "bornvi_mps_environments": dict(cores="in", log_Z_out="out?", workspace="workspace"),
    "bornvi_mps_sample": dict(cores="in", epoch_dev="in", idx="out", logq="out", status="out", workspace="workspace"),
    "bornvi_mps_score_vjp": dict(cores="in", idx="in", w="in", logq="out", grad_cores="out", status="out", workspace="workspace"),
    "bornvi_fisher_gram": dict(shifted="in@16", q="in@16", F="out", workspace="workspace"),
    "bornvi_spd_solve": dict(A="in", b="in", x="out", info="out", workspace="workspace"),
    "bornvi_spd_solve_batched": dict(A="in", b="in", x="out", info="out", workspace="workspace"),
    "bornvi_mps_score_rows": dict(cores="in", idx="in", rows="out-partial@16", status="out", workspace="workspace"),   # sites outside the range
    "bornvi_score_fisher_gram": dict(rows="in@16", F="out", workspace="workspace"),
    "bornvi_mps_score_sample_gram": dict(cores="in", idx="in", T="out", status="out", env_workspace="workspace", workspace="workspace"),
    "bornvi_mps_score_jvp": dict(cores="in", idx="in", v="in", t="out", status="out", env_workspace="workspace"),
    "bornvi_mps_log_marginals": dict(cores="in", mask="in", value="in", logm="out", status="out", workspace="workspace"),
    "bornvi_mps_sample_clamped": dict(cores="in", mask="in", value="in", epoch_dev="in", idx="out", logq="out", logm="out",
                                      status="out", workspace="workspace"),
    "bornvi_mps_marginals": dict(cores="in", m1="out", m2="out?", workspace="workspace"),
    "bornvi_mps_canonicalise": dict(cores="in", cores_out="out", schmidt="out", discarded="out", rank="out", log_norm="out",
                                    status="out", workspace="workspace"),
    "bornvi_bn_sample": dict(bn="host", epoch_dev="in", idx="out", logp="out", status="out"),
    "bornvi_mps_log_marginals_vjp": dict(cores="in", mask="in", value="in", c="in", grad_cores="out", logm="out", status="out",
                                         workspace="workspace"),
    "bornvi_cg_init": dict(g="in", x="out", r="out", p="out", state="out", info="out"),
    "bornvi_cg_step": dict(Fp="in", x="inout", r="inout", p="inout", state="inout"),        # nothing written once the done flag is set
    "bornvi_cg_finish": dict(g="in", x="inout", state="in", info="out", iters="out", relres="out"),
    "bornvi_paramshift_states": dict(theta="in", states="out@16", workspace="workspace"),
    "bornvi_qfi_gram": dict(phi="in@16", psi="in@16", Q="out", workspace="workspace"),
    "bornvi_clip_cast_grad": dict(grad64="in", grad32="out", total_norm="out"),
    "bornvi_clip_cast_grad_guard": dict(grad64="in", loss="in", grad32="out", total_norm="out", found_inf="out"),
    "bornvi_clip_adam_step": dict(grad64="in", loss="in", theta="inout", grad32="out", theta64="out", exp_avg="inout",
                                  exp_avg_sq="inout", counters="inout", lr_table="in", total_norm="out",
                                  loss_history="out-partial?", norm_history="out-partial?"),    # only this epoch's entry is written
    "bornvi_adjoint_state": dict(theta="in", state="out", probs="out?", workspace="workspace@16"),
    "bornvi_adjoint_vjp": dict(theta="in", state="in", dLdq="in", grad="out", workspace="workspace@16"),
}
_ROLE = re.compile(r"(in|out|inout|workspace|host|out-partial)(\?)?(@\d+)?")


def role_of(fn, param):
    """(role, optional, stated alignment or None) of one pointer."""
    m = _ROLE.fullmatch(ROLES[fn][param])
    assert m, (fn, param, ROLES[fn][param])
    return ("out" if m[1] == "out-partial" else m[1]), bool(m[2]), (int(m[3][1:]) if m[3] else None)


def header_params(text):
    """{function: [(type, name)]} of every declaration of the header text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(bornvi_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for a in m[2].split(","):
            a = " ".join(a.split())
            if a in ("void", ""):
                continue
            pm = re.fullmatch(r"(.*?)(\w+)", a)
            params.append((pm[1].strip(), pm[2]))
        out[m[1]] = params
    return out


def launching_functions(text):
    """Declared functions with a `stream` parameter, in declaration order: the ones that touch device memory."""
    from tensornetworks_amd import _ext
    declared = _ext.parse_header(text)[2]
    params = header_params(text)
    return [f for f in declared if any(t == "bornvi_stream" for t, _ in params[f])]


def check_complete(text, roles, covered):
    """The problems that keep the specification from covering the header text: a launching function without a role table or
    without a GPU case, a pointer parameter without a role, a role for a parameter the header does not have."""
    params = header_params(text)
    problems = []
    for f in launching_functions(text):
        if f not in roles:
            problems.append(f"{f}: no memory contract")
            continue
        if f not in covered:
            problems.append(f"{f}: no case runs it")
        pointers = [n for t, n in params[f] if "*" in t]
        for n in pointers:
            if n not in roles[f]:
                problems.append(f"{f}: pointer '{n}' has no role")
            elif not _ROLE.fullmatch(roles[f][n]):
                problems.append(f"{f}: pointer '{n}' has the unknown role '{roles[f][n]}'")
        problems += [f"{f}: role for '{n}', which is no pointer parameter" for n in roles[f] if n not in pointers]
    return problems


# ---------------------------------------------------------------------------------------------------------------------------
# GPU cases: good arguments, exact extents, the workspace size query and, for pairs and chains, the sequence of every entry.
# A family names the functions it runs (`covers`), its shapes (the smallest at which each kernel changes path, from the
# family's own test file) and build(b, shape, seed), which fills a Builder: buffers through b.inp / b.out / b.ws, whose role,
# "or NULL" and alignment come from ROLES, and calls in order.  The fills are applied before the first call of a sequence only.
#
# Workspace regions, read off each launcher (who writes a region, who reads it), stand in a comment above each family.

OPTION_NAMES = ("tile_bits", "tile_bits_multi", "fast_workgroups_per_cu", "reg_wires", "read_map", "zero_support", "direct_stages",
                "prefix_share", "batched_quadform", "grad_engine")


class Desc:
    """A network descriptor: a host struct whose five arrays are device inputs of the case."""

    def __init__(self, num_nodes, max_parents, arrays):
        self.num_nodes, self.max_parents, self.arrays = num_nodes, max_parents, arrays


class Builder:
    def __init__(self, handle):
        from tensornetworks_amd import _ext
        self.h, self.ext, self.buffers, self.steps = handle, _ext, [], []

    # -- buffers
    def _add(self, fn, param, name, **kw):
        role, optional, stated = role_of(fn, param)
        kw.setdefault("align", stated)
        buf = Buffer(name or param, role, optional=optional and role == "out", **kw)
        buf.stated = stated is not None
        self.buffers.append(buf)
        return buf

    def inp(self, fn, param, data, name=None, unwritten=None, alt=None):
        """An `in` or `inout` pointer of fn starting from `data`; alt: the same with other bytes in the parts the header documents
        as never read."""
        data = np.ascontiguousarray(data)
        role, _, stated = role_of(fn, param)
        assert role in ("in", "inout"), (fn, param, role)
        buf = self._add(fn, param, name, data=data, align=stated or data.dtype.itemsize, unwritten=unwritten)
        buf.alt = None if alt is None else torch.from_numpy(np.frombuffer(np.ascontiguousarray(alt).tobytes(), dtype=np.uint8).copy())
        return buf

    def out(self, fn, param, dtype, count, name=None, unwritten=None):
        role, _, stated = role_of(fn, param)
        assert role == "out", (fn, param, role)
        dt = np.dtype(dtype)
        return self._add(fn, param, name, nbytes=dt.itemsize * int(count), align=stated or dt.itemsize, unwritten=unwritten)

    def ws(self, fn, param, nbytes, name=None):
        role, _, stated = role_of(fn, param)
        assert role == "workspace", (fn, param, role)
        return self._add(fn, param, name, nbytes=int(nbytes), align=stated or WS_ALIGN)

    def desc(self, packed):
        arrays = {k: self._add_raw("bn_" + k, np.ascontiguousarray(packed[k])) for k in ("role", "n_parents", "parents", "cpt_off", "cpt")}
        return Desc(int(np.asarray(packed["role"]).size), int(np.asarray(packed["parents"]).shape[1]), arrays)

    def _add_raw(self, name, data):
        buf = Buffer(name, "in", data=data, align=data.dtype.itemsize)
        self.buffers.append(buf)
        return buf

    # -- calls
    def option(self, name, value):
        """Set an option of the handle NOW, because the size queries that follow depend on it (plan, gradient engine), and record
        it as a step: run() sets it again before the calls, since the donor's build may have changed it in between.  The test's
        fixture puts every option back after the case."""
        assert name in OPTION_NAMES, name
        set_option(self.h, name.encode(), int(value))
        self.steps.append(("bornvi_set_option", (name.encode(), int(value))))

    def size(self, query, *args):
        return self.h.size(query, *args)

    def call(self, fn, *args):
        assert fn in ROLES, fn
        nargs = len(self.ext.PROTOTYPES[fn][1])
        assert len(args) == nargs - 2, (fn, len(args), nargs)          # without the handle and the stream
        self.steps.append((fn, args))

    def case(self):
        steps, h, BnDesc = self.steps, self.h, self.ext.BnDesc

        def run(mem, addr):
            alive = []
            for fn, args in steps:
                if fn == "bornvi_set_option":
                    set_option(h, *args)
                    continue
                real = []
                for a in args:
                    if isinstance(a, Buffer):
                        real.append(addr[a.name])
                    elif isinstance(a, Desc):
                        d = BnDesc(a.num_nodes, a.max_parents, *(addr[a.arrays[k].name] for k in ("role", "n_parents", "parents", "cpt_off", "cpt")))
                        alive.append(d)
                        real.append(C.byref(d))
                    elif isinstance(a, np.ndarray):                    # a host array
                        alive.append(a)
                        real.append(a.ctypes.data)
                    else:
                        real.append(a)
                h.call(fn, *real, None)
        return Case(self.buffers, run)


def set_option(h, name, value):
    """Set an option where it differs (a planner option clears the plan cache when set)."""
    v = C.c_longlong(0)
    h.call("bornvi_get_option", name, C.byref(v))
    if int(v.value) != value:
        h.call("bornvi_set_option", name, value)


def shape_weight(shape):
    """The default measure of a call's size: the product of the shape's numbers (flags and names count as 1)."""
    w = 1
    for v in (shape if isinstance(shape, tuple) else (shape,)):
        if isinstance(v, int) and v > 1:
            w *= v
    return w


class Family:
    def __init__(self, name, covers, shapes, build, weight=shape_weight):
        self.name, self.covers, self.shapes, self.build, self.weight = name, tuple(covers), list(shapes), build, weight

    def case(self, handle, i, seed):
        b = Builder(handle)
        self.build(b, self.shapes[i], seed)
        return b.case()

    def donor(self, handle, i):
        """A valid call of the same entry whose leftovers run L starts from: the next larger shape of the list by the family's
        weight (the first of equals), with other input values; for the largest, the same shape with other values."""
        w = [self.weight(s) for s in self.shapes]
        larger = [j for j in range(len(w)) if w[j] > w[i]]
        return self.case(handle, min(larger, key=lambda j: (w[j], j)) if larger else i, 1)


FAMILIES = []


def family(name, covers, shapes, weight=shape_weight):
    def deco(build):
        FAMILIES.append(Family(name, covers, shapes, build, weight))
        return build
    return deco


def covered():
    return {f for fam in FAMILIES for f in fam.covers}


def rng_for(seed, *key):
    return np.random.default_rng([int(seed)] + [int(k) for k in key])


def f64(b, fn, param, count, **kw):
    return b.out(fn, param, np.float64, count, **kw)


def i32(b, fn, param, count=1, **kw):
    return b.out(fn, param, np.int32, count, **kw)


def pad_mask(rows, cols, ld, itemsize=8):
    """Byte mask of the columns cols .. ld - 1 of a [rows, ld] matrix."""
    m = np.zeros((rows, ld, itemsize), bool)
    m[:, cols:] = True
    return m


# ---- circuits -----------------------------------------------------------------------------------------------------------
# bornvi_circuit_probs, bornvi_paramshift_probs(_strided) (api.hip: circuit_batch; regions from the raw pointer, 256-byte pieces):
#   gates  [chunk][slots][8]      build_gates_kernel writes every slot of every circuit of the chunk; every pass reads them
#   stateA / stateB [chunk][2^n]  pass i writes one, pass i + 1 reads it; with zero_support = 1 the first two passes leave out
#                                 tiles that no later pass loads (tests/plan_emulator.py poisons them on the CPU)
#   trash  [2^n]                  prefix sharing only: rows the final pass must not deliver; written, never read
# bornvi_paramshift_grad: shifted [2 ns][2^n] written by the circuit batch, read by the dot kernel; then the circuit regions.
# bornvi_paramshift_states: thetas [chunk][P] (pi_shift_thetas_kernel -> build_gates), gates, stateA / stateB as above; the tail
#   kernel reads the final buffer and writes `states`.
# bornvi_paramshift_dot_begin / _finish: gates, stateA, stateB as above for all 1 + 2 p_count circuits (begin writes, finish's last
#   pass reads the state the last-but-one pass left); partials [2 p_count][tiles] written by finish's last pass, read by dot_finish.
# bornvi_adjoint_state: `other` [2^n] at +256, the entangler's ping-pong partner: written by every entangler block before read.
# bornvi_adjoint_vjp: phi (memcpy of state), lam (adj_lambda_kernel), phi2 / lam2 (entangler writes before reads), partials
#   [blocks][workgroups][4]: every workgroup of a block's launch writes its four slots, adj_reduce reads them; grad is memset.
ANSATZ = {"hardware_efficient": 0, "all_to_all": 1, "basic": 2}
R3_CASES = [("all_to_all", 12, 2, 9), ("all_to_all", 13, 2, 9), ("hardware_efficient", 13, 3, 11), ("hardware_efficient", 14, 3, 11),
            ("hardware_efficient", 12, 4, 9), ("basic", 14, 3, 11)]          # test_gpu_r3_spread.CASES
R3_DOT_CASES = [("all_to_all", 14, 3, 11), ("hardware_efficient", 14, 3, 11)]   # test_gpu_r3_spread.DOT_CASES
GENERIC = [("hardware_efficient", 2, 2, 0), ("basic", 8, 2, 0)]             # the generic pass kernel (kb 0: default options)
# every circuit entry: (cases + generic) x zero_support {1, 0} x {workspace for the full batch, one that forces two chunks}.  At
# n = 2 a circuit is smaller than the slack of the size query, so no size forces chunks there: full only.
CIRCUIT_SHAPES = [GENERIC[0] + (zs, "full") for zs in (1, 0)] + \
                 [c + (zs, wsk) for c in GENERIC[1:] + R3_CASES for zs in (1, 0) for wsk in ("full", "chunks")]


def circuit_weight(shape):
    return (shape[1], shape[2])          # (n, layers): the state and the gate records


def circuit_options(b, kb, zero_support=1):
    if kb:
        b.option("reg_wires", 3)
        b.option("read_map", 1)
        b.option("tile_bits", kb)
    else:
        b.option("reg_wires", 3)
        b.option("read_map", -1)
        b.option("tile_bits", 13)          # (the defaults; setting tile_bits also sets tile_bits_multi)
        b.option("tile_bits_multi", 0)
    b.option("zero_support", zero_support)


def num_params(b, ansatz, n, L):
    return int(b.ext.lib().bornvi_num_params(ANSATZ[ansatz], n, L))


def circuit_ws(b, a, n, L, batch, kind):
    """The full-batch size, or one that holds more than half of the batch and not all of it: two chunks."""
    full = b.size("bornvi_circuit_workspace_bytes", ANSATZ[a], n, L, batch)
    if kind == "full":
        return full
    part = b.size("bornvi_circuit_workspace_bytes", ANSATZ[a], n, L, (batch + 1) // 2)
    assert part < full
    return part


@family("circuit_probs", ["bornvi_circuit_probs"], CIRCUIT_SHAPES, circuit_weight)
def _circuit_probs(b, shape, seed):
    a, n, L, kb, zs, wsk = shape
    circuit_options(b, kb, zs)
    batch, P, fn = 5, num_params(b, a, n, L), "bornvi_circuit_probs"
    th = b.inp(fn, "thetas", rng_for(seed, n, L).uniform(-np.pi, np.pi, (batch, P)))
    pr = f64(b, fn, "probs", batch << n)
    ws = b.ws(fn, "workspace", circuit_ws(b, a, n, L, batch, wsk))
    b.call(fn, ANSATZ[a], n, L, batch, th, pr, ws, ws.nbytes)


@family("paramshift_probs", ["bornvi_paramshift_probs"], CIRCUIT_SHAPES, circuit_weight)
def _paramshift_probs(b, shape, seed):
    a, n, L, kb, zs, wsk = shape
    circuit_options(b, kb, zs)
    P, fn = num_params(b, a, n, L), "bornvi_paramshift_probs"
    p0, p1 = 1, 4
    rows = 1 + 2 * (p1 - p0)
    th = b.inp(fn, "theta", rng_for(seed, n, L).uniform(-np.pi, np.pi, P))
    pr = f64(b, fn, "probs", rows << n)
    ws = b.ws(fn, "workspace", circuit_ws(b, a, n, L, rows, wsk))
    b.call(fn, ANSATZ[a], n, L, th, p0, p1, 1, pr, ws, ws.nbytes)


# option prefix_share = 1: [gates | stateA | stateB | trash row], the base circuit in slot 0 of every chunk (api.hip: circuit_batch)
@family("paramshift_probs_prefix_share", ["bornvi_paramshift_probs"],
        [c + (1, wsk) for c in (R3_CASES[0], R3_CASES[2], R3_CASES[4]) for wsk in ("full", "chunks")], circuit_weight)
def _paramshift_probs_shared(b, shape, seed):
    b.option("prefix_share", 1)
    _paramshift_probs(b, shape, seed)


@family("paramshift_probs_strided", ["bornvi_paramshift_probs_strided"], CIRCUIT_SHAPES, circuit_weight)
def _paramshift_probs_strided(b, shape, seed):
    a, n, L, kb, zs, wsk = shape
    circuit_options(b, kb, zs)
    P, fn = num_params(b, a, n, L), "bornvi_paramshift_probs_strided"
    p0, count, stride = 1, 3, 2
    rows = 2 * count
    th = b.inp(fn, "theta", rng_for(seed, n, L).uniform(-np.pi, np.pi, P))
    pr = f64(b, fn, "probs", rows << n)
    ws = b.ws(fn, "workspace", circuit_ws(b, a, n, L, rows, wsk))
    b.call(fn, ANSATZ[a], n, L, th, p0, count, stride, 0, pr, ws, ws.nbytes)


# "adjoint": option grad_engine = 1, the call answers with the adjoint walk: [state | gfull [P] | the adjoint workspace], its own
# term of the size query (state and gfull are written by bornvi_adjoint_state / _vjp before the copy into grad reads gfull)
GRAD_SHAPES = CIRCUIT_SHAPES + [c + (1, "adjoint") for c in GENERIC + R3_CASES]


@family("paramshift_grad", ["bornvi_paramshift_grad"], GRAD_SHAPES, circuit_weight)
def _paramshift_grad(b, shape, seed):
    a, n, L, kb, zs, wsk = shape
    circuit_options(b, kb, zs)
    b.option("grad_engine", 1 if wsk == "adjoint" else 0)
    P, fn = num_params(b, a, n, L), "bornvi_paramshift_grad"
    p0, p1 = 1, 4
    r = rng_for(seed, n, L)
    th = b.inp(fn, "theta", r.uniform(-np.pi, np.pi, P))
    dl = b.inp(fn, "dLdq", r.standard_normal(1 << n))
    g = f64(b, fn, "grad", p1 - p0)
    need = b.size("bornvi_paramshift_grad_workspace_bytes", ANSATZ[a], n, L, p0, p1)
    if wsk == "chunks":          # the shifted rows, then a circuit workspace that holds more than half of the 2 ns circuits, not all
        rows = 2 * (p1 - p0)
        need += circuit_ws(b, a, n, L, rows, "chunks") - circuit_ws(b, a, n, L, rows, "full")
    ws = b.ws(fn, "workspace", need)
    b.call(fn, ANSATZ[a], n, L, th, dl, p0, p1, g, ws, ws.nbytes)


@family("paramshift_states", ["bornvi_paramshift_states"], CIRCUIT_SHAPES, circuit_weight)
def _paramshift_states(b, shape, seed):
    a, n, L, kb, zs, wsk = shape
    circuit_options(b, kb, zs)
    P, fn = num_params(b, a, n, L), "bornvi_paramshift_states"
    p0, count = 1, 3
    rows = 1 + count
    th = b.inp(fn, "theta", rng_for(seed, n, L).uniform(-np.pi, np.pi, P))
    st = b.out(fn, "states", np.complex128, rows << n)
    ws = b.ws(fn, "workspace", b.size("bornvi_paramshift_states_workspace_bytes", ANSATZ[a], n, L, rows if wsk == "full" else rows // 2 + 1))
    b.call(fn, ANSATZ[a], n, L, th, p0, count, 1, st, ws, ws.nbytes)


@family("paramshift_dot", ["bornvi_paramshift_dot_begin", "bornvi_paramshift_dot_finish"], [c + (zs,) for c in R3_DOT_CASES for zs in (1, 0)],
        circuit_weight)
def _paramshift_dot(b, shape, seed):
    a, n, L, kb, zs = shape
    circuit_options(b, kb, zs)
    P, f0, f1 = num_params(b, a, n, L), "bornvi_paramshift_dot_begin", "bornvi_paramshift_dot_finish"
    p0, count, stride = 1, 3, 2
    r = rng_for(seed, n, L)
    th = b.inp(f0, "theta", r.uniform(-np.pi, np.pi, P))
    q = f64(b, f0, "q_out", 1 << n)
    ws = b.ws(f0, "workspace", b.size("bornvi_paramshift_dot_workspace_bytes", ANSATZ[a], n, L, count))
    w = b.inp(f1, "w", r.standard_normal(1 << n))
    k2 = b.inp(f1, "ksd2", np.array([3.7]))
    g = f64(b, f1, "grad", count)
    lo = f64(b, f1, "loss_out", 1)
    b.call(f0, ANSATZ[a], n, L, th, p0, count, stride, q, ws, ws.nbytes)
    b.call(f1, ANSATZ[a], n, L, count, w, k2, g, lo, ws, ws.nbytes)


# the (ansatz, n, layers) of the circuit cases (the walk has no planner: no tile size, zero support or chunks), and n = 1
ADJ_SHAPES = [("hardware_efficient", 1, 2)] + sorted({c[:3] for c in GENERIC + R3_CASES + R3_DOT_CASES}, key=lambda c: (c[1], c[2], c[0]))


@family("adjoint_state", ["bornvi_adjoint_state"], ADJ_SHAPES, circuit_weight)
def _adjoint_state(b, shape, seed):
    a, n, L = shape
    P, fn = num_params(b, a, n, L), "bornvi_adjoint_state"
    th = b.inp(fn, "theta", rng_for(seed, n, L).uniform(-np.pi, np.pi, P))
    st = b.out(fn, "state", np.complex128, 1 << n)
    pr = f64(b, fn, "probs", 1 << n)
    ws = b.ws(fn, "workspace", b.size("bornvi_adjoint_workspace_bytes", ANSATZ[a], n, L))
    b.call(fn, ANSATZ[a], n, L, th, st, pr, ws, ws.nbytes)


def unit_states(r, rows, n):
    s = r.standard_normal((rows, 1 << n, 2))
    return np.ascontiguousarray(s / np.sqrt((s * s).sum(axis=(1, 2), keepdims=True))).view(np.complex128)[..., 0]


@family("adjoint_vjp", ["bornvi_adjoint_vjp"], ADJ_SHAPES, circuit_weight)
def _adjoint_vjp(b, shape, seed):
    a, n, L = shape
    P, fn = num_params(b, a, n, L), "bornvi_adjoint_vjp"
    r = rng_for(seed, n, L)
    th = b.inp(fn, "theta", r.uniform(-np.pi, np.pi, P))
    st = b.inp(fn, "state", unit_states(r, 1, n))          # (any normalised state: the walk is linear in it)
    dl = b.inp(fn, "dLdq", r.standard_normal(1 << n))
    g = f64(b, fn, "grad", P)
    ws = b.ws(fn, "workspace", b.size("bornvi_adjoint_workspace_bytes", ANSATZ[a], n, L))
    b.call(fn, ANSATZ[a], n, L, th, st, dl, g, ws, ws.nbytes)


# ---- un-fused gates (no workspace) ------------------------------------------------------------------------------------------
GATE_SHAPES = [(2, 1), (3, 2), (12, 3)]          # (n, batch): one workgroup, several


@family("gate1q_apply", ["bornvi_gate1q_apply"], GATE_SHAPES)
def _gate1q(b, shape, seed):
    n, batch = shape
    r, fn = rng_for(seed, n), "bornvi_gate1q_apply"
    st = b.inp(fn, "state", unit_states(r, batch, n))
    U = np.ascontiguousarray(r.standard_normal(8))
    b.call(fn, n, batch, st, n - 1, U)


@family("cnot_apply", ["bornvi_cnot_apply"], GATE_SHAPES)
def _cnot(b, shape, seed):
    n, batch = shape
    st = b.inp("bornvi_cnot_apply", "state", unit_states(rng_for(seed, n), batch, n))
    b.call("bornvi_cnot_apply", n, batch, st, 0, n - 1)


@family("born_probs", ["bornvi_born_probs"], GATE_SHAPES)
def _born_probs(b, shape, seed):
    n, batch = shape
    fn = "bornvi_born_probs"
    st = b.inp(fn, "state", unit_states(rng_for(seed, n), batch, n))
    pr = f64(b, fn, "probs", batch << n)
    b.call(fn, n, batch, st, pr)


# ---- network calls (no workspace) -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def packed_network(n, seed):
    from tensornetworks_amd.bayesian_network import pack_network, synthetic_network
    bn, latent, _, x = synthetic_network(n, seed=seed)
    return pack_network(bn, latent, x)


@family("score_from_cpts", ["bornvi_score_from_cpts"], [2, 5, 10])
def _score_from_cpts(b, n, seed):
    fn = "bornvi_score_from_cpts"
    d = b.desc(packed_network(n, seed))
    S = f64(b, fn, "S", n << n)
    pxz = f64(b, fn, "pxz", 1 << n)
    b.call(fn, d, n, S, pxz)


BN_SAMPLE_SHAPES = [(2, 1), (5, 3), (20, 300), (63, 65)]         # (n, B)


def sample_idx(r, n, B):
    return r.integers(0, 1 << n, B, dtype=np.int64) if n < 63 else r.integers(0, 1 << 62, B, dtype=np.int64) * 2 + r.integers(0, 2, B)


@family("bn_logjoint_samples", ["bornvi_bn_logjoint_samples"], BN_SAMPLE_SHAPES)
def _bn_logjoint(b, shape, seed):
    n, B = shape
    fn = "bornvi_bn_logjoint_samples"
    d = b.desc(packed_network(n, seed))
    idx = b.inp(fn, "idx", sample_idx(rng_for(seed, n, B), n, B))
    lp = f64(b, fn, "logp", B)
    b.call(fn, d, n, B, idx, 1e-30, lp)


@family("bn_score_samples", ["bornvi_bn_score_samples"], BN_SAMPLE_SHAPES)
def _bn_score(b, shape, seed):
    n, B = shape
    fn = "bornvi_bn_score_samples"
    d = b.desc(packed_network(n, seed))
    idx = b.inp(fn, "idx", sample_idx(rng_for(seed, n, B), n, B))
    S = f64(b, fn, "S", B * n)
    lp = f64(b, fn, "logp", B)
    b.call(fn, d, n, B, idx, 1e-30, S, lp)


@functools.lru_cache(maxsize=None)
def packed_latent_network(n, seed):
    """The synthetic network with its observed leaf dropped (bornvi_bn_sample refuses observed roles)."""
    p = packed_network(n, seed)
    keep = np.asarray(p["role"]) >= 0
    assert keep[:int(keep.sum())].all()                 # the latent nodes come first, so parent indices stay valid
    k = int(keep.sum())
    return {"role": np.asarray(p["role"])[:k], "n_parents": np.asarray(p["n_parents"])[:k], "parents": np.asarray(p["parents"])[:k],
            "cpt_off": np.asarray(p["cpt_off"])[:k], "cpt": np.asarray(p["cpt"])}


@family("bn_sample", ["bornvi_bn_sample"], BN_SAMPLE_SHAPES)
def _bn_sample(b, shape, seed):
    n, B = shape
    fn = "bornvi_bn_sample"
    d = b.desc(packed_latent_network(n, seed))
    ep = b.inp(fn, "epoch_dev", np.array([3 + seed], np.int64))
    idx = b.out(fn, "idx", np.int64, B)
    lp = f64(b, fn, "logp", B)
    st = i32(b, fn, "status")
    b.call(fn, d, n, B, 1234 + seed, ep, idx, lp, st)


# bornvi_stein_pairs_rowsum (kernels_ksd_sampled.hip: KpLayout): the packed operands and the partials [G][B] of the row sums are
# written by the pack and the pair kernels before the finishing launch reads them.
@family("stein_pairs_rowsum", ["bornvi_stein_pairs_rowsum"], [(5, 2), (5, 33), (20, 300), (63, 1025)])
def _stein_pairs(b, shape, seed):
    n, B = shape
    fn, r = "bornvi_stein_pairs_rowsum", rng_for(seed, n, B)
    idx = b.inp(fn, "idx", sample_idx(r, n, B))
    S = b.inp(fn, "S", r.uniform(-1, 1, (B, n)))
    rr = f64(b, fn, "r", B)
    tot = f64(b, fn, "total", 1)
    ws = b.ws(fn, "workspace", b.size("bornvi_stein_pairs_workspace_bytes", n, B))
    b.call(fn, n, B, 1.0, idx, S, rr, tot, ws, ws.nbytes)


# ---- dense Stein --------------------------------------------------------------------------------------------------------
def scores(n, seed):
    import hp_reference as hp
    return hp.scores("mild", n, seed)


def qvec(n, seed, rows=None):
    import hp_reference as hp
    if rows is None:
        return hp.qvec("dirichlet", n, seed)
    return np.stack([hp.qvec("dirichlet", n, seed + 10 * i) for i in range(rows)])


DENSE_N = [2, 8, 9, 11]


@family("stein_gram_build", ["bornvi_stein_gram_build"], DENSE_N)
def _gram_build(b, n, seed):
    fn = "bornvi_stein_gram_build"
    S = b.inp(fn, "S", scores(n, seed))
    K = f64(b, fn, "K", 1 << (2 * n))
    b.call(fn, n, 0.7, S, K)


def row_range(n):
    N = 1 << n
    return (1, N - 1) if N <= 4 else (N // 4 + 2, N // 2 + 4)       # a strict sub-range, even start (a row pair of the kernel)


@family("stein_gram_build_rows", ["bornvi_stein_gram_build_rows"], DENSE_N)
def _gram_build_rows(b, n, seed):
    fn = "bornvi_stein_gram_build_rows"
    r0, r1 = row_range(n)
    S = b.inp(fn, "S", scores(n, seed))
    K = f64(b, fn, "K_rows", (r1 - r0) << n)
    b.call(fn, n, 0.7, S, r0, r1, K)


@family("stein_gram_build_rows_ld", ["bornvi_stein_gram_build_rows_ld"], [(n, pad) for n in DENSE_N for pad in (0, 32)])
def _gram_build_rows_ld(b, shape, seed):
    n, pad = shape
    fn, ld = "bornvi_stein_gram_build_rows_ld", (1 << n) + pad
    r0, r1 = row_range(n)
    S = b.inp(fn, "S", scores(n, seed))
    K = f64(b, fn, "K_rows", (r1 - r0) * ld, unwritten=pad_mask(r1 - r0, 1 << n, ld) if pad else None)
    b.call(fn, n, 0.7, S, r0, r1, K, ld)


@family("stein_kp_pairs", ["bornvi_stein_kp_pairs"], [(2, 1), (6, 3), (14, 1000)])
def _kp_pairs(b, shape, seed):
    n, M = shape
    fn, r = "bornvi_stein_kp_pairs", rng_for(seed, n, M)
    zi = b.inp(fn, "zi", r.integers(0, 1 << n, M, dtype=np.int64))
    zj = b.inp(fn, "zj", r.integers(0, 1 << n, M, dtype=np.int64))
    si = b.inp(fn, "si", r.uniform(-1, 1, (M, n)))
    sj = b.inp(fn, "sj", r.uniform(-1, 1, (M, n)))
    o = f64(b, fn, "out", M)
    b.call(fn, n, 0.7, M, zi, zj, si, sj, o)


@functools.lru_cache(maxsize=None)
def sym_matrix(n, seed):
    a = np.random.default_rng([seed, n, 77]).standard_normal((1 << n, 1 << n))
    return a + a.T


def padded(K, pad, fill):
    out = np.full((K.shape[0], K.shape[1] + pad), fill)
    out[:, :K.shape[1]] = K
    return out


def k_input(b, fn, param, K, pad):
    """K with `pad` padded columns per row, never read: NaN in them, and other bytes (1.0) in a run of their own."""
    if not pad:
        return b.inp(fn, param, K)
    return b.inp(fn, param, padded(K, pad, np.nan), alt=padded(K, pad, 1.0))


# bornvi_stein_quadform(_ld) (kernels_stein.hip: launch_quadform): partials [quadform_partials(rows)] written by the row kernel, read
#   by the finishing launch; batched form: Y [B][2^n] in the workspace when the caller passes none -- written by the matrix-core
#   kernel, read by the ksd2 reduction.
# bornvi_stein_quadform_sym(_ld), _sym_pairs(_ld): column partials per band written by the band kernel before the combine reads
#   them.  bornvi_stein_quadform_rows: as launch_quadform.
@family("stein_quadform", ["bornvi_stein_quadform"], [(n, B) for n in DENSE_N for B in (1, 3)])
def _quadform(b, shape, seed):
    n, B = shape
    fn = "bornvi_stein_quadform"
    K = b.inp(fn, "K", sym_matrix(n, seed))
    Q = b.inp(fn, "Q", qvec(n, seed, B))
    k2 = f64(b, fn, "ksd2", B)
    Y = f64(b, fn, "Y", B << n)
    ws = b.ws(fn, "workspace", b.size("bornvi_stein_quadform_workspace_bytes", n, B))
    b.call(fn, n, K, Q, B, k2, Y, ws, ws.nbytes)


@family("stein_quadform_ld", ["bornvi_stein_quadform_ld"], [(n, 0, B) for n in DENSE_N for B in (1, 3)] + [(n, 32, 3) for n in DENSE_N if n >= 8])          # (a padded K: n >= 8, B >= 2 only)
def _quadform_ld(b, shape, seed):
    n, pad, B = shape
    fn = "bornvi_stein_quadform_ld"
    K = k_input(b, fn, "K", sym_matrix(n, seed), pad)
    Q = b.inp(fn, "Q", qvec(n, seed, B))
    k2 = f64(b, fn, "ksd2", B)
    Y = f64(b, fn, "Y", B << n)
    ws = b.ws(fn, "workspace", b.size("bornvi_stein_quadform_workspace_bytes", n, B))
    b.call(fn, n, K, (1 << n) + pad, Q, B, k2, Y, ws, ws.nbytes)


@family("stein_quadform_sym", ["bornvi_stein_quadform_sym"], DENSE_N)
def _quadform_sym(b, n, seed):
    fn = "bornvi_stein_quadform_sym"
    K = b.inp(fn, "K", sym_matrix(n, seed))
    q = b.inp(fn, "q", qvec(n, seed))
    k2 = f64(b, fn, "ksd2", 1)
    y = f64(b, fn, "y", 1 << n)
    ws = b.ws(fn, "workspace", b.size("bornvi_stein_quadform_sym_workspace_bytes", n))
    b.call(fn, n, K, q, k2, y, ws, ws.nbytes)


@family("stein_quadform_sym_ld", ["bornvi_stein_quadform_sym_ld"], [(n, 0) for n in DENSE_N] + [(n, 32) for n in DENSE_N if n >= 9])          # (a padded K: n >= 9 only)
def _quadform_sym_ld(b, shape, seed):
    n, pad = shape
    fn = "bornvi_stein_quadform_sym_ld"
    K = k_input(b, fn, "K", sym_matrix(n, seed), pad)
    q = b.inp(fn, "q", qvec(n, seed))
    k2 = f64(b, fn, "ksd2", 1)
    y = f64(b, fn, "y", 1 << n)
    ws = b.ws(fn, "workspace", b.size("bornvi_stein_quadform_sym_workspace_bytes", n))
    b.call(fn, n, K, (1 << n) + pad, q, k2, y, ws, ws.nbytes)


def strip_pairs(n):
    """(pair_begin, pair_end): a strict sub-range of the n_strips / 2 pairs where there is more than one."""
    pairs = (1 << n) // 256 // 2
    return (0, 1) if pairs == 1 else (1, pairs - 1)


def sym_pairs_case(b, fn, n, pad, seed):
    p0, p1 = strip_pairs(n)
    strips = (1 << n) // 256
    K = sym_matrix(n, seed)
    lo = k_input(b, fn, "K_lo", K[256 * p0:256 * p1], pad)
    hi = k_input(b, fn, "K_hi", K[256 * (strips - p1):256 * (strips - p0)], pad)
    q = b.inp(fn, "q", qvec(n, seed))
    k2 = f64(b, fn, "ksd2_partial", 1)
    y = f64(b, fn, "y_partial", 1 << n)
    ws = b.ws(fn, "workspace", b.size("bornvi_stein_quadform_sym_workspace_bytes", n))
    return lo, hi, p0, p1, q, k2, y, ws


@family("stein_quadform_sym_pairs", ["bornvi_stein_quadform_sym_pairs"], [9, 11])
def _quadform_sym_pairs(b, n, seed):
    fn = "bornvi_stein_quadform_sym_pairs"
    lo, hi, p0, p1, q, k2, y, ws = sym_pairs_case(b, fn, n, 0, seed)
    b.call(fn, n, lo, hi, p0, p1, q, k2, y, ws, ws.nbytes)


@family("stein_quadform_sym_pairs_ld", ["bornvi_stein_quadform_sym_pairs_ld"], [(9, 32), (11, 0), (11, 32)])
def _quadform_sym_pairs_ld(b, shape, seed):
    n, pad = shape
    fn = "bornvi_stein_quadform_sym_pairs_ld"
    lo, hi, p0, p1, q, k2, y, ws = sym_pairs_case(b, fn, n, pad, seed)
    b.call(fn, n, lo, hi, (1 << n) + pad, p0, p1, q, k2, y, ws, ws.nbytes)


@family("stein_quadform_rows", ["bornvi_stein_quadform_rows"], DENSE_N)
def _quadform_rows(b, n, seed):
    fn = "bornvi_stein_quadform_rows"
    r0, r1 = row_range(n)
    K = b.inp(fn, "K_rows", sym_matrix(n, seed)[r0:r1])
    q = b.inp(fn, "q", qvec(n, seed))
    y = f64(b, fn, "y_rows", r1 - r0)
    k2 = f64(b, fn, "ksd2_partial", 1)
    ws = b.ws(fn, "workspace", b.size("bornvi_stein_quadform_workspace_bytes", n, 1))
    b.call(fn, n, K, r0, r1, q, y, k2, ws, ws.nbytes)


# bornvi_stein_matvec_kron (api.hip): gate [8] at +0 and the packed states (kron_pack_kernel writes both), the circuit engine's
#   ping-pong buffers behind them (each pass writes what the next reads), partials [kron_partials(n)] written by the combine
#   kernel's workgroups before its finishing step adds them.
@family("stein_matvec_kron", ["bornvi_stein_matvec_kron"], [2, 12, 14])
def _matvec_kron(b, n, seed):
    fn = "bornvi_stein_matvec_kron"
    S = b.inp(fn, "S", scores(n, seed))
    q = b.inp(fn, "q", qvec(n, seed))
    y = f64(b, fn, "y", 1 << n)
    k2 = f64(b, fn, "ksd2", 1)
    ws = b.ws(fn, "workspace", b.size("bornvi_stein_matvec_kron_workspace_bytes", n))
    b.call(fn, n, 0.7, S, q, y, k2, ws, ws.nbytes)


@family("ksd_grad_finish", ["bornvi_ksd_grad_finish"], [(2, 1), (3, 2), (12, 5)])
def _ksd_grad_finish(b, shape, seed):
    n, ns = shape
    fn, r = "bornvi_ksd_grad_finish", rng_for(seed, n, ns)
    sh = b.inp(fn, "shifted", r.dirichlet(np.ones(1 << n), 2 * ns))
    y = b.inp(fn, "y", r.standard_normal(1 << n))
    k2 = b.inp(fn, "ksd2", np.array([2.5]))
    lo = f64(b, fn, "loss_out", 1)
    dl = f64(b, fn, "dLdq_out", 1 << n)
    g = f64(b, fn, "grad", ns)
    b.call(fn, n, sh, ns, y, k2, lo, dl, g)


# ---- table family -------------------------------------------------------------------------------------------------------
TABLE_SHAPES = [(n, rows) for n in (1, 6, 11, 14) for rows in (1, 3)]


# bornvi_shots_histogram (kernels_shots.hip), per level l >= 1 (only n > 12 has one): masses [B][len_l] written by the mass
#   kernel of the level below, read by the next mass kernel and the level's draw; counts [B][len_l] written by the level's draw,
#   read (as the number of draws) by the draw of the level below.
@family("shots_histogram", ["bornvi_shots_histogram"], TABLE_SHAPES)
def _shots(b, shape, seed):
    n, B = shape
    fn = "bornvi_shots_histogram"
    pr = b.inp(fn, "probs", qvec(n, seed, B))
    fr = f64(b, fn, "freq", B << n)
    ep = b.inp(fn, "epoch_dev", np.array([5 + seed], np.int64))
    ws = b.ws(fn, "workspace", b.size("bornvi_shots_workspace_bytes", n, B))
    b.call(fn, n, B, pr, fr, 1000, 99 + seed, ep, 1, 1, 2, ws, ws.nbytes)


# bornvi_born_table_probs / _vjp (kernels_born_table.hip): part [rows][G][2] written by the stats kernel, read by the second kernel;
#   hpart [rows][G] (entropy given) written by the second kernel, read by the entropy kernel.  Each call fills what it reads.
@family("born_table_probs", ["bornvi_born_table_probs"], [(0, 1)] + TABLE_SHAPES)
def _born_table_probs(b, shape, seed):
    n, rows = shape
    fn = "bornvi_born_table_probs"
    w = b.inp(fn, "w", rng_for(seed, n, rows).standard_normal((rows, 1 << n)).astype(np.float32))
    q32 = b.out(fn, "q32", np.float32, rows << n)
    q64 = f64(b, fn, "q64", rows << n)
    H = b.out(fn, "entropy", np.float32, rows)
    ws = b.ws(fn, "workspace", b.size("bornvi_born_table_workspace_bytes", n, rows))
    b.call(fn, n, rows, seed % 2, w, q32, q64, H, ws, ws.nbytes)


@family("born_table_vjp", ["bornvi_born_table_vjp"], [(0, 1)] + TABLE_SHAPES)
def _born_table_vjp(b, shape, seed):
    n, rows = shape
    fn, r = "bornvi_born_table_vjp", rng_for(seed, n, rows)
    w32 = r.standard_normal((rows, 1 << n)).astype(np.float32)
    e = np.exp(w32 - w32.max(axis=1, keepdims=True))
    q = (e / e.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    w = b.inp(fn, "w", w32)
    q64 = b.inp(fn, "q64", q)
    y = b.inp(fn, "y", r.standard_normal((rows, 1 << n)))
    k2 = b.inp(fn, "ksd2", r.uniform(0.5, 2.0, rows))
    g = b.out(fn, "grad", np.float32, rows << n)
    lo = f64(b, fn, "loss_out", rows)
    ws = b.ws(fn, "workspace", b.size("bornvi_born_table_workspace_bytes", n, rows))
    b.call(fn, n, rows, 0, w, q64, y, k2, 0.1, g, lo, ws, ws.nbytes)


# bornvi_reinforce_step (kernels_reinforce.hip): scalars at +0 (scatter kernel's workgroup 0 writes all four, finish and loss kernels
#   read), part [2 G] (stats kernel writes, scatter reads), lpart [Gz] (finish writes, loss reads).  dLdq doubles as the integer
#   accumulator: zeroed by the stats kernel.
@family("reinforce_step", ["bornvi_reinforce_step"], [(1, 1), (6, 5), (11, 1000), (14, 4099)])
def _reinforce(b, shape, seed):
    n, B = shape
    fn, r, N = "bornvi_reinforce_step", rng_for(seed, n, B), 1 << n
    ix = r.integers(0, N, B, dtype=np.int64)
    if B > 1:
        ix[B // 2] = N + 3          # out of range: "is not dereferenced" (log_p[N + 3] would be margin bytes that differ by run)
        ix[B - 1] = -2
    idx = b.inp(fn, "idx", ix)
    lg = b.inp(fn, "logit", r.standard_normal(B).astype(np.float32))
    lp = b.inp(fn, "log_p", (-r.uniform(0.1, 5.0, N)).astype(np.float32))
    q = b.inp(fn, "q32", r.dirichlet(np.ones(N)).astype(np.float32))
    bl = b.inp(fn, "baseline", np.array([0.25]))
    dl = f64(b, fn, "dLdq", N)
    lo = b.out(fn, "loss", np.float32, 1)
    fi = b.out(fn, "found_inf", np.float32, 1)
    ws = b.ws(fn, "workspace", b.size("bornvi_reinforce_workspace_bytes", n, B))
    b.call(fn, n, B, idx, lg, lp, q, bl, 0, 0.9, 0.01, 1e-10, dl, lo, fi, ws, ws.nbytes)


# bornvi_elbo_weights (kernels_elbo.hip): part [rows][G][2] written by the weights kernel, read by the finishing kernel.
@family("elbo_weights", ["bornvi_elbo_weights"], TABLE_SHAPES)
def _elbo(b, shape, seed):
    n, rows = shape
    fn, r = "bornvi_elbo_weights", rng_for(seed, n, rows)
    q = b.inp(fn, "q", qvec(n, seed, rows))
    lp = b.inp(fn, "log_p", -r.uniform(0.1, 9.0, 1 << n))
    w = f64(b, fn, "w", rows << n)
    ne = f64(b, fn, "neg_elbo", rows)
    H = f64(b, fn, "entropy", rows)
    ws = b.ws(fn, "workspace", b.size("bornvi_elbo_workspace_bytes", n, rows))
    b.call(fn, n, rows, q, lp, 1e-10, w, ne, H, ws, ws.nbytes)


# ---- enumerated MPS -----------------------------------------------------------------------------------------------------
# bornvi_mps_probs -> bornvi_mps_vjp (kernels_mps.hip: MpsLayout): the levels of the prefix-doubling sweep, psi and the Z partials
#   are written by the probs call's sweep and finishing kernels, and read by the vjp; the vjp's own partials (sum q g, the core
#   gradients' prefix sums) are written by its sweep kernels before its finishing step reads them.
@family("mps_probs_vjp", ["bornvi_mps_probs", "bornvi_mps_vjp"], [(1, 1), (5, 3), (11, 5), (12, 8), (13, 32)])
def _mps(b, shape, seed):
    from test_gpu_mps_kernel import make_inputs
    n, D = shape
    f0, f1 = "bornvi_mps_probs", "bornvi_mps_vjp"
    cores, g = make_inputs(n, D, seed)
    c = b.inp(f0, "cores", cores.numpy())
    q64 = f64(b, f0, "q64", 1 << n)
    q32 = b.out(f0, "q32", np.float32, 1 << n)
    psi = f64(b, f0, "psi", 1 << n)
    Z = f64(b, f0, "Z_out", 1)
    ws = b.ws(f0, "workspace", b.size("bornvi_mps_workspace_bytes", n, D))
    gg = b.inp(f1, "g", g.numpy())
    gc = f64(b, f1, "grad_cores", n * 2 * D * D)
    b.call(f0, n, D, c, q64, q32, psi, Z, ws, ws.nbytes)
    b.call(f1, n, D, c, gg, gc, ws, ws.nbytes)


# ---- sampled MPS --------------------------------------------------------------------------------------------------------
# The (n, D, B) workspace (kernels_mps_sample.hip: MsLayout):
#   hdr (log Z, E_0[0,0], eE[0]), E, L [n + 1][D][D], eE, eL [n + 1] int   bornvi_mps_environments writes all; every later call reads
#   r [G][n][64][DS], er [G][n][64] int     the score kernels' right sweep writes a slot before their left sweep reads it
#   parts [G][n][2][D][D], wpart [256]      score_vjp's first launch writes (every workgroup its slice), its finish reads; the jvp
#                                           writes the first n doubles of wpart (mps_jvp_dot_kernel) before its sweep reads them
#   mu [n][2][D][D]                         mps_score_mu_kernel writes (score_rows, sample_gram, jvp), the same call's kernels read
# The exponents are integers used as powers of two only: never as an index.
SAMPLED_SHAPES = [(1, 1, 2), (3, 17, 65), (12, 16, 64), (63, 4, 257), (2, 32, 257)]


def sampled_cores(n, D, seed):
    from test_gpu_mps_sampled_kernel import make_cores
    return make_cores(n, D, seed).numpy()


def environments(b, n, D, B, seed, log_Z=True):
    fn = "bornvi_mps_environments"
    c = b.inp(fn, "cores", sampled_cores(n, D, seed))
    ws = b.ws(fn, "workspace", b.size("bornvi_mps_sample_workspace_bytes", n, D, B), name="env_workspace")
    lz = f64(b, fn, "log_Z_out", 1) if log_Z else None
    b.call(fn, n, D, B, c, lz, ws, ws.nbytes)
    return c, ws


@family("mps_environments", ["bornvi_mps_environments"], SAMPLED_SHAPES)
def _environments(b, shape, seed):
    environments(b, *shape, seed)


@family("mps_sample", ["bornvi_mps_environments", "bornvi_mps_sample"], SAMPLED_SHAPES)
def _mps_sample(b, shape, seed):
    n, D, B = shape
    fn = "bornvi_mps_sample"
    c, ws = environments(b, n, D, B, seed)
    ep = b.inp(fn, "epoch_dev", np.array([7 + seed], np.int64))
    idx = b.out(fn, "idx", np.int64, B)
    lq = f64(b, fn, "logq", B)
    st = i32(b, fn, "status")
    b.call(fn, n, D, B, c, 4321 + seed, ep, idx, lq, st, ws, ws.nbytes)


@family("mps_score_vjp", ["bornvi_mps_environments", "bornvi_mps_score_vjp"], SAMPLED_SHAPES)
def _mps_score_vjp(b, shape, seed):
    n, D, B = shape
    fn, r = "bornvi_mps_score_vjp", rng_for(seed, n, D, B)
    c, ws = environments(b, n, D, B, seed, log_Z=False)
    idx = b.inp(fn, "idx", sample_idx(r, n, B))
    w = b.inp(fn, "w", r.standard_normal(B))
    lq = f64(b, fn, "logq", B)
    gc = f64(b, fn, "grad_cores", n * 2 * D * D)
    st = i32(b, fn, "status")
    b.call(fn, n, D, B, c, idx, w, lq, gc, st, ws, ws.nbytes)


def score_ld(B, which):
    p2 = 1 << max(6, (B - 1).bit_length())
    return max(64, p2) if which == 0 else 2 * p2


@family("mps_score_rows", ["bornvi_mps_environments", "bornvi_mps_score_rows"],
        [s + (k,) for s in SAMPLED_SHAPES for k in (0, 1)])
def _mps_score_rows(b, shape, seed):
    n, D, B, which = shape
    fn, r = "bornvi_mps_score_rows", rng_for(seed, n, D, B)
    ld = score_ld(B, which)                                   # 64 or the next power of two above B; and twice that
    k0, kc = (0, n) if n < 3 else (1, n - 2)                  # a strict sub-range where there is one
    c, ws = environments(b, n, D, B, seed, log_Z=False)
    idx = b.inp(fn, "idx", sample_idx(r, n, B))
    rows = f64(b, fn, "rows", kc * 2 * D * D * ld)            # exactly the range's rows: sites outside it have no memory here
    st = i32(b, fn, "status")
    b.call(fn, n, D, B, c, idx, k0, kc, ld, rows, st, ws, ws.nbytes)


@family("mps_score_sample_gram", ["bornvi_mps_environments", "bornvi_mps_score_sample_gram"], SAMPLED_SHAPES)
def _mps_sample_gram(b, shape, seed):
    n, D, B = shape
    fn, r = "bornvi_mps_score_sample_gram", rng_for(seed, n, D, B)
    c, env = environments(b, n, D, B, seed, log_Z=False)
    idx = b.inp(fn, "idx", sample_idx(r, n, B))
    T = f64(b, fn, "T", B * B)
    st = i32(b, fn, "status")
    ws = b.ws(fn, "workspace", b.size("bornvi_mps_score_sample_gram_workspace_bytes", n, D, B))
    b.call(fn, n, D, B, c, idx, T, st, env, env.nbytes, ws, ws.nbytes)


@family("mps_score_jvp", ["bornvi_mps_environments", "bornvi_mps_score_jvp"], SAMPLED_SHAPES)
def _mps_score_jvp(b, shape, seed):
    n, D, B = shape
    fn, r = "bornvi_mps_score_jvp", rng_for(seed, n, D, B)
    c, env = environments(b, n, D, B, seed, log_Z=False)
    idx = b.inp(fn, "idx", sample_idx(r, n, B))
    v = b.inp(fn, "v", r.standard_normal((n, 2, D, D)))
    t = f64(b, fn, "t", B)
    st = i32(b, fn, "status")
    b.call(fn, n, D, B, c, idx, v, 0.5, t, st, env, env.nbytes)


# bornvi_score_fisher_gram, bornvi_fisher_gram, bornvi_qfi_gram (syrk_f64.hpp): slab partials [G][tiles][T][T] written by the SYRK
#   kernel's workgroups (every (tile, slab) its block), read by the finishing launch.
GRAM_SHAPES = [(1, 1), (17, 5), (65, 9)]          # (P, n)


@family("score_fisher_gram", ["bornvi_score_fisher_gram"], [(2, 1, 2, 64), (34, 3, 65, 128), (130, 2, 300, 512), (65, 1, 64, 64)])
def _score_fisher(b, shape, seed):
    R, nb, B, ld = shape
    fn = "bornvi_score_fisher_gram"
    rows = rng_for(seed, R, nb, B).standard_normal((nb * R, ld))
    rows[:, B:] = 0.0
    x = b.inp(fn, "rows", rows)
    F = f64(b, fn, "F", nb * R * R)
    ws = b.ws(fn, "workspace", b.size("bornvi_score_fisher_workspace_bytes", R, nb, ld))
    b.call(fn, R, nb, B, ld, x, F, ws, ws.nbytes)


@family("fisher_gram", ["bornvi_fisher_gram"], GRAM_SHAPES)
def _fisher(b, shape, seed):
    P, n = shape
    fn, r = "bornvi_fisher_gram", rng_for(seed, P, n)
    sh = b.inp(fn, "shifted", r.dirichlet(np.ones(1 << n), 2 * P))
    q = b.inp(fn, "q", r.dirichlet(np.ones(1 << n)))
    F = f64(b, fn, "F", P * P)
    ws = b.ws(fn, "workspace", b.size("bornvi_fisher_workspace_bytes", n, P))
    b.call(fn, n, sh, P, q, 1e-10, F, ws, ws.nbytes)


@family("qfi_gram", ["bornvi_qfi_gram"], GRAM_SHAPES)
def _qfi(b, shape, seed):
    P, n = shape
    fn, r = "bornvi_qfi_gram", rng_for(seed, P, n)
    phi = b.inp(fn, "phi", unit_states(r, P, n))
    psi = b.inp(fn, "psi", unit_states(r, 1, n))
    Q = f64(b, fn, "Q", P * P)
    ws = b.ws(fn, "workspace", b.size("bornvi_qfi_workspace_bytes", n, P))
    b.call(fn, n, P, phi, psi, Q, ws, ws.nbytes)


# bornvi_spd_solve(_batched) (kernels_fisher.hip): the factor W [P][P] per system; the kernel copies A's upper triangle in (with the
#   damping) before it factors, and reads only what it wrote.
def spd_inputs(r, nb, P):
    a = r.standard_normal((nb, P, P))
    return a @ a.transpose(0, 2, 1) / P + np.eye(P), r.standard_normal((nb, P))


@family("spd_solve", ["bornvi_spd_solve"], [1, 17, 65])
def _spd(b, P, seed):
    fn = "bornvi_spd_solve"
    A, rhs = spd_inputs(rng_for(seed, P), 1, P)
    a = b.inp(fn, "A", A)
    bb = b.inp(fn, "b", rhs)
    x = f64(b, fn, "x", P)
    info = i32(b, fn, "info")
    ws = b.ws(fn, "workspace", b.size("bornvi_spd_solve_workspace_bytes", P))
    b.call(fn, P, a, 1e-3, bb, x, info, ws, ws.nbytes)


@family("spd_solve_batched", ["bornvi_spd_solve_batched"], [(P, nb) for P in (1, 17, 65) for nb in (1, 3)])
def _spd_batched(b, shape, seed):
    P, nb = shape
    fn = "bornvi_spd_solve_batched"
    A, rhs = spd_inputs(rng_for(seed, P, nb), nb, P)
    a = b.inp(fn, "A", A)
    bb = b.inp(fn, "b", rhs)
    x = f64(b, fn, "x", nb * P)
    info = i32(b, fn, "info", nb)
    ws = b.ws(fn, "workspace", b.size("bornvi_spd_solve_batched_workspace_bytes", P, nb))
    b.call(fn, P, nb, a, 1e-3, bb, x, info, ws, ws.nbytes)


# ---- queries (kernels_mps_query.hip: MqLayout, MqVjpLayout) ---------------------------------------------------------------
#   pairs [Q + 1][2]   the environment kernel's workgroup j writes (mass, exponent) of evidence j, slot Q the empty mask; read by
#                      the logm kernel and the clamped sampler
#   E, eE              sample_clamped: the evidence's stack, written by the environment kernel, read by the sampler
#   hdr, E, L, eE, eL  marginals: written by its own unclamped sweeps, read by the per-site kernel
#   vjp: parts [G + 1][n][2][D][D] zeroed by their own workgroup before it adds into them; stacks [G + 1][n + 1][D][D] written by a
#        query's right sweep before its left sweep reads them; wpart [G + 1]; pairs as above; all read by the two finishing launches
QUERY_SHAPES = [(1, 1), (2, 2), (3, 5), (3, 17), (12, 3), (12, 16), (33, 32), (63, 4), (63, 16), (63, 1)]     # test_gpu_mps_query_kernel.SHAPES


def evidences(r, n, Q):
    full = (1 << n) - 1
    mask = sample_idx(r, n, Q) & full
    mask[0] = 0                                                # the empty evidence
    if Q > 1:
        mask[1] = full                                         # all n sites clamped
    return mask, sample_idx(r, n, Q) & mask


@family("mps_log_marginals", ["bornvi_mps_log_marginals"], [s + (Q,) for s in QUERY_SHAPES for Q in (1, 65)])
def _log_marginals(b, shape, seed):
    n, D, Q = shape
    fn, r = "bornvi_mps_log_marginals", rng_for(seed, n, D, Q)
    mk, vl = evidences(r, n, Q)
    c = b.inp(fn, "cores", sampled_cores(n, D, seed))
    m = b.inp(fn, "mask", mk)
    v = b.inp(fn, "value", vl)
    lm = f64(b, fn, "logm", Q)
    st = i32(b, fn, "status")
    ws = b.ws(fn, "workspace", b.size("bornvi_mps_query_workspace_bytes", n, D, Q))
    b.call(fn, n, D, Q, c, m, v, lm, st, ws, ws.nbytes)


@family("mps_log_marginals_vjp", ["bornvi_mps_log_marginals_vjp"], [s + (Q,) for s in QUERY_SHAPES for Q in (1, 65)])
def _log_marginals_vjp(b, shape, seed):
    n, D, Q = shape
    fn, r = "bornvi_mps_log_marginals_vjp", rng_for(seed, n, D, Q)
    mk, vl = evidences(r, n, Q)
    c = b.inp(fn, "cores", sampled_cores(n, D, seed))
    m = b.inp(fn, "mask", mk)
    v = b.inp(fn, "value", vl)
    cc = b.inp(fn, "c", r.standard_normal(Q))
    g = f64(b, fn, "grad_cores", n * 2 * D * D)
    lm = f64(b, fn, "logm", Q)
    st = i32(b, fn, "status")
    ws = b.ws(fn, "workspace", b.size("bornvi_mps_log_marginals_vjp_workspace_bytes", n, D, Q))
    b.call(fn, n, D, Q, c, m, v, cc, g, lm, st, ws, ws.nbytes)


@family("mps_sample_clamped", ["bornvi_mps_sample_clamped"], [s + (B,) for s in QUERY_SHAPES for B in (1, 65)])
def _sample_clamped(b, shape, seed):
    n, D, B = shape
    fn, r = "bornvi_mps_sample_clamped", rng_for(seed, n, D, B)
    mk, vl = evidences(r, n, 3)
    c = b.inp(fn, "cores", sampled_cores(n, D, seed))
    m = b.inp(fn, "mask", mk[2:3])
    v = b.inp(fn, "value", vl[2:3])
    ep = b.inp(fn, "epoch_dev", np.array([11 + seed], np.int64))
    idx = b.out(fn, "idx", np.int64, B)
    lq = f64(b, fn, "logq", B)
    lm = f64(b, fn, "logm", 1)
    st = i32(b, fn, "status")
    ws = b.ws(fn, "workspace", b.size("bornvi_mps_query_workspace_bytes", n, D, 1))
    b.call(fn, n, D, B, c, m, v, 777 + seed, ep, idx, lq, lm, st, ws, ws.nbytes)


@family("mps_marginals", ["bornvi_mps_marginals"], QUERY_SHAPES)
def _marginals(b, shape, seed):
    n, D = shape
    fn = "bornvi_mps_marginals"
    c = b.inp(fn, "cores", sampled_cores(n, D, seed))
    m1 = f64(b, fn, "m1", n)
    m2 = f64(b, fn, "m2", n * n)
    ws = b.ws(fn, "workspace", b.size("bornvi_mps_query_workspace_bytes", n, D, 1))
    b.call(fn, n, D, c, m1, m2, ws, ws.nbytes)


# bornvi_mps_canonicalise (kernels_mps_canon.hip: McLayout): hdr int 0, the largest sweep count: set to 0 at the start, written at
#   the end, never read by the kernel; T [n][2][D][D]: the left sweep writes Q_k and T_n, the right sweep reads what it wrote.
@family("mps_canonicalise", ["bornvi_mps_canonicalise"], [(1, 1, 1), (3, 17, 17), (3, 17, 5), (12, 16, 16), (12, 16, 7), (63, 4, 4), (63, 4, 2)])
def _canonicalise(b, shape, seed):
    n, D, Do = shape
    fn = "bornvi_mps_canonicalise"
    c = b.inp(fn, "cores", sampled_cores(n, D, seed))
    co = f64(b, fn, "cores_out", n * 2 * Do * Do)
    nb = max(n - 1, 1)                                         # n = 1 has no bonds: one slot each that nothing may write
    sm = f64(b, fn, "schmidt", nb * D, unwritten=np.ones(8 * nb * D, bool) if n == 1 else None)
    di = f64(b, fn, "discarded", nb, unwritten=np.ones(8 * nb, bool) if n == 1 else None)
    rk = i32(b, fn, "rank", nb, unwritten=np.ones(4 * nb, bool) if n == 1 else None)
    ln = f64(b, fn, "log_norm", 1)
    st = i32(b, fn, "status")
    ws = b.ws(fn, "workspace", b.size("bornvi_mps_canon_workspace_bytes", n, D))
    b.call(fn, n, D, Do, 0.0, c, co, sm, di, rk, ln, st, ws, ws.nbytes)


# ---- CG recurrence, optimiser hand-off (no workspace) -------------------------------------------------------------------------
VEC_SHAPES = [5, 3000]          # one wave's worth, and more than one workgroup's stride


@family("cg", ["bornvi_cg_init", "bornvi_cg_step", "bornvi_cg_finish"], VEC_SHAPES)
def _cg(b, P, seed):
    f0, f1, f2 = "bornvi_cg_init", "bornvi_cg_step", "bornvi_cg_finish"
    r_ = rng_for(seed, P)
    g = b.inp(f0, "g", r_.standard_normal(P))
    x = f64(b, f0, "x", P)
    r = f64(b, f0, "r", P)
    p = f64(b, f0, "p", P)
    state = f64(b, f0, "state", 8)
    info = i32(b, f0, "info")
    Fp = b.inp(f1, "Fp", r_.standard_normal(P) * 0.01)
    info2 = i32(b, f2, "info", name="info_finish")
    iters = i32(b, f2, "iters")
    rel = f64(b, f2, "relres", 1)
    b.call(f0, P, g, x, r, p, state, info)
    b.call(f1, P, 0.5, 1e-8, Fp, x, r, p, state)
    b.call(f2, P, g, x, state, info2, iters, rel)


@family("cg_step", ["bornvi_cg_step"], [(P, done) for P in VEC_SHAPES for done in (0, 1)])
def _cg_step(b, shape, seed):
    P, done = shape
    fn, r_ = "bornvi_cg_step", rng_for(seed, P)
    g = r_.standard_normal(P)
    rr = float(g @ g)
    all_ = (lambda k: np.ones(8 * k, bool)) if done else (lambda k: None)       # done: "writes nothing"
    Fp = b.inp(fn, "Fp", r_.standard_normal(P) * 0.01)
    x = b.inp(fn, "x", np.zeros(P), unwritten=all_(P))
    r = b.inp(fn, "r", g, unwritten=all_(P))
    p = b.inp(fn, "p", g.copy(), unwritten=all_(P))
    state = b.inp(fn, "state", np.array([rr, rr, 0.0, float(done), 1.0, 0.0, 0.0, 0.0]), unwritten=all_(8))
    b.call(fn, P, 0.5, 1e-8, Fp, x, r, p, state)


@family("cg_finish", ["bornvi_cg_finish"], VEC_SHAPES)
def _cg_finish(b, P, seed):
    fn, r_ = "bornvi_cg_finish", rng_for(seed, P)
    g = b.inp(fn, "g", r_.standard_normal(P))
    x = b.inp(fn, "x", r_.standard_normal(P))
    state = b.inp(fn, "state", np.array([1e-3, 2.0, 3.0, 0.0, 0.02, 0.0, 0.0, 0.0]))
    info = i32(b, fn, "info")
    iters = i32(b, fn, "iters")
    rel = f64(b, fn, "relres", 1)
    b.call(fn, P, g, x, state, info, iters, rel)


@family("clip_cast_grad", ["bornvi_clip_cast_grad"], VEC_SHAPES)
def _clip(b, P, seed):
    fn = "bornvi_clip_cast_grad"
    g = b.inp(fn, "grad64", rng_for(seed, P).standard_normal(P))
    g32 = b.out(fn, "grad32", np.float32, P)
    tn = b.out(fn, "total_norm", np.float32, 1)
    b.call(fn, P, g, 1.0, g32, tn)


@family("clip_cast_grad_guard", ["bornvi_clip_cast_grad_guard"], VEC_SHAPES)
def _clip_guard(b, P, seed):
    fn = "bornvi_clip_cast_grad_guard"
    g = b.inp(fn, "grad64", rng_for(seed, P).standard_normal(P))
    lo = b.inp(fn, "loss", np.array([0.75]))
    g32 = b.out(fn, "grad32", np.float32, P)
    tn = b.out(fn, "total_norm", np.float32, 1)
    fi = b.out(fn, "found_inf", np.float32, 1)
    b.call(fn, P, g, 1.0, lo, g32, tn, fi)


@family("clip_adam_step", ["bornvi_clip_adam_step"], VEC_SHAPES)
def _clip_adam(b, P, seed):
    fn, r = "bornvi_clip_adam_step", rng_for(seed, P)
    n_lr, epoch = 4, 2
    one = lambda size: np.array([k != epoch for k in range(n_lr) for _ in range(size)])      # only this epoch's entry is written
    g = b.inp(fn, "grad64", r.standard_normal(P))
    lo = b.inp(fn, "loss", np.array([0.75]))
    th = b.inp(fn, "theta", r.standard_normal(P).astype(np.float32))
    g32 = b.out(fn, "grad32", np.float32, P)
    t64 = f64(b, fn, "theta64", P)
    m = b.inp(fn, "exp_avg", (0.1 * r.standard_normal(P)).astype(np.float32))
    v = b.inp(fn, "exp_avg_sq", (0.1 * r.uniform(0, 1, P)).astype(np.float32))
    cnt = b.inp(fn, "counters", np.array([epoch, epoch], np.int32))
    lr = b.inp(fn, "lr_table", np.linspace(1e-2, 1e-3, n_lr))
    tn = b.out(fn, "total_norm", np.float32, 1)
    lh = f64(b, fn, "loss_history", n_lr, unwritten=one(8))
    nh = b.out(fn, "norm_history", np.float32, n_lr, unwritten=one(4))
    b.call(fn, P, g, 1.0, lo, th, g32, t64, m, v, cnt, lr, n_lr, 0.9, 0.999, 1e-8, tn, lh, nh)
