"""ctypes binding of libbornvi_hip.so (C ABI declared in include/bornvi.h).

The HIP library is the only compute backend of this package: there is no CPU fallback.  If the
shared object is missing or a GPU entry point is called without a GPU, an exception is raised.

`import torch` happens before the library is loaded so that the process uses ONE HIP runtime
(libamdhip64.so.7 is resolved to the copy PyTorch already mapped); device memory, streams and
collectives all come from PyTorch.
"""
import ctypes as C
import os
import re

import torch  # noqa: F401  (must precede loading the HIP library, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libbornvi_hip.so"
LIB_PATH = os.environ.get("BORNVI_LIB") or os.path.join(_HERE, LIB_NAME)   # BORNVI_LIB: a tuning build of the same library

_lib = None


class BornviError(RuntimeError):
    pass


class BnDesc(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("max_parents", C.c_int32),
                ("role", C.c_void_p), ("n_parents", C.c_void_p), ("parents", C.c_void_p),
                ("cpt_off", C.c_void_p), ("cpt", C.c_void_p)]


# include/bornvi.h is the one statement of the ABI: prototypes, status and ansatz codes and every BORNVI_* limit are read
# from it.  The header keeps to a narrow subset of C (block comments, plain `#define NAME <decimal>`, two enums with
# explicit values, typedefs, declarations `ret bornvi_name(args);`), and the parser refuses what lies outside it.
_TYPES = {"int": C.c_int, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t,
          "double": C.c_double, "bornvi_handle": C.c_void_p, "bornvi_stream": C.c_void_p, "const char*": C.c_char_p,
          "const bornvi_bn_desc*": C.POINTER(BnDesc), "bornvi_handle*": C.POINTER(C.c_void_p)}


def _ctype(text, decl, is_return=False):
    t = re.sub(r"\s*\*", "*", " ".join(text.split()))
    if t in _TYPES:
        return _TYPES[t]
    if is_return and t == "void":
        return None
    if re.fullmatch(r"[\w ]+\*", t):      # every other pointer: device memory, or a host array passed by reference
        return C.c_void_p
    raise BornviError(f"bornvi.h: no ctypes mapping for type '{t}' in declaration '{' '.join(decl.split())}'")


def parse_header(text):
    """(defines, enums, prototypes) of the header text: {BORNVI_NAME: int} of the #define lines, {NAME: int} of the enums,
    {symbol: (restype, argtypes)} in declaration order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(BORNVI_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    enums = {}
    for body in re.findall(r"typedef\s+enum\s*\{(.*?)\}", text, re.S):
        enums.update((m[1], int(m[2])) for m in re.finditer(r"(\w+)\s*=\s*(-?\d+)", body))
    text = re.sub(r"typedef\s+(enum|struct)\s*\{.*?\}\s*\w+\s*;|typedef\s[^;{]*;", "", text, flags=re.S)
    protos = {}

    def declaration(m):
        args = [] if m[3].strip() == "void" else [_ctype(re.sub(r"\w+\s*$", "", a), m[0]) for a in m[3].split(",")]
        protos[m[2]] = (_ctype(m[1], m[0], is_return=True), args)
        return ""
    rest = re.sub(r"([\w \t\n*]+?)\b(bornvi_\w+)\s*\(([^()]*)\)\s*;", declaration, text)
    if "".join(rest.split()) not in ("", 'extern"C"{}'):
        raise BornviError(f"bornvi.h: text the binding cannot read: '{' '.join(rest.split())[:200]}'")
    return defines, enums, protos


HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bornvi.h")
if not os.path.exists(HEADER_PATH):
    raise BornviError(f"{HEADER_PATH} not found: the binding reads the C ABI from it")
with open(HEADER_PATH) as _f:
    LIMITS, _ENUMS, PROTOTYPES = parse_header(_f.read())      # LIMITS: every `#define BORNVI_*` integer of the header

BORNVI_OK = _ENUMS["BORNVI_OK"]
ANSATZ_IDS = {k: _ENUMS["BORNVI_ANSATZ_" + k.upper()] for k in ("hardware_efficient", "all_to_all", "basic")}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

# The side headers include/bornvi_<name>.h, each a family's own in the same subset of C: the two-site sweeps, the complex-cores
# sampled MPS, MMD with a Hamming-distance kernel, the locally purified sampled MPS, the tree tensor network.  The same parser reads each into tables of
# its own, <NAME>_HEADER_PATH, <NAME>_LIMITS and <NAME>_PROTOTYPES (LIMITS, PROTOTYPES and EXPORTED_SYMBOLS above are
# bornvi.h's alone); lib() binds every set.
_SIDE = {}
for _name in ("twosite", "cmps", "mmd", "lps", "ttn"):
    _path = os.path.join(os.path.dirname(_HERE), "include", f"bornvi_{_name}.h")
    if not os.path.exists(_path):
        raise BornviError(f"{_path} not found: the binding reads the C ABI from it")
    with open(_path) as _f:
        _limits, _, _protos = parse_header(_f.read())
    _SIDE[_name] = (_path, _limits, _protos)
TWOSITE_HEADER_PATH, TWOSITE_LIMITS, TWOSITE_PROTOTYPES = _SIDE["twosite"]
CMPS_HEADER_PATH, CMPS_LIMITS, CMPS_PROTOTYPES = _SIDE["cmps"]
MMD_HEADER_PATH, MMD_LIMITS, MMD_PROTOTYPES = _SIDE["mmd"]
LPS_HEADER_PATH, LPS_LIMITS, LPS_PROTOTYPES = _SIDE["lps"]
TTN_HEADER_PATH, TTN_LIMITS, TTN_PROTOTYPES = _SIDE["ttn"]


def lib():
    """The loaded library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BornviError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for protos in [PROTOTYPES] + [side[2] for side in _SIDE.values()]:
            for name, (res, args) in protos.items():
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
        _lib = handle
    return _lib


def plan_words(ansatz_id, n, layers, tile_bits=0):
    """Serialised execution plan (host only; no GPU needed)."""
    import numpy as np
    L = lib()
    need = L.bornvi_plan_describe(ansatz_id, n, layers, tile_bits, None, 0)
    if need < 0:
        raise BornviError("bornvi_plan_describe: unsupported configuration")
    buf = (C.c_uint32 * need)()
    L.bornvi_plan_describe(ansatz_id, n, layers, tile_bits, buf, need)
    return np.frombuffer(buf, dtype=np.uint32).copy()


def plan_param_first_pass(words):
    """First pass whose matrices depend on parameter p, read off a serialised plan (plan.hpp: PW_MATS lists the fused
    gates of every stage of a pass, a fused gate lists its parameters) -- the same rule the library applies when it
    orders a parameter-shift batch for prefix sharing (Plan::param_first_pass)."""
    import numpy as np
    W = words
    npass, nparams, off_fused, off_passtab = int(W[3]), int(W[5]), int(W[6]), int(W[7])
    first = np.full(nparams, -1, dtype=np.int64)
    for i in range(npass):
        base = int(W[off_passtab + i])
        for sm in range(int(W[base + 3]) * 4):                    # PW_NSTAGES stages x 4 register bits
            w = int(W[base + 128 + (sm >> 1)])                    # PW_MATS
            f = (w >> 16) if (sm & 1) else (w & 0xffff)
            if f == 0xffff:
                continue
            fw = W[off_fused + f * 10: off_fused + (f + 1) * 10]  # FUSED_WORDS
            for e in range(int(fw[1])):
                par = int(fw[3 + 2 * e])
                if par != 0xffffffff and par < nparams and first[par] < 0:
                    first[par] = i
    first[first < 0] = 0
    return first


def plan_fast_words(ansatz_id, n, layers, tile_bits=0):
    """Fast-path tables of a plan: (words, pass offsets), or (None, None) when the plan is not eligible."""
    import numpy as np
    L = lib()
    need = L.bornvi_plan_fast_describe(ansatz_id, n, layers, tile_bits, None, 0, None, 0)
    if need < 0:
        raise BornviError("bornvi_plan_fast_describe: unsupported configuration")
    if need == 0:
        return None, None
    npass = int(plan_words(ansatz_id, n, layers, tile_bits)[3])
    buf = (C.c_uint32 * need)()
    offs = (C.c_uint32 * npass)()
    L.bornvi_plan_fast_describe(ansatz_id, n, layers, tile_bits, buf, need, offs, npass)
    return np.frombuffer(buf, dtype=np.uint32).copy(), np.frombuffer(offs, dtype=np.uint32).copy()


R3 = 0x200     # flag in `tile_bits` of the plan_* helpers: the 3-register-wire plan (8 amplitudes per thread)


def plan_compact_words(ansatz_id, n, layers, tile_bits=0):
    """Compact tables of the 3-register-wire plan (plan.hpp: CompactTables): (words, pass offsets) or (None, None) when the
    plan is not eligible for circuit_pass_r3_kernel.  The library checks every word against its point evaluation."""
    import numpy as np
    L = lib()
    need = L.bornvi_plan_compact_describe(ansatz_id, n, layers, tile_bits, None, 0, None, 0)
    if need < 0:
        raise BornviError("bornvi_plan_compact_describe: unsupported configuration")
    if need == 0:
        return None, None
    npass = int(plan_words(ansatz_id, n, layers, tile_bits | R3)[3])
    buf = (C.c_uint32 * need)()
    offs = (C.c_uint32 * npass)()
    L.bornvi_plan_compact_describe(ansatz_id, n, layers, tile_bits, buf, need, offs, npass)
    return np.frombuffer(buf, dtype=np.uint32).copy(), np.frombuffer(offs, dtype=np.uint32).copy()


class Handle:
    """One bornvi handle per device; thin checked wrappers around the C ABI."""

    def __init__(self, device_index=0):
        self._lib = lib()
        h = C.c_void_p()
        rc = self._lib.bornvi_create(int(device_index), C.byref(h))
        if rc != BORNVI_OK:
            raise BornviError(f"bornvi_create failed ({rc}): {self._lib.bornvi_last_error(None).decode()}")
        self.h = h
        self.device_index = int(device_index)

    def close(self):
        if getattr(self, "h", None):
            self._lib.bornvi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, what):
        if rc != BORNVI_OK:
            raise BornviError(f"{what} failed ({rc}): {self._lib.bornvi_last_error(self.h).decode()}")

    def call(self, name, *args):
        self.check(getattr(self._lib, name)(self.h, *args), name)

    def size(self, name, *args):
        v = getattr(self._lib, name)(self.h, *args)
        if v == 0:
            raise BornviError(f"{name} returned 0: {self._lib.bornvi_last_error(self.h).decode()}")
        return int(v)


_handles = {}


def handle_for(device):
    """Cached handle for a torch.device (must be a 'cuda' device: PyTorch-ROCm's spelling)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise BornviError(f"the bornvi backend runs on MI355X only; got device '{dev}' (no CPU fallback)")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _handles:
        _handles[idx] = Handle(idx)
    return _handles[idx]


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
