"""ctypes binding of libfiber_hip.so (the C ABI declared in include/fiber_hip.h).

PyTorch is plumbing only: tensors provide device memory (``data_ptr()``) and the current HIP stream.  There is no
CPU or eager fallback -- if the shared library is missing or a tensor is not on a HIP device the call raises.
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FIBER_HIP_LIB") or os.path.join(_HERE, "libfiber_hip.so")   # env: A/B builds (tools/)

P, I, F, L, U64, DBL = C.c_void_p, C.c_int, C.c_float, C.c_long, C.c_uint64, C.c_double

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fiber_hip.h")                 # the one statement of the C ABI

# C parameter type (without const) -> ctypes; anything with a `*` is a pointer.  Everything else is refused, never guessed.
_SCALAR = {"int": I, "long": L, "long long": C.c_longlong, "unsigned": C.c_uint, "unsigned int": C.c_uint, "uint64_t": U64,
           "unsigned long long": U64, "float": F, "double": DBL}
_RETURN = {"int": I, "long": L}
_STREAM = "fiber_stream_t"


class FiberHipError(RuntimeError):
    pass


def _param(p, proto):
    """ctypes type of one named parameter of `proto`."""
    if re.search(r"[()\[\]]", p):
        raise FiberHipError(f"fiber_hip.h: function-pointer or array parameter '{p}' in: {proto}")
    if "*" in p:
        return P
    words = [w for w in p.split() if w != "const"]
    ctype = _SCALAR.get(" ".join(words[:-1]))
    if ctype is None or any(words[-1] in t.split() for t in _SCALAR):
        raise FiberHipError(f"fiber_hip.h: no ctypes mapping for parameter '{p}' (each needs a known type and a name) in: {proto}")
    return ctype


def parse_header(text):
    """(signatures, plain, restypes, defines) of the declarations in `text`, which is C in the narrow subset fiber_hip.h keeps:
    comments, preprocessor lines, one `<ret> fiber_<name>(<named params>);` per entry point and `#define FIBER_<NAME> <int>`.
    A prototype whose last parameter is the stream is a call() entry (argument types listed without the stream), one without a
    stream a plain() helper.  Raises FiberHipError naming the prototype for anything outside that subset."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(FIBER_\w+)[ \t]+(.*\S)[ \t]*$", text, flags=re.M):
        try:
            defines[name] = int(value, 0)
        except ValueError:
            raise FiberHipError(f"fiber_hip.h: #define {name} {value} is not an integer literal") from None
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', " ", text, flags=re.M)
    signatures, plain, restypes = {}, {}, {}
    for stmt in text.split(";"):
        if not re.search(r"\bfiber_\w+\s*\(", stmt):
            continue
        proto = " ".join(stmt.split())
        m = re.fullmatch(r"(.*?)\b(fiber_\w+) ?\((.*)\)", proto)
        if m is None:
            raise FiberHipError(f"fiber_hip.h: cannot split the declaration: {proto}")
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret not in _RETURN:
            raise FiberHipError(f"fiber_hip.h: no ctypes mapping for return type '{ret}' in: {proto}")
        params = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
        has_stream = bool(params) and params[-1].split()[:1] == [_STREAM] and "*" not in params[-1]
        if has_stream:
            params.pop()
        if any(_STREAM in p for p in params):
            raise FiberHipError(f"fiber_hip.h: the stream must be the last parameter, by value, in: {proto}")
        (signatures if has_stream else plain)[name] = [_param(p, proto) for p in params]
        restypes[name] = _RETURN[ret]
    return signatures, plain, restypes, defines


def read_header(path=HEADER_PATH):
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise FiberHipError(f"C ABI header {path} not readable ({e.strerror}); the binding is derived from it") from None


# name -> argtypes without the stream (call() appends it); name -> argtypes of the helpers without a stream; name -> restype;
# the header's FIBER_<NAME> integer constants (return codes, FIBER_DOT_PARTS, the act bits of fiber_gemm_nt_bf16).  Read once, here:
# tools index these tables before (or without) load().
SIGNATURES, PLAIN, RESTYPES, DEFINES = read_header()
_RC_TEXT = {DEFINES["FIBER_EINVAL"]: "invalid argument", DEFINES["FIBER_ELAUNCH"]: "launch failure"}
_lib = None


def load():
    """Load libfiber_hip.so and declare every prototype.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise FiberHipError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "or `make -C fiber_amd/csrc` (there is no fallback path)")
    lib = C.CDLL(LIB_PATH)
    for name, restype in RESTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = SIGNATURES[name] + [P] if name in SIGNATURES else PLAIN[name]
        fn.restype = restype
    _lib = lib
    return lib


def exported_symbols():
    return list(SIGNATURES) + list(PLAIN)


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses anything that is not contiguous HIP memory."""
    if t is None:
        return None
    if not t.is_cuda:
        raise FiberHipError("fiber_amd ops need HIP device tensors (no CPU fallback)")
    return t.data_ptr()


_TRACE = [] if os.environ.get("FIBER_TRACE_LAUNCHES") else None     # debug: (stream, entry point, scalar args, event after launch)


def call(name, *args):
    lib = load()
    cur = torch.cuda.current_stream()
    stream = cur.cuda_stream
    rc = getattr(lib, name)(*args, stream)
    if _TRACE is not None:
        ev = torch.cuda.Event()
        ev.record(cur)
        _TRACE.append((stream, name, [a for a in args if isinstance(a, (int, float))], ev))
        del _TRACE[:-4000]
    if rc != DEFINES["FIBER_OK"]:
        raise FiberHipError(f"{name} failed with code {rc} ({_RC_TEXT.get(rc, '?')})")


def plain(name, *args):
    return getattr(load(), name)(*args)
