"""The C ABI is stated once, in include/fiber_hip.h: the ctypes binding is derived from it and the compiler checks every
definition against it.  Host tests: no GPU."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

from fiber_amd import lib
from fiber_amd.lib import DBL, F, I, L, P, U64, FiberHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Rows of the hand-written tables this binding replaced, which together use every type token of the header.
CALL_ROWS = {
    "fiber_gemm_nt_bf16": [P, P, P, P, P, P, P, I, P, I, P, I, I, I, I, I, I, I, I],
    "fiber_stream_add": [P, I, P, P, P, P, L, F, U64, F, U64, P, P, P, L],
    "fiber_ground_recall": [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, DBL, I],
    "fiber_mlm_mask_i64": [P, P, P, L, U64, C.c_uint, I, I, I, I],
    "fiber_ap_accumulate": [P, P, P, P, P, P, P, C.c_longlong, I, I, I, I],
}
PLAIN_ROWS = {                                   # name -> (argtypes, restype)
    "fiber_adamw_chunk": ([], I),
    "fiber_dcn_dx_workspace": ([I, I, I, I, I, I, I], L),
    "fiber_atss_num_candidates": ([P, I, I], I),
}


def test_derived_rows_equal_the_hand_written_ones():
    l = lib.load()
    for name, row in CALL_ROWS.items():
        assert lib.SIGNATURES[name] == row and name not in lib.PLAIN, name
        assert getattr(l, name).argtypes == row + [P] and getattr(l, name).restype is I, name
    for name, (row, restype) in PLAIN_ROWS.items():
        assert lib.PLAIN[name] == row and name not in lib.SIGNATURES, name
        assert getattr(l, name).argtypes == row and getattr(l, name).restype is restype, name
    assert len(lib.SIGNATURES) + len(lib.PLAIN) == len(lib.RESTYPES) == len(set(lib.exported_symbols()))


def test_every_type_token_maps_by_name():
    """c_long and c_longlong (c_uint64 and c_ulonglong) are one class on LP64, so the rows above cannot tell `long` from
    `long long`: pin the mapping token by token, with const and pointers of each."""
    sig, plain, restypes, defines = lib.parse_header(
        "#define FIBER_A 0x10\n#define FIBER_B 7 /* seven */\n#define FIBER_HIP_H\n"
        "int fiber_t(int a, long b, long long c, unsigned d, unsigned int e, uint64_t f, unsigned long long g, float h, double i,\n"
        "            const long long* p, unsigned char* q, const void* r, const int n, fiber_stream_t stream);\n"
        "long fiber_u(void); // a helper\nint fiber_v();\n")
    assert sig == {"fiber_t": [C.c_int, C.c_long, C.c_longlong, C.c_uint, C.c_uint, C.c_uint64, C.c_uint64, C.c_float, C.c_double,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]}
    assert [C.sizeof(t) for t in sig["fiber_t"][:9]] == [4, 8, 8, 4, 4, 8, 8, 4, 8]
    assert plain == {"fiber_u": [], "fiber_v": []}
    assert restypes == {"fiber_t": C.c_int, "fiber_u": C.c_long, "fiber_v": C.c_int}
    assert defines == {"FIBER_A": 16, "FIBER_B": 7}


def test_shared_constants_come_from_the_header():
    from fiber_amd import ops
    want = {"FIBER_OK": 0, "FIBER_EINVAL": 1, "FIBER_ELAUNCH": 2, "FIBER_DOT_PARTS": 512, "FIBER_ACT_GELU": 1, "FIBER_ACT_GELU_BWD": 2,
            "FIBER_ACT_OUT_F32": 0x100, "FIBER_ACT_STREAM_F32": 0x800, "FIBER_ACT_TRACE": 0x1000, "FIBER_ACT_NT_STORES": 0x2000,
            "FIBER_ACT_KEEP_STAGGER": 0x4000}
    assert lib.DEFINES == want
    assert ops._DOT_PARTS == 512 and (ops.ACT_GELU, ops.ACT_GELU_BWD, ops.ACT_OUT_F32, ops.ACT_STREAM_F32) == (1, 2, 0x100, 0x800)
    common = open(os.path.join(ROOT, "fiber_amd", "csrc", "common.h")).read()
    assert not [n for n in want if f"#define {n} " in common]


def _exported_fiber_functions(path):
    """Names of the defined global functions fiber_* in the dynamic symbol table of an ELF64 little-endian shared object."""
    d = open(path, "rb").read()
    assert d[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    dynsym = next(s for s in secs if s[1] == 11)                      # SHT_DYNSYM; s[4] offset, s[5] size, s[6] link = its string table
    names = secs[dynsym[6]][4]
    out = set()
    for off in range(dynsym[4], dynsym[4] + dynsym[5], 24):
        st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", d, off)
        if st_shndx != 0 and st_info & 0xF == 2 and st_info >> 4 in (1, 2):   # defined, STT_FUNC, global or weak
            s = d[names + st_name:d.index(b"\0", names + st_name)].decode()
            if s.startswith("fiber_"):
                out.add(s)
    return out


def test_parsed_prototypes_are_the_exported_functions():
    lib.load()
    exported = _exported_fiber_functions(lib.LIB_PATH)
    assert set(lib.RESTYPES) == exported, set(lib.RESTYPES) ^ exported


@pytest.mark.parametrize("name, text", [
    ("fiber_a", "int fiber_ok(int n, fiber_stream_t stream);\nint fiber_a(const void* x, size_t n, fiber_stream_t stream);"),
    ("fiber_b", "typedef struct { int a; } box_t;\nint fiber_b(box_t box, fiber_stream_t stream);"),
    ("fiber_b", "int fiber_b(struct box b);"),
    ("fiber_c", "int fiber_c(const void* x, fiber_stream_t stream, int n);"),
    ("fiber_d", "double fiber_d(int n);"),
    ("fiber_e", "int fiber_e(void (*done)(int), fiber_stream_t stream);"),
    ("fiber_f", "int fiber_f(int, long long);"),
    ("fiber_g", "static inline int fiber_g(int n) { return n; }"),
    ("fiber_h", "int fiber_h(int n, fiber_stream_t* stream);"),
])
def test_reader_refuses_what_it_cannot_map(name, text):
    with pytest.raises(FiberHipError, match=name + r"\b"):
        lib.parse_header(text)


def test_reader_refuses_a_define_that_is_no_integer():
    with pytest.raises(FiberHipError, match="FIBER_N"):
        lib.parse_header("#define FIBER_N (1 << 4)\n")


def test_missing_header_raises_with_its_path(tmp_path):
    path = str(tmp_path / "nowhere" / "fiber_hip.h")
    with pytest.raises(FiberHipError, match="nowhere"):
        lib.read_header(path)


def test_compiler_checks_definitions_against_the_header(tmp_path):
    """A definition that drifts from its declaration no longer compiles: common.h includes the header."""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc here")
    tu = tmp_path / "drift.hip"
    tu.write_text('#include "%s"\n'
                  'extern "C" long fiber_gemm_row_tile(int, int, int) { return 0; }\n'
                  % os.path.join(ROOT, "fiber_amd", "csrc", "common.h"))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", str(tu)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "conflicting types for 'fiber_gemm_row_tile'" in r.stderr, r.stderr[-2000:]
