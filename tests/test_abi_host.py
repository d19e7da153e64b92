"""Host tests of the header-derived ctypes binding (seq2seq_vc_amd/_abi.py): the parser on the real header and on small synthetic
texts, and the derived struct layouts against what the C compiler makes of the same header.  No GPU."""
import ctypes
import keyword
import os
import subprocess

import pytest

import abi_header
from seq2seq_vc_amd import _abi, _lib

C_NAMES = ["s2svc_operand", "s2svc_gemm_desc", "s2svc_colreduce_item", "s2svc_scalar_terms", "s2svc_gather3_job", "s2svc_derived_job",
           "s2svc_conv1d_wgrad_item"]


def test_parser_reads_every_declaration_of_the_real_header():
    functions, structs = _abi.read_header()
    # a declaration the parser dropped would be a name the plain regular expression finds and the parser does not
    assert set(functions) == abi_header.declared() and len(functions) > 170
    assert sorted(functions) == _lib.exported_symbols() and functions.keys() == _lib._FUNCTIONS.keys()
    L = abi_header.library()
    for name, (restype, argtypes) in functions.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert list(structs) == [_abi.class_name(n) for n in C_NAMES]
    assert all(getattr(_lib, n) is _lib._STRUCTS[n] for n in structs)
    assert functions["s2svc_last_error"] == (ctypes.c_char_p, []) and functions["s2svc_abi_version"] == (ctypes.c_int, [])
    assert functions["s2svc_mas_ws_bytes"] == (ctypes.c_int64, [ctypes.c_int32] * 3)
    assert functions["s2svc_gemm"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    assert [f for f, _ in _lib.Gather3Job._fields_][:2] == ["in_", "out"]


SYNTHETIC = """
/* a comment with a declaration inside: int foo(int a, int b); and a struct: typedef struct { int x; } s2svc_ghost; */
#ifndef H
#define H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
// int bar(int a);
enum { S2SVC_A = 0, /* , ( ; */ S2SVC_B = 1 };
#define S2SVC_N 3
typedef struct { const void* p; int32_t a, b; int64_t c; } s2svc_inner;
typedef struct s2svc_outer {
  s2svc_inner A, B;                 /* nested */
  const float* x[S2SVC_N];          /* array of pointers, bound from a #define */
  float w[2];
  const void* in;
  uint64_t seed;
  double g;
} s2svc_outer;
int s2svc_f(void** out /* host */, const uint64_t* p, const s2svc_outer* d /* host; x[] are (outputs), with commas */, double g,
            uint64_t seed, float a, int64_t n, int32_t m, int k);
int64_t s2svc_bytes(int n);
const char* s2svc_msg(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    functions, structs = _abi.parse(SYNTHETIC)
    assert list(functions) == ["s2svc_f", "s2svc_bytes", "s2svc_msg"]            # nothing from the comments
    assert functions["s2svc_f"] == (ctypes.c_int, [vp, vp, vp, ctypes.c_double, ctypes.c_uint64, ctypes.c_float, ctypes.c_int64, i32, i32])
    assert functions["s2svc_bytes"] == (ctypes.c_int64, [i32]) and functions["s2svc_msg"] == (ctypes.c_char_p, [])
    assert list(structs) == ["Inner", "Outer"]
    inner, outer = structs["Inner"], structs["Outer"]
    assert inner._fields_ == [("p", vp), ("a", i32), ("b", i32), ("c", ctypes.c_int64)] and ctypes.sizeof(inner) == 24
    assert [f for f, _ in outer._fields_] == ["A", "B", "x", "w", "in_", "seed", "g"]
    kinds = dict(outer._fields_)
    assert kinds["A"] is inner and kinds["B"] is inner and outer.B.offset == 24
    assert kinds["x"]._type_ is vp and kinds["x"]._length_ == 3 and kinds["w"]._type_ is ctypes.c_float and kinds["w"]._length_ == 2
    assert kinds["seed"] is ctypes.c_uint64 and kinds["g"] is ctypes.c_double and ctypes.sizeof(outer) == 48 + 24 + 8 + 8 + 8 + 8


STRUCT = "typedef struct { int a; } s2svc_s;\n"


@pytest.mark.parametrize("text,named", [
    ("int s2svc_f(size_t n);", "int s2svc_f(size_t n)"),                                   # unknown scalar type
    (STRUCT + "int s2svc_g(s2svc_s item);", "int s2svc_g(s2svc_s item)"),                  # a struct passed by value
    ("int s2svc_h(int (*cb)(int, int), void* stream);", "int s2svc_h(int (*cb)(int, int), void* stream)"),   # a function pointer
    ("int s2svc_ok(int n);\nint s2svc_i(int n)\n", "int s2svc_i(int n)"),                  # an unterminated declaration
    ("void s2svc_j(int n);", "void s2svc_j(int n)"),                                       # a return type outside the ABI's three
    ("int s2svc_k(unsigned int n);", "int s2svc_k(unsigned int n)"),
    ("typedef struct { size_t n; } s2svc_t;", "size_t n"),
    ("typedef struct { float w[S2SVC_UNDEFINED]; } s2svc_u;", "float w[S2SVC_UNDEFINED]"),
    ("typedef struct { union { int a; float b; } u; } s2svc_v;", "union"),
    ("static inline int s2svc_l(int n) { return n; }", "s2svc_l"),
    ("#pragma pack(1)\nint s2svc_m(int n);", "#pragma pack(1)"),
], ids=["size_t", "by_value", "function_pointer", "unterminated", "void_return", "two_word_type", "field_type", "array_bound", "union",
        "definition", "pragma"])
def test_parser_refuses_what_it_does_not_understand(text, named):
    with pytest.raises(_abi.AbiError) as e:
        _abi.parse(text)
    assert named in str(e.value)


def test_missing_header_raises():
    with pytest.raises(OSError):
        _abi.read_header(os.path.join(abi_header.ROOT, "include", "no_such_header.h"))


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    """The header compiled AS C by the host compiler: sizeof of every ABI struct and offsetof of every field against the derived
    ctypes classes (a field of the wrong width, a missed field or a wrong array bound moves everything behind it)."""
    structs = _lib._STRUCTS
    assert list(structs) == [_abi.class_name(n) for n in C_NAMES]
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{os.path.join(abi_header.ROOT, "include", "s2svc_hip.h")}"',
             "int main(void) {"]
    expected = []
    for c_name, cls in zip(C_NAMES, structs.values()):
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        expected.append(f"{c_name} {ctypes.sizeof(cls)}")
        for field, _ in cls._fields_:
            c_field = field[:-1] if keyword.iskeyword(field[:-1]) else field             # in_ is C's `in`
            lines.append(f'  printf("{c_name}.{c_field} %zu\\n", offsetof({c_name}, {c_field}));')
            expected.append(f"{c_name}.{c_field} {getattr(cls, field).offset}")
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-x", "c", "-std=c99", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert out == expected
    assert [ctypes.sizeof(c) for c in structs.values()] == [80, 392, 88, 136, 64, 72, 56]
    assert len(expected) == 7 + sum(len(c._fields_) for c in structs.values()) == 7 + 110
