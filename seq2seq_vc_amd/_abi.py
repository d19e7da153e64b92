"""The ctypes view of the C ABI, read from include/s2svc_hip.h: the header is the only place where an entry point's arguments or a
struct's fields are written down.  `parse` understands the whole text it is given or raises AbiError naming the declaration it could
not read; it never guesses and never skips, because a wrong argument list here is a kernel launched with a garbage pointer."""
import ctypes
import keyword
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "s2svc_hip.h")
SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double}
RESTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}     # and `const char*` -> c_char_p

_PREPROCESSOR = re.compile(r"#\s*(?:(?:ifndef|ifdef|include)\s+\S+|endif|define\s+(\w+)(?:\s+(\d+))?)")
_DECLARATION = re.compile(r"((?:[^;{}]|\{[^{}]*\})*);")
_ENUM = re.compile(r"enum\s*\w*\s*\{[^{}]*\}")
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)")
_FUNCTION = re.compile(r"(const\s+char\s*\*|int64_t|int)\s*\b(\w+)\s*\((.*)\)")
_PARAMETER = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*)*)\b(\w+)")
_FIELDS = re.compile(r"(?:const\s+)?(\w+)\b\s*(.+)")
_DECLARATOR = re.compile(r"((?:\*\s*)*)(\w+)\s*(?:\[\s*(\w+)\s*\])?")


class AbiError(ValueError):
    pass


def class_name(c_name):
    """s2svc_gemm_desc -> GemmDesc"""
    return "".join(p.capitalize() for p in c_name[len("s2svc_"):].split("_"))


def _declarations(text):
    """-> the header's top-level declarations without their `;` (white space squeezed), and its `#define NAME <integer>` lines."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    if "/*" in text:
        raise AbiError("unterminated comment: " + text[text.index("/*"):][:80])
    defines, lines = {}, []
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):
            m = _PREPROCESSOR.fullmatch(line.strip())
            if not m:
                raise AbiError("preprocessor line not understood: " + line.strip())
            if m.group(2):
                defines[m.group(1)] = int(m.group(2))
            line = ""
        lines.append(line)
    text, n = re.subn(r'extern\s+"C"\s*\{', "", "\n".join(lines).rstrip(), count=1)
    if n:
        if not text.endswith("}"):
            raise AbiError('extern "C" { is never closed')
        text = text[:-1].rstrip()
    decls, pos = [], 0
    while pos < len(text):
        m = _DECLARATION.match(text, pos)                               # up to the next `;` outside braces, one level of braces
        if not m:
            raise AbiError("unterminated declaration (or nested braces): " + " ".join(text[pos:].split())[:200])
        decls.append(" ".join(m.group(1).split()))
        pos = m.end()
    return decls, defines


def _struct(decl, body, types, defines):
    fields = []
    for line in filter(None, (s.strip() for s in body.split(";"))):
        m = _FIELDS.fullmatch(line)
        if not m:
            raise AbiError(f"field `{line}` not understood in: {decl}")
        base = m.group(1)
        for d in m.group(2).split(","):
            dm = _DECLARATOR.fullmatch(d.strip())
            if not dm:
                raise AbiError(f"field `{line}` not understood in: {decl}")
            stars, name, bound = dm.groups()
            ctype = ctypes.c_void_p if stars else types.get(base)
            if ctype is None:
                raise AbiError(f"unknown type `{base}` of field `{line}` in: {decl}")
            if bound is not None:
                if not (bound.isdigit() or bound in defines):
                    raise AbiError(f"unknown array bound `{bound}` of field `{line}` in: {decl}")
                ctype = ctype * (int(bound) if bound.isdigit() else defines[bound])
            fields.append((name + "_" if keyword.iskeyword(name) else name, ctype))
    return fields


def _function(decl, params, types):
    if params.strip() == "void":
        return []
    argtypes = []
    for p in params.split(","):
        m = _PARAMETER.fullmatch(p.strip())
        if not m:
            raise AbiError(f"parameter `{p.strip()}` not understood in: {decl}")
        base, stars, _ = m.groups()
        if stars:
            argtypes.append(ctypes.c_void_p)
        elif base in SCALARS:
            argtypes.append(SCALARS[base])
        elif base in types:
            raise AbiError(f"struct `{base}` passed by value in: {decl}")
        else:
            raise AbiError(f"unknown type `{base}` of parameter `{p.strip()}` in: {decl}")
    return argtypes


def parse(text):
    """Header text -> (functions: name -> (restype, argtypes), structs: Python class name -> ctypes.Structure subclass), both in the
    header's order.  Every pointer, to whatever, is c_void_p: callers pass ctypes.byref(...), an address or None."""
    functions, structs, types = {}, {}, dict(SCALARS)                 # types: C name -> ctype, the structs read so far included
    decls, defines = _declarations(text)
    for decl in decls:
        if _ENUM.fullmatch(decl):
            continue
        m = _STRUCT.fullmatch(decl)
        if m:
            name = class_name(m.group(2))
            types[m.group(2)] = structs[name] = type(name, (ctypes.Structure,), {"_fields_": _struct(decl, m.group(1), types, defines)})
            continue
        m = _FUNCTION.fullmatch(decl)
        if not m:
            raise AbiError("declaration not understood: " + decl)
        functions[m.group(2)] = (RESTYPES.get(m.group(1), ctypes.c_char_p), _function(decl, m.group(3), types))
    return functions, structs


def read_header(path=HEADER):
    with open(path) as f:
        return parse(f.read())
