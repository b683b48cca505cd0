"""The C ABI as include/bcx.h states it, read from the header's text at import: prototypes become ctypes signatures, enums and integer
#defines constants, the two structs ctypes.Structure classes.  The header's opening comment names the grammar; a declaration outside
it raises here and names itself -- nothing is skipped, and there is no second table to fall back on."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_SCALAR = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
_RETURN = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}


def header_path(here=_HERE):
    """include/bcx.h of a source checkout, else the copy setup.py puts next to libbcx.so in an installed package."""
    paths = (os.path.join(os.path.dirname(os.path.dirname(here)), "include", "bcx.h"), os.path.join(here, "_lib", "bcx.h"))
    for p in paths:
        if os.path.exists(p):
            return p
    raise RuntimeError("bcx.h found neither at %s nor at %s: the binding takes every signature from it" % paths)


def _declarator(decl, where):
    """(name, ctypes type) of one `TYPE name`, a parameter or a struct field; any pointer is a c_void_p."""
    toks = re.findall(r"\w+|\S", decl)                          # words, and * [ ] ( ) one by one
    kind = [t for t in toks[:-1] if t != "const"]
    named = len(toks) > 1 and re.fullmatch(r"\w+", toks[-1]) and toks[-1] != "const" and toks[-1] not in _SCALAR
    pointer = "*" in kind and all(re.fullmatch(r"\w+|\*", t) for t in kind)
    if not named or not (pointer or (len(kind) == 1 and kind[0] in _SCALAR)):
        raise ValueError("%s: `%s` is not `TYPE name` with TYPE a pointer or one of %s" % (where, decl.strip(), ", ".join(_SCALAR)))
    return toks[-1], ctypes.c_void_p if pointer else _SCALAR[kind[0]]


def parse(text):
    """(constants {name: int}, structs {name: Structure class}, prototypes {name: (restype, [argtypes])}) of a header's text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(BCX_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    n_calls = len(re.findall(r"bcx_\w+\s*\(", text))
    structs, protos = {}, {}

    def enum(m):
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            e = re.fullmatch(r"(BCX_\w+)\s*=\s*(-?\d+)", item)
            if not e:
                raise ValueError("enum entry `%s` is not NAME = integer" % item)
            consts[e.group(1)] = int(e.group(2))
        return " "

    def struct(m):
        fields = [_declarator(f, "struct " + m.group(1)) for f in m.group(2).split(";") if f.strip()]
        structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": fields})
        return " "

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", struct, text)
    text = re.sub(r'\btypedef\s+struct\s+\w+\s+\w+\s*;|\bextern\s+"C"\s*\{|\}', " ", text)      # the opaque handle, the C++ guard
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):                   # what is left: one prototype per `;`
        m = re.fullmatch(r"(.*?)\s*\b(bcx_\w+)\s*\((.*)\)", stmt)
        ret = re.sub(r"\s*\*\s*", "*", m.group(1)) if m else None
        if ret not in _RETURN:
            raise ValueError("cannot read the declaration `%s`" % stmt)
        params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
        protos[m.group(2)] = (_RETURN[ret], [_declarator(p, m.group(2))[1] for p in params])
    if len(protos) != n_calls:
        raise ValueError("%d prototypes read, but `bcx_name(` occurs %d times: one was lost or stands twice" % (len(protos), n_calls))
    return consts, structs, protos


with open(header_path()) as _f:
    CONSTANTS, STRUCTS, PROTOTYPES = parse(_f.read())
