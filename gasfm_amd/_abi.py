"""include/gasfm.h as ctypes: the header is the only statement of the C ABI.

Read once at import:
  functions  name -> (restype, argtypes) of every ``gasfm_*`` prototype
  constants  name -> int, the members of the anonymous enums and ``#define GASFM_X <integer>``
  structs    name -> ctypes.Structure subclass of every ``typedef struct gasfm_x { ... } gasfm_x;``

The parser knows the header's grammar and nothing beyond it: block comments, the scalar types
below, pointer declarators, one-dimensional fixed arrays and several declarators per line.  Any
pointer is a ``c_void_p`` (callers pass byref / addressof / data_ptr() values), a ``const char*``
return a ``c_char_p``.  Whatever it cannot place raises ValueError naming the declaration.
"""
import ctypes
import re

from .build import HEADER

_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
            "uint16_t": ctypes.c_uint16, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double}
_POINTEES = {"void", "char", "uint8_t", "uint64_t"}  # further types the header only points to

_STATEMENT = re.compile(r"\s*(?:enum\s*\{(?P<enum>[^{}]*)\}"
                        r"|typedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<fields>[^{}]*)\}\s*(?P=struct)"
                        r"|(?P<proto>[^;{}]+))\s*;")
_PROTOTYPE = re.compile(r"(?P<ret>(?:const\s+)?\w+\s*\*?)\s*(?P<name>gasfm_\w+)\s*\((?P<params>[^()]*)\)")
_DECLARATORS = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[(\d+)\])?")
_DEFINE = re.compile(r"#\s*define\s+(\w+)[ \t]*(.*)")
_SKIPPED = re.compile(r"#\s*(?:include|ifndef|ifdef|endif)\b")


def _declared(decl, structs):
    """[(name, ctype)] of one declaration: 'const float *W1, *b1', 'int64_t E, m, n', 'float r[3]'."""
    m = _DECLARATORS.fullmatch(decl.strip())
    if not m:
        raise ValueError(f"gasfm.h: cannot parse the declaration '{decl.strip()}'")
    base, out = m.group(1), []
    for d in m.group(2).split(","):
        m = _DECLARATOR.fullmatch(d.strip())
        if not m:
            raise ValueError(f"gasfm.h: cannot parse the declarator '{d.strip()}' of '{decl.strip()}'")
        stars, name, count = m.groups()
        if base not in _SCALARS and not (stars and (base in _POINTEES or base in structs)):
            raise ValueError(f"gasfm.h: unknown type '{base}' in '{decl.strip()}'")
        t = ctypes.c_void_p if stars else _SCALARS[base]
        out.append((name, t * int(count) if count else t))
    return out


def _prototype(stmt, structs):
    m = _PROTOTYPE.fullmatch(stmt)
    if not m:
        raise ValueError(f"gasfm.h: cannot parse the declaration '{stmt}'")
    ret = m.group("ret").replace("const", "").split()
    if ret == ["void"]:
        restype = None
    elif "".join(ret) == "char*":
        restype = ctypes.c_char_p
    elif len(ret) == 1 and ret[0] in _SCALARS:
        restype = _SCALARS[ret[0]]
    else:
        raise ValueError(f"gasfm.h: unknown return type of '{stmt}'")
    params = m.group("params").strip()
    argtypes = []
    for p in [] if params in ("", "void") else params.split(","):
        (_, t), = _declared(p, structs)
        argtypes.append(t)
    return m.group("name"), (restype, argtypes)


def parse(text):
    """(functions, constants, structs) of the header text."""
    functions, constants, structs = {}, {}, {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus\n.*?#endif\n", "", text, flags=re.S)  # the extern "C" braces
    code = []
    for line in text.splitlines():
        line = line.strip()
        m = _DEFINE.match(line)
        if not line.startswith("#"):
            code.append(line)
        elif m and m.group(2):  # a define without a value (the include guard) is no constant
            if not re.fullmatch(r"-?\d+", m.group(2)):
                raise ValueError(f"gasfm.h: '{line}' does not define an integer")
            constants[m.group(1)] = int(m.group(2))
        elif not m and not _SKIPPED.match(line):
            raise ValueError(f"gasfm.h: unknown preprocessor line '{line}'")
    text, pos = "\n".join(code), 0
    while text[pos:].strip():
        m = _STATEMENT.match(text, pos)
        if not m:
            raise ValueError(f"gasfm.h: cannot parse the declaration '{' '.join(text[pos:].split(';')[0].split())}'")
        pos = m.end()
        if m.group("enum") is not None:
            for member in filter(None, (s.strip() for s in m.group("enum").split(","))):
                mm = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", member)
                if not mm:
                    raise ValueError(f"gasfm.h: enum member '{member}' has no explicit integer value")
                constants[mm.group(1)] = int(mm.group(2))
        elif m.group("struct"):
            fields = [f for decl in m.group("fields").split(";") if decl.strip() for f in _declared(decl, structs)]
            structs[m.group("struct")] = type(m.group("struct"), (ctypes.Structure,), {"_fields_": fields})
        else:
            name, sig = _prototype(" ".join(m.group("proto").split()), structs)
            functions[name] = sig
    return functions, constants, structs


with open(HEADER) as _f:
    functions, constants, structs = parse(_f.read())
