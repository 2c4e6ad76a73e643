"""Reader of include/zira_msda.h and include/zira_metrics.h: a header's prototypes, structs and limits as ctypes objects.

Not a C parser.  The headers keep to ``ret zira_name(type name, ...);``, ``typedef struct zira_x { type a, b; type c[N]; ... }
zira_x;`` and ``#define ZIRA_NAME <integer>``; anything else raises ``HeaderError`` with the line it stands on -- nothing is guessed and
nothing is skipped.  Where a new declaration does not read, respell the declaration."""
import ctypes
import re

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "long long": ctypes.c_longlong, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
POINTEES = frozenset(["void", "float", "double", "int32_t", "int64_t", "uint8_t", "uint32_t", "uint64_t", "unsigned char"])
RESULTS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}

_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", re.M)
_INTEGER = re.compile(r"(0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)[uUlL]*")
_NOT_C = re.compile(r'^[ \t]*(#.*|extern[ \t]+"C"[ \t]*\{|\})[ \t]*$', re.M)     # preprocessor lines, the extern "C" bracket
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
_VARIABLE = re.compile(r"(?:const\s+)?(\w+(?:\s+\w+)*?)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)")    # [const] type [*] name[, name ...]
_ARRAY = re.compile(r"(.+?)\s*\[\s*(\w+)\s*\]", re.S)                                      # declaration [N]
_FUNCTION = re.compile(r"(.+?)\s*\b(zira_\w+)\s*\((.*)\)", re.S)


class HeaderError(ImportError):
    pass


def parse(text, device_tables=(), name="zira_msda.h"):
    """``(prototypes, structs, constants)`` of the header ``text``: name -> (restype, argtypes), name -> ctypes.Structure
    subclass, name -> int, each in header order.  A scalar is its ctypes scalar, a pointer to a scalar or to void is
    ``c_void_p`` (callers pass addresses, None and ctypes arrays), a pointer to a struct is ``POINTER`` of its class -- except
    for the structs named in ``device_tables``, whose arrays live in device memory and are passed by address: ``c_void_p``."""
    blank = lambda m: "\n" * m.group().count("\n")      # line numbers stay the header's
    text = _COMMENT.sub(blank, text)
    prototypes, structs, constants = {}, {}, {}

    def fail(pos, what, chunk):
        raise HeaderError("%s line %d: %s: %r" % (name, text.count("\n", 0, pos) + 1, what, " ".join(chunk.split())))

    def variable(pos, decl, member=False):
        """``decl`` as (names, ctypes type).  A struct member may be one array, ``type name[N]``, N an integer or a limit
        defined above it."""
        a = _ARRAY.fullmatch(decl.strip()) if member else None
        if a:
            count = constants.get(a.group(2), int(a.group(2)) if a.group(2).isdigit() else 0)
            names, ctype = variable(pos, a.group(1))
            if len(names) != 1 or count < 1:
                fail(pos, "no ctypes mapping for", decl)
            return names, ctype * count
        m = _VARIABLE.fullmatch(decl.strip())
        base, star, names = (" ".join(m.group(1).split()), m.group(2), m.group(3).replace(",", " ").split()) if m else ("", "", [])
        if not star and base in SCALARS:
            return names, SCALARS[base]
        if star and len(names) == 1 and (base in POINTEES or base in device_tables and base in structs):
            return names, ctypes.c_void_p
        if star and len(names) == 1 and base in structs:
            return names, ctypes.POINTER(structs[base])
        fail(pos, "no ctypes mapping for", decl)

    for m in _DEFINE.finditer(text):
        value = m.group(2).strip()
        if value:                                         # the include guard has none
            if not _INTEGER.fullmatch(value):
                fail(m.start(), "not an integer literal", m.group())
            constants[m.group(1)] = int(value.rstrip("uUlL"), 0)
    text = _NOT_C.sub("", text)

    def struct(m):
        if m.group(1) != m.group(3) or m.group(1) in structs:
            fail(m.start(), "struct tag and typedef name differ, or declared twice", m.group(1) + " / " + m.group(3))
        fields = []
        for member in re.finditer(r"[^;]+", m.group(2)):
            if member.group().strip():
                names, ctype = variable(m.start(2) + member.end() - len(member.group().lstrip()), member.group(), member=True)
                fields += [(name, ctype) for name in names]
        structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": fields})
        return blank(m)

    text = _STRUCT.sub(struct, text)
    for m in re.finditer(r"[^;]+", text):
        decl = m.group().strip()
        if decl:
            pos = m.end() - len(m.group().lstrip())
            f = _FUNCTION.fullmatch(decl)
            result = " ".join(f.group(1).split()) if f else None
            if result not in RESULTS or f.group(2) in prototypes:
                fail(pos, "not a readable declaration (or declared twice)", decl)
            args = f.group(3).strip()
            prototypes[f.group(2)] = (RESULTS[result],
                                      [] if args in ("", "void") else [variable(pos, a)[1] for a in args.split(",")])
    return prototypes, structs, constants
