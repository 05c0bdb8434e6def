"""Reader of include/dawn_hip.h: the header is the one definition of the C ABI and _lib.lib() binds from what this module reads.

It takes the header TEXT and understands exactly what that file uses: `ret dawn_name(args);`, `typedef struct T { fields } T;`,
opaque `typedef struct T T;`, anonymous enums and integer `#define`s.  Any other statement, an unknown type or a function-pointer
argument raises HeaderError with the declaration quoted -- nothing is skipped, because an unbound function would silently take
ctypes' default int arguments.

Scalars map by name and exactly.  `const char*` maps to c_char_p and EVERY other pointer to c_void_p, whatever it points to: the C
type cannot tell a device address (tensor.data_ptr(), an int) from a host array or an out-parameter (a ctypes array, byref, a
pointer instance), and c_void_p takes all of them and None.  So the element type of a host pointer argument is not checked."""
import ctypes as C
import re

SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "unsigned": C.c_uint,
           "unsigned long long": C.c_ulonglong, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int16_t": C.c_int16,
           "unsigned char": C.c_ubyte}
_DECLARATOR = re.compile(r"([\w ]*?)\s*((?:\*\s*)*)\b(\w+)\s*(?:\[\s*(\w+)\s*\])?")     # [base words] [stars] name [array size]


class HeaderError(ValueError):
    pass


def defines(text):
    """{NAME: value} of the integer `#define NAME value` lines."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#define[ \t]+(\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$", text, flags=re.M)}


def _statements(text):
    """The `;`-terminated statements outside braces, without comments, preprocessor lines and the extern "C" wrapper."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    depth, start = 0, 0
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            yield " ".join(text[start:i].split())
            start = i + 1
    if text[start:].strip():
        raise HeaderError(f"unterminated declaration: {' '.join(text[start:].split())[:200]!r}")


def _ctype(base, stars, known, decl):
    """The ctypes type of `base` followed by `stars` asterisks; known = the struct names declared so far ({name: Structure or None})."""
    words = base.split()
    is_const, base = "const" in words, " ".join(w for w in words if w != "const")
    if base not in SCALARS and base not in ("void", "char") and base not in known:
        raise HeaderError(f"unknown type {base!r} in: {decl}")
    if stars:
        return C.c_char_p if (base, stars, is_const) == ("char", 1, True) else C.c_void_p
    if base in SCALARS:
        return SCALARS[base]
    if known.get(base) is None:
        raise HeaderError(f"{base!r} by value in: {decl}")
    return known[base]


def _fields(body, known, sizes, decl):
    fields = []
    for d in filter(None, (d.strip() for d in body.split(";"))):
        fp = re.fullmatch(r"[\w ]+\(\s*\*\s*(\w+)\s*\)\s*\(.*\)", d)             # a function-pointer field is one pointer
        if fp:
            fields.append((fp.group(1), C.c_void_p))
            continue
        base = None
        for part in d.split(","):                                               # `int a, b[8]`: the base carries over, stars do not
            m = _DECLARATOR.fullmatch(part.strip().replace("const*", "*"))
            if not m or (base is None and not m.group(1)) or (base is not None and m.group(1)):
                raise HeaderError(f"cannot read field {d!r} of: {decl[:120]}")
            base = base or m.group(1)
            t = _ctype(base, m.group(2).count("*"), known, d)
            if m.group(4):
                n = m.group(4)
                if not n.isdigit() and n not in sizes:
                    raise HeaderError(f"unknown array size {n!r} in field {d!r} of: {decl[:120]}")
                t = t * (int(n) if n.isdigit() else sizes[n])
            fields.append((m.group(3), t))
    return fields


def _parse(text):
    sizes, known, structs, funcs = defines(text), {}, {}, {}
    for s in _statements(text):
        m = re.fullmatch(r"typedef struct (\w+) (?:\{(.*)\} ?)?(\w+)", s)
        if m and m.group(1) == m.group(3):
            if m.group(2) is None:
                known.setdefault(m.group(1), None)                                # opaque handle
            else:
                structs[m.group(1)] = _fields(m.group(2), known, sizes, s)
                known[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": structs[m.group(1)]})
            continue
        if re.fullmatch(r"enum \{[^{}]*\}", s):
            continue
        m = re.fullmatch(r"([\w ]+?\s*\**)\s*\b(dawn_\w+)\s*\(([^()]*)\)", s)          # (a function-pointer argument has parentheses)
        if not m or m.group(2) in funcs:
            raise HeaderError(f"{'declared twice' if m else 'cannot read'}: {s}")
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        argtypes = []
        for a in ([] if args == "void" else args.split(",")):
            am = _DECLARATOR.fullmatch(a.strip().replace("const*", "*"))
            if not am or not am.group(1) or am.group(4):
                raise HeaderError(f"cannot read argument {a.strip()!r} of: {s}")
            argtypes.append(_ctype(am.group(1), am.group(2).count("*"), known, s))
        restype = None if ret.strip() == "void" else _ctype(ret.replace("*", " "), ret.count("*"), known, s)
        funcs[name] = (restype, argtypes)
    return funcs, structs


def functions(text):
    """{name: (restype, [argtypes])} of every function the header declares."""
    return _parse(text)[0]


def structs(text):
    """{name: [(field, ctype)]} of every struct the header defines, for ctypes' natural C layout."""
    return _parse(text)[1]
