"""Regex reader of include/mia.h and its comparison with the ctypes table of mlx_swift_audio_amd/_abi.py (tests only).

The header is plain C89-style declarations over a closed set of types: `int`, `int32_t`, `int64_t`, `float`, `double`, `void`,
`const char*` and pointers (to those scalars, `uint32_t`, `void`, an opaque handle or one of the header's structs).  Anything else
raises ValueError, so a new kind of argument cannot pass unclassified.

Layout: the structs hold only 4-byte and 8-byte scalars, pointers and arrays of those, and ctypes aligns each field naturally exactly
as the C compiler does.  Equal field names, order, kinds and array lengths therefore mean equal layout; no sizeof probe is needed.
"""
import ctypes as C
import re

SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "float": "f32", "double": "f64"}
POINTEES = set(SCALARS) | {"void", "char", "uint32_t"}
CTYPES = {C.c_int: "i32", C.c_int64: "i64", C.c_float: "f32", C.c_double: "f64", C.c_char_p: "str", C.c_void_p: "ptr", None: "void"}


def _kind(ctype: str, names: dict) -> str:
    """'const int32_t* const*' -> 'ptr', 'const char*' -> 'str', 'const mia_tensor_view*' -> 'struct:mia_tensor_view', 'int' -> 'i32'."""
    words = re.sub(r"\bconst\b", " ", ctype).replace("*", " * ").split()
    base, stars = [w for w in words if w != "*"], words.count("*")
    if len(base) != 1 or (base[0] not in POINTEES and base[0] not in names):
        raise ValueError(f"type outside the closed set: '{ctype}'")
    if stars == 0:
        if base[0] == "void":
            return "void"
        if base[0] not in SCALARS:
            raise ValueError(f"type outside the closed set: '{ctype}'")
        return SCALARS[base[0]]
    if base[0] == "char":
        return "str" if stars == 1 else "ptr"
    return f"struct:{base[0]}" if stars == 1 and names.get(base[0]) == "struct" else "ptr"


def parse(text: str):
    """-> (functions {name: (return kind, [argument kinds])}, structs {name: [(field, kind, array_len or 0)]})."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"typedef\s+enum\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    struct_re = re.compile(r"typedef\s+struct\s*\{(.*?)\}\s*(mia_\w+)\s*;", re.S)
    names = {n: "handle" for n in re.findall(r"typedef\s+struct\s+(mia_\w+)\s+\1\s*;", text)}
    names.update({n: "struct" for _, n in struct_re.findall(text)})
    structs = {}
    for body, name in struct_re.findall(text):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"((?:const\s+)?\w+\s*\**)\s*(\w+(?:\s*\[\d+\])?(?:\s*,\s*\w+(?:\s*\[\d+\])?)*)", decl, re.S)
            if not m:
                raise ValueError(f"{name}: cannot read field declaration '{decl}'")
            for d in m.group(2).split(","):
                f = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
                fields.append((f.group(1), _kind(m.group(1), names), int(f.group(2) or 0)))
        structs[name] = fields
    text = struct_re.sub(" ", text)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", text)
    functions = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(mia_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [] if args.strip() == "void" else [a.strip() for a in args.split(",")]
        kinds = []
        for a in args:
            m = re.fullmatch(r"(.*?[\s\*])(\w+)", a, re.S)
            if not m:
                raise ValueError(f"{name}: cannot read argument '{a}'")
            kinds.append(_kind(m.group(1), names))
        functions[name] = (_kind(ret, names), kinds)
    return functions, structs


def mem_entry_points(text: str) -> list:
    """Names of the functions whose last parameter is `int mem`, in header order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return [name for name, args in re.findall(r"\b(mia_\w+)\s*\(([^()]*)\)\s*;", text) if re.search(r"[\s,]int\s+mem\s*$", args)]


def _ckind(t, structs) -> str:
    if t in CTYPES:
        return CTYPES[t]
    for name, cls in structs.items():
        if t is C.POINTER(cls):
            return f"struct:{name}"
    return f"unknown:{t!r}"


def compare(header_text: str, prototypes: dict, structs: dict) -> list:
    """Every difference between the header and the table, one string each, starting with the function or struct it concerns."""
    functions, hstructs = parse(header_text)
    out = [f"{n}: in the header, not in PROTOTYPES" for n in functions if n not in prototypes]
    out += [f"{n}: in PROTOTYPES, not in the header" for n in prototypes if n not in functions]
    out += [f"{n}: in the header, not in STRUCTS" for n in hstructs if n not in structs]
    out += [f"{n}: in STRUCTS, not in the header" for n in structs if n not in hstructs]
    for n, (hret, hargs) in functions.items():
        if n not in prototypes:
            continue
        restype, argtypes = prototypes[n]
        if _ckind(restype, structs) != hret:
            out.append(f"{n}: returns {hret} in the header, {_ckind(restype, structs)} in the table")
        if len(argtypes) != len(hargs):
            out.append(f"{n}: {len(hargs)} arguments in the header, {len(argtypes)} in the table")
            continue
        for i, (h, t) in enumerate(zip(hargs, argtypes)):
            k = _ckind(t, structs)
            if k != h and not (h.startswith("struct:") and k == "ptr"):
                out.append(f"{n}: argument {i} is {h} in the header, {k} in the table")
    for n, hfields in hstructs.items():
        if n not in structs:
            continue
        mirror = [(f, _ckind(getattr(t, "_type_", t) if hasattr(t, "_length_") else t, structs), getattr(t, "_length_", 0))
                  for f, t in structs[n]._fields_]
        if mirror != hfields:
            out.append(f"{n}: fields {hfields} in the header, {mirror} in the mirror")
    return out
