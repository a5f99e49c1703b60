"""The C ABI as ONE surface (no GPU): every header of include/ against its table of m2trans_amd._lib.ABI against libm2t.so.

* the headers of include/ are the keys of ABI, the build lists every header and every source;
* the m2t_* names a header declares, in order, are the keys of its table; no symbol sits under two headers;
* every prototype agrees with its (restype, argtypes) type by type under the one rule of ``allowed`` below -- a float where the C side
  takes a double, or a c_int for a long long, does not raise at the call: it hands a kernel a garbage size or pointer;
* the whole surface equals tests/golden/abi_surface.json, which was written from the commit BEFORE the tables became ABI
  (``python tests/test_abi_surface_cpu.py --write PATH_TO_THAT_CHECKOUT``), never from the code under test: a deliberate change of the
  ABI regenerates it from the checkout that makes the change and shows up in the diff of the JSON;
* with the library loaded, every symbol is exported and carries the table's restype and argtypes."""
import ctypes as C
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_surface.json")
HEADERS = sorted(os.listdir(os.path.join(ROOT, "include")))

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
           "size_t": C.c_size_t}
TYPED_POINTEES = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong, "unsigned char": C.c_ubyte}
_PROTOTYPE = re.compile(r"([A-Za-z_][\w\s\*]*?)\b(m2t_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def prototypes(root, header):
    """[(name, return type, [parameter, ...])] of the functions a header declares, in order; comments and preprocessor lines removed."""
    src = open(os.path.join(root, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^[ \t]*#[^\n]*$", " ", src, flags=re.M)
    found = [(m.group(2), m.group(1), m.group(3)) for m in _PROTOTYPE.finditer(src)]
    # (the parser may not lose a declaration: every m2t_* name in front of a parenthesis is one of the prototypes)
    assert [n for n, _, _ in found] == re.findall(r"\b(m2t_[a-z0-9_]+)\s*\(", src), header
    return [(n, ret, [] if args.strip() in ("", "void") else [a.strip() for a in args.split(",")]) for n, ret, args in found]


def _split(decl, named):
    """(base type without const, pointer depth, const seen) of a return type or of a parameter (its name and array bound dropped)."""
    decl, is_array = re.subn(r"\[\s*\w*\s*\]\s*$", "", decl)
    tokens = decl.replace("*", " * ").split()
    if named and len(tokens) > 1 and tokens[-1] != "*":
        tokens = tokens[:-1]
    return " ".join(t for t in tokens if t not in ("*", "const")), tokens.count("*") + is_array, "const" in tokens


def allowed(decl, named=True):
    """The ctypes types that may stand for one C type: the one rule of this ABI."""
    base, depth, const = _split(decl, named)
    if depth == 0:
        return [None] if base == "void" and not named else [SCALARS[base]]        # (KeyError: a by-value type the rule does not know)
    if depth == 2:
        return [C.POINTER(C.c_void_p)]
    if base == "char" and const:
        return [C.c_char_p]
    if base in TYPED_POINTEES:
        return [C.c_void_p, C.POINTER(TYPED_POINTEES[base])]
    return [C.c_void_p]


def _name(t):
    return None if t is None else f"POINTER({t._type_.__name__})" if hasattr(t, "contents") else t.__name__


def _type(name):
    if name is None:
        return None
    m = re.fullmatch(r"POINTER\((\w+)\)", name)
    return C.POINTER(getattr(C, m.group(1))) if m else getattr(C, name)


def surface(abi):
    """header -> symbol -> [restype, [argtypes]] with the ctypes types written by name."""
    return {h: {n: [_name(res), [_name(a) for a in args]] for n, (res, args) in table.items()} for h, table in abi.items()}


# ------------------------------------------------------------------------------------------------------------- the tests
def test_headers_are_the_keys_of_the_table_and_the_build_lists_every_file():
    from m2trans_amd import _lib, build as B
    assert sorted(_lib.ABI) == HEADERS
    listed = {os.path.normpath(os.path.join(B.CSRC, h)) for h in B.HEADERS}
    for h in HEADERS:
        assert os.path.join(ROOT, "include", h) in listed, h
    csrc = os.listdir(B.CSRC)
    assert sorted(f for f in csrc if f.endswith(".hip")) == sorted(B.SOURCES)
    assert {f for f in csrc if f.endswith(".h")} <= set(B.HEADERS)


@pytest.mark.parametrize("header", HEADERS)
def test_header_declares_the_tables_names_in_order_and_every_prototype_agrees_type_by_type(header):
    from m2trans_amd import _lib
    table = _lib.ABI[header]
    protos = prototypes(ROOT, header)
    assert [n for n, _, _ in protos] == list(table)
    for name, ret, params in protos:
        res, args = table[name]
        assert res in allowed(ret, named=False), (name, ret, res)
        assert len(args) == len(params), (name, len(args), len(params))
        for k, (p, a) in enumerate(zip(params, args)):
            assert a in allowed(p), (name, k, p, a)


def test_no_symbol_under_two_headers():
    from m2trans_amd import _lib
    every = [n for table in _lib.ABI.values() for n in table]
    assert len(every) == len(set(every))


def test_the_surface_is_the_recorded_one():
    from m2trans_amd import _lib
    want = json.load(open(GOLDEN))
    assert len(want) == 18 and sum(len(t) for t in want.values()) == 133
    got = surface(_lib.ABI)
    assert list(got) == list(want)                                   # the headers in their order
    for h in want:
        assert list(got[h]) == list(want[h]), h                      # the symbols in declaration order
        for n in want[h]:
            assert got[h][n] == want[h][n], (h, n)
    # (by name is by type: the names resolve to the very ctypes objects of the table)
    for h, table in _lib.ABI.items():
        for n, (res, args) in table.items():
            assert _type(want[h][n][0]) is res and [_type(a) for a in want[h][n][1]] == list(args), (h, n)


def test_the_loaded_library_exports_every_symbol_with_the_tables_types():
    from m2trans_amd import _lib
    lib = _lib.load()
    for h, table in _lib.ABI.items():
        for n, (res, args) in table.items():
            fn = getattr(lib, n)
            assert fn.restype is res and list(fn.argtypes) == list(args), (h, n)


# ------------------------------------------------------------------------------------------------------------- --write
def _tables_of(root):
    """header -> table of the _lib.py of another checkout, imported by path.  A checkout that has ABI gives it; one from before gives
    its module-level tables, in the order its load() binds them, each filed under the header that declares its symbols.  Within a
    header the symbols are written in the header's declaration order (the one table of that time that was not kept in that order is
    include/m2t.h's: its nine operator entries stood at the end)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_abi_parent_lib", os.path.join(root, "m2trans_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    declared = {h: [n for n, _, _ in prototypes(root, h)] for h in sorted(os.listdir(os.path.join(root, "include")))}
    if hasattr(mod, "ABI"):
        tables = dict(mod.ABI)
    else:
        home = {n: h for h, names in declared.items() for n in names}
        tables = {}
        for value in vars(mod).values():
            if isinstance(value, dict) and value and all(isinstance(k, str) and k.startswith("m2t_") for k in value):
                headers = {home[n] for n in value}
                assert len(headers) == 1 and not headers & set(tables), headers
                tables[headers.pop()] = value
    assert all(sorted(t) == sorted(declared[h]) for h, t in tables.items())
    return {h: {n: t[n] for n in declared[h]} for h, t in tables.items()}


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_abi_surface_cpu.py --write PATH_TO_PARENT_CHECKOUT")
    with open(GOLDEN, "w") as f:                                     # one symbol per line
        f.write("{\n" + ",\n".join(f" {json.dumps(h)}: {{\n" + ",\n".join(f"  {json.dumps(n)}: {json.dumps(e)}" for n, e in t.items()) + "\n }"
                                   for h, t in surface(_tables_of(sys.argv[2])).items()) + "\n}\n")
    print(f"wrote {GOLDEN}")
