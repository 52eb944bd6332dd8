"""pcodec_amd._lib.SIGNATURES against the prototypes of include/pco_gfx.h: every declared function has an entry of the right return type and
the right kind of argument at every position, the table names nothing else, and lib() has applied it.  A function without argtypes takes a
Python int as a C int: a device address passed that way is cut to 32 bits."""
import ctypes as C
import os
import re

import pytest

from pcodec_amd import _lib as G
from pcodec_amd import build as B
from test_abi import ROOT, declared_functions

RETURN_TYPES = {"enum PcoError": C.c_int, "int": C.c_int, "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong, "int64_t": C.c_int64,
                "const char*": C.c_char_p, "void": None}
SCALARS = {"size_t": C.c_size_t, "unsigned char": C.c_ubyte, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}


def prototypes():
    """{name: (return type, [argument type])} of the header: `<return type> pco_...(...);`, some over two or three lines.  An argument's type is
    its text without the parameter name (the handle arguments have none); any pointer is "*"."""
    src = open(os.path.join(ROOT, "include", "pco_gfx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^(\w[\w ]*?\*?)\s*\b(pco_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        kinds = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            a = " ".join(a.split())
            if "*" in a:
                kinds.append("*")
            else:
                words = [w for w in a.split() if w != "const"]
                kinds.append(" ".join(words if " ".join(words) in SCALARS else words[:-1]))
        out[name] = (" ".join(ret.split()).replace(" *", "*"), kinds)
    return out


def test_the_parser_finds_every_declared_function():
    protos = prototypes()
    assert sorted(protos) == declared_functions() and len(protos) >= 71
    assert protos["pco_gfx_last_error"] == ("const char*", [])
    assert protos["pco_chunk_compressor_page_n"] == ("size_t", ["*", "size_t"])
    assert protos["pco_gfx_compact_wrapped_chunks"] == ("enum PcoError", ["size_t", "*", "*", "*", "uint32_t", "*", "uint64_t", "uint64_t", "*", "*", "*"])
    assert protos["pco_gfx_profile_end"] == ("int", ["*", "size_t", "*", "int"])


@pytest.mark.parametrize("name", declared_functions())
def test_signature_matches_the_prototype(name):
    ret, kinds = prototypes()[name]
    assert name in G.SIGNATURES, f"{name} is declared in include/pco_gfx.h and has no ctypes signature"
    restype, argtypes = G.SIGNATURES[name]
    assert restype is RETURN_TYPES[ret], f"{name} returns {ret}"
    assert len(argtypes) == len(kinds), f"{name} takes {len(kinds)} arguments"
    for i, (got, kind) in enumerate(zip(argtypes, kinds)):
        assert got is (C.c_void_p if kind == "*" else SCALARS[kind]), f"argument {i} of {name} is {kind}"


def test_the_table_names_only_declared_functions():
    assert sorted(set(G.SIGNATURES) - set(declared_functions())) == []


def test_lib_applies_the_table():
    if B.needs_build():
        B.build()
    L = G.lib()
    for name in declared_functions():
        f = getattr(L, name)
        assert f.argtypes is not None, f"{name} has no argtypes"
        assert list(f.argtypes) == list(G.SIGNATURES[name][1]) and f.restype is G.SIGNATURES[name][0]


def test_a_size_beyond_32_bits_arrives_whole():
    """What the table is for, on a host-only entry point that reads two bytes: a plain Python int for its size_t length.  Cut to 32 bits, 1 << 32
    would arrive as 0 and the header as empty."""
    if B.needs_build():
        B.build()
    src = (C.c_uint8 * 16)(4, 1)
    used, major, minor = C.c_size_t(0), C.c_uint8(0), C.c_uint8(0)
    G.check(G.lib().pco_wrapped_read_header(src, 1 << 32, C.byref(used), C.byref(major), C.byref(minor)))
    assert (used.value, major.value, minor.value) == (2, 4, 1)
