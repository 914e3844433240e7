"""The C headers against the ctypes bindings (vcm_ts_amd/lib.py), one case per header: what include/<header> declares,
comments stripped, is what lib.py's table binds for that header -- the same functions, one argtype per parameter, every
symbol in the built library, no function under two headers.  No GPU: nothing is called."""
import os
import re

import pytest

from vcm_ts_amd import lib

INCLUDE = os.path.join(os.path.dirname(lib.HERE), "include")
HEADERS = list(lib.HEADERS) + ["dcvc_rans.h"]


def declared(header):
    """{function: (return type, number of parameters)} of the header's declarations."""
    text = open(os.path.join(INCLUDE, header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = re.findall(r"([\w \*]+?)\b(dcvc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    assert len({name for _, name, _ in found}) == len(found), header  # declared once
    return {name: (" ".join(ret.split()), 0 if params.strip() == "void" else len(params.split(",")))
            for ret, name, params in found}


def bound(header):
    """{function: argtypes as set on the loaded library} of the table's entry for the header."""
    if header == "dcvc_rans.h":
        return {name: getattr(lib.rans(), name).argtypes for name in lib.RANS_SYMBOLS}
    L = lib.hip()
    for name, entry in lib.HEADERS[header].items():  # the library carries what the table says
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == (lib._signature(entry)[0], lib._signature(entry)[1]), name
    return {name: getattr(L, name).argtypes for name in lib.HEADERS[header]}


@pytest.mark.parametrize("header", HEADERS)
def test_header_declares_what_the_table_binds(header):
    decl, table = declared(header), bound(header)  # bound() resolves every symbol: a missing one raises AttributeError
    assert set(decl) == set(table), (sorted(set(decl) - set(table)), sorted(set(table) - set(decl)))
    for name, argtypes in table.items():
        if argtypes is None:  # dcvc_rans.h's two constructors: (void), and rans() sets no argtypes for them
            assert header == "dcvc_rans.h" and decl[name][1] == 0, name
        else:
            assert decl[name][1] == len(argtypes), name
        if header != "dcvc_rans.h":  # what answers the int status (or nothing) is in _SIGS, which test_build.py walks
            assert (decl[name][0] in ("int", "void")) == (name in lib._SIGS), (name, decl[name][0])
    elsewhere = {name for h in HEADERS if h != header for name in declared(h)}
    assert not set(decl) & elsewhere, sorted(set(decl) & elsewhere)
    others = lib.RANS_SYMBOLS if header != "dcvc_rans.h" else []
    others = others + [name for h in lib.HEADERS if h != header for name in lib.HEADERS[h]]
    assert not set(table) & set(others), sorted(set(table) & set(others))


def test_the_lists_are_the_table():
    """Every *_SYMBOLS list is its header's functions; HIP_SYMBOLS the three kernel headers' (sorted); _SIGS the status
    entry points, which tests/test_build.py walks with NULL arguments."""
    core = ("dcvc_hip.h", "dcvc_hip_grad.h", "dcvc_hip_rans.h")
    assert list(lib.HEADERS)[:3] == list(core) and lib.HIP_SYMBOLS == sorted(name for h in core for name in lib.HEADERS[h])
    for h in lib.HEADERS:
        if h not in core:
            listed = getattr(lib, h[len("dcvc_hip_"):-2].upper() + "_SYMBOLS")
            assert listed == list(lib.HEADERS[h]), h
    assert sorted(lib.ALL_HIP_SYMBOLS) == sorted(name for h in lib.HEADERS for name in lib.HEADERS[h])
    assert len(set(lib.ALL_HIP_SYMBOLS)) == len(lib.ALL_HIP_SYMBOLS)
    assert set(lib._SIGS) <= set(lib.ALL_HIP_SYMBOLS)
    L = lib.hip()
    for name in lib._SIGS:
        assert getattr(L, name).restype is (None if name == "dcvc_pack_plan_destroy" else lib.C.c_int), name
