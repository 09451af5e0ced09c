"""The prototype table of the Python binding (pyft8_amd/_abi.py) against the C header it states: the same functions, the same
argument counts, the same class of type at every position and for the result; both built libraries export all of them and carry
the table after loading; nothing else declares a prototype of an ft8rx_ symbol.  No GPU needed."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from pyft8_amd import _abi, _lib

CLASS_OF = {ctypes.c_char_p: "string", ctypes.c_void_p: "pointer", ctypes.c_int: "int", ctypes.c_int32: "int", ctypes.c_uint64: "uint64",
            ctypes.c_float: "float", None: "void"}


def c_class(decl):
    """Class of one C parameter or result type ('const int32_t* counts', 'int n', 'const char*'): `const char*` is a string, any
    other pointer a pointer, then the scalar's own class."""
    decl = " ".join(decl.split())
    if re.fullmatch(r"const char ?\*( ?\w+)?", decl):
        return "string"
    if "*" in decl:
        return "pointer"
    base = re.sub(r"\bconst\b", "", decl).split()[0]
    return {"int": "int", "int32_t": "int", "uint64_t": "uint64", "float": "float", "void": "void"}[base]


def c_prototypes(text, name_re):
    """{name: (result class, [argument classes])} of the functions matching name_re that `text` declares or defines."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    out = {}
    for res, name, args in re.findall(r"(?:^|[;{}])\s*([\w \t\*]+?)\s*\b(" + name_re + r")\s*\(([^()]*)\)\s*[;{]", text, flags=re.M):
        args = [] if args.strip() in ("", "void") else args.split(",")
        out[name] = (c_class(res), [c_class(a) for a in args])
    return out


def mismatches(table, header):
    """Every way `table` (name -> (restype, argtypes)) disagrees with `header` (c_prototypes), one line each, by name."""
    bad = [f"{n}: in the header, not in the table" for n in sorted(set(header) - set(table))]
    bad += [f"{n}: in the table, not in the header" for n in sorted(set(table) - set(header))]
    for n in sorted(set(table) & set(header)):
        res, args = table[n]
        h_res, h_args = header[n]
        if CLASS_OF[res] != h_res:
            bad.append(f"{n}: result {CLASS_OF[res]}, header {h_res}")
        if len(args) != len(h_args):
            bad.append(f"{n}: {len(args)} arguments, header {len(h_args)}")
            continue
        bad += [f"{n}: argument {i} {CLASS_OF[a]}, header {h}" for i, (a, h) in enumerate(zip(args, h_args)) if CLASS_OF[a] != h]
    return bad


@pytest.fixture(scope="module")
def header():
    return c_prototypes(open(os.path.join(ROOT, "include", "ft8rx.h")).read(), r"ft8rx_\w+")


def test_table_states_the_header(header):
    assert len(header) >= 80 and header["ft8rx_last_error"] == ("string", ["pointer"])          # the parser reads the header
    assert header["ft8rx_set_weak"] == ("int", ["pointer", "int", "float", "int"]) and header["ft8rx_device_count"] == ("int", [])
    assert header["ft8rx_get_stage_times"][1][2] == "pointer" and header["ft8rx_device_pci_bus_id"][1][1] == "pointer"  # char**, char*
    assert mismatches(_abi.PROTOTYPES, header) == []


def test_optional_section_is_the_debug_entries_of_the_source():
    src = open(os.path.join(ROOT, "pyft8_amd", "csrc", "ft8rx.hip")).read()
    debug = c_prototypes(src, r"ft8rx_debug_\w+")
    assert len(debug) == 3 and mismatches(_abi.OPTIONAL, debug) == []
    assert not set(_abi.OPTIONAL) & set(_abi.PROTOTYPES)


def test_a_deleted_entry_and_a_wrong_arity_are_reported_by_name(header):
    scratch = dict(_abi.PROTOTYPES)                       # a copy: the module's table stays as it is
    del scratch["ft8rx_fetch_reports"]
    res, args = scratch["ft8rx_ldpc"]
    scratch["ft8rx_ldpc"] = (res, args[:-1])
    res, args = scratch["ft8rx_set_weak"]
    scratch["ft8rx_set_weak"] = (res, args[:2] + (ctypes.c_int32,) + args[3:])          # the float taken for an int
    bad = mismatches(scratch, header)
    assert len(bad) == 3 and bad[0].startswith("ft8rx_fetch_reports: in the header") and bad[1].startswith("ft8rx_ldpc: 10 arguments")
    assert bad[2] == "ft8rx_set_weak: argument 2 int, header float"
    assert mismatches(_abi.PROTOTYPES, header) == []


@pytest.mark.parametrize("wide", [False, True])
def test_built_library_exports_and_carries_the_table(wide):
    raw = ctypes.CDLL(_lib.LIB_PATH_WIDE if wide else _lib.LIB_PATH)
    assert [n for n in _abi.PROTOTYPES if not hasattr(raw, n)] == []
    L = _lib.lib(wide)
    for n, (res, args) in _abi.PROTOTYPES.items():
        fn = getattr(L, n)
        assert fn.argtypes == list(args) and fn.restype is res, n
    # a name the library lacks is reported, not raised one by one; the optional section is declared only where it is exported
    assert _abi.declare(raw, dict(_abi.PROTOTYPES, ft8rx_not_there=(None, ()), ft8rx_nor_this=(None, ()))) == ["ft8rx_not_there", "ft8rx_nor_this"]
    assert not any(hasattr(raw, n) for n in _abi.OPTIONAL)


def test_load_refuses_a_library_that_lacks_entries_naming_all_of_them(monkeypatch):
    monkeypatch.setattr(_lib, "_libs", {})
    monkeypatch.setattr(_abi, "declare", lambda L: ["ft8rx_not_there", "ft8rx_nor_this"])
    with pytest.raises(_lib.Ft8rxError, match="does not export ft8rx_not_there, ft8rx_nor_this: .*build it again"):
        _lib.lib()


def test_no_other_file_declares_a_prototype():
    found = []
    for top in ("pyft8_amd", "tests", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                path = os.path.join(d, f)
                if not f.endswith(".py") or path == os.path.join(ROOT, "pyft8_amd", "_abi.py"):
                    continue
                for i, line in enumerate(open(path, errors="replace"), 1):
                    if re.search(r"\.(argtypes|restype)\s*=[^=]", line) and "ft8o_" not in line:
                        found.append(f"{os.path.relpath(path, ROOT)}:{i}")
    assert found == []
