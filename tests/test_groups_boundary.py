"""CPU: the companion header of the grouped-observation export (include/dbg_mi355x_groups.h) -- the library exports every symbol
it declares, the ctypes mirror binds them, and its generated Rust binding (integration/dbg_mi355x_groups_sys.rs) is current and
lays its structs out like the ctypes mirror."""
import ctypes as C
import importlib.util
import os
import re

from pkg import capi, ROOT

spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)

MIRROR = {"dbg_group_params": capi.GroupParams, "dbg_kmer_groups": capi.KmerGroups}


def parsed():
    return G.parse(open(G.GROUPS_HEADER).read())


def test_library_exports_every_group_symbol():
    hdr = G.strip_comments(open(G.GROUPS_HEADER).read())
    declared = set(re.findall(r"\b(dbg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(capi.GROUP_EXPORTS), declared ^ set(capi.GROUP_EXPORTS)
    lib = capi.load()
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes, name


def test_abi_version_is_7():
    hdr = open(os.path.join(ROOT, "include", "dbg_mi355x.h")).read()
    assert re.search(r"#define DBG_ABI_VERSION 7\b", hdr)


def test_generated_groups_binding_is_current():
    structs, enums, funcs = parsed()
    assert open(G.GROUPS_OUT).read() == G.emit_groups(structs, enums, funcs), "run python tools/gen_rust_ffi.py --groups"
    assert sorted(f[0] for f in funcs) == sorted(capi.GROUP_EXPORTS)


def test_group_struct_layouts_match_the_ctypes_mirror():
    structs, _, _ = parsed()
    assert {n for n, _ in structs} == set(MIRROR)
    for name, fields in structs:
        cls = MIRROR[name]
        size, offs = G.c_layout(fields)
        assert size == C.sizeof(cls), (name, size, C.sizeof(cls))
        assert [n for n, _ in offs] == [f[0] for f in cls._fields_], name
        for fname, off in offs:
            assert getattr(cls, fname).offset == off, (name, fname)
