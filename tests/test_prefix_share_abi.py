"""What the dense head shared by prefix (phmm_last_call_prefix_share) is part of the ABI: declared in
include/phmm_amd_share.h (a companion header of phmm_amd.h, whose own symbol table is closed), exported by the library,
bound in Python and in the Rust declarations, its knob documented.  No GPU needed."""
import ctypes as C
import os
import re

from dbgphmm_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_share.h"
SYMBOL = "phmm_last_call_prefix_share"


def _header():
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        return f.read()


def test_header_declares_the_getter():
    src = _header()
    decl = re.search(r"int\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", src)
    assert decl, SYMBOL + " is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["int *out_columns", "uint64_t *out_virtual_lanes"], args
    assert '#include "phmm_amd.h"' in src
    # the header's symbols are exactly those the binding lists for it, and none of them is one of phmm_amd.h's
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(_ffi.EXTENSION_SYMBOLS[HEADER]) == [SYMBOL]
    assert not set(declared) & set(_ffi.DECLARED_SYMBOLS)


def test_library_exports_the_getter():
    lib = _ffi.lib()
    assert hasattr(lib, SYMBOL)
    # read-only, no device needed: nothing has run on this thread, so nothing was shared; NULL outputs are skipped
    j, n = C.c_int(-1), C.c_uint64(99)
    assert lib.phmm_last_call_prefix_share(C.byref(j), C.byref(n)) == _ffi.PHMM_OK
    assert (j.value, n.value) == (0, 0)
    assert lib.phmm_last_call_prefix_share(None, None) == _ffi.PHMM_OK
    assert _ffi.last_call_prefix_share() == (0, 0)


def test_rust_declaration():
    with open(os.path.join(ROOT, "integration", "rust", "amd_sys.rs")) as f:
        src = f.read()
    assert re.search(r"pub fn " + SYMBOL + r"\(out_columns: \*mut c_int, out_virtual_lanes: \*mut u64\) -> c_int;", src)


def test_knob_is_documented():
    """the off switch is named in the comment on the declaration and in the README"""
    doc = _header()
    at = doc.index("PHMM_SHARE_PREFIX")
    assert at < doc.index("int " + SYMBOL) < at + 1000
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "PHMM_SHARE_PREFIX" in f.read()
