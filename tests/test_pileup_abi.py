"""The pileup over mapping lists (phmm_run_with_mapping_pileup) is part of the ABI: declared in include/phmm_amd_pileup.h
(the eleventh companion header, which includes phmm_amd_usage.h: the rows come back in that header's handle) with the key,
the rows, the position rule, the column order, the Del note, the promise about bits and the refusals written out,
exported by the library, bound in dbgphmm_amd/_ffi_pileup.py (the tables of _ffi.py stay as they are), named in the
documents.  No GPU needed."""
import inspect
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_pileup, _ffi_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_pileup.h"
SIGNATURES = {
    "phmm_run_with_mapping_pileup": ("int", ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                                             "double *out_logp_forward", "double *out_node_pileup", "phmm_read_usage **out"]),
}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_the_one_symbol():
    """Fails without the feature: the header does not exist."""
    src = _read("include", HEADER)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, (res, want) in SIGNATURES.items():
        decl = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want, name
    assert '#include "phmm_amd_usage.h"' in src and "typedef" not in code  # no new handle type
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(SIGNATURES) == sorted(_ffi_pileup.PILEUP_SYMBOLS[HEADER])
    assert list(_ffi_pileup.PILEUP_SYMBOLS) == [HEADER]


def test_the_closed_tables_stay_closed():
    new = set(SIGNATURES)
    assert not new & set(_ffi.DECLARED_SYMBOLS)
    assert not new & {s for syms in _ffi.EXTENSION_SYMBOLS.values() for s in syms}
    assert not new & {s for syms in _ffi_usage.USAGE_SYMBOLS.values() for s in syms}
    assert HEADER not in _ffi.EXTENSION_SYMBOLS
    assert "pileup" not in _read("include", "phmm_amd.h") and "pileup" not in _read("include", "phmm_amd_usage.h")
    assert len(_ffi_usage.USAGE_SYMBOLS["phmm_amd_usage.h"]) == 6


def test_contract_is_written_out_in_the_header():
    doc = _read("include", HEADER)
    decl = doc.index("int phmm_run_with_mapping_pileup")
    text = " ".join(doc[:decl].replace("\n *", " ").split())
    for word in (
            # what the call runs
            "phmm_run_with_mapping_states", "kept on the device", "for the same inputs and knobs", "A 0, C 1, G 2, T 3",
            # the position rule
            "POSITION of an entry", "the last g with pos_off[g] <= a < pos_off[g + 1]",
            "empty lists before, between and behind are passed over",
            # the key and the row
            "KEY.", "4 * v + c(x)", "K = 4 * N", "ROW of read r", "phmm_read_usage_keys() == 4N", "in ascending order",
            "the sum of exp(state_logp[a][s])", "exp(-inf) is exactly 0", "n <= 64", "n > 64",
            "decided by the lists alone", "stays, with zeros", "listed twice at a position counts twice",
            # the Del note
            "the Del mass of v at the positions whose base is c", "only its sum over c has a meaning of its own",
            "no handle type is added",
            # the column order
            "out_node_pileup[N][9]", "COLUMNS", "0-3 the Match mass", "4-7 the Ins mass", "8 the Del mass",
            "in read order by the one-wave rule", "d = 32, 16, 8, 4, 2, 1", "for any n",
            "4 v .. 4 v + 3 in sorted order (key, then read)", "A node in no row gets zeros",
            "bit for bit", "out == NULL", "NULL, a host pointer or a device pointer",
            # what is promised about bits
            "BITS.", "no floating-point atomics", "the model, the read and its lists alone", "not on the other reads",
            "the chunking under phmm_set_workspace_limit", "the capacity class", "repeated calls return the same bits",
            # the refusals and the rest
            "REFUSALS", "*out left as it was", "those of phmm_run_with_mapping_read_usage", "PHMM_EINVAL",
            "a byte other than A C G T", "naming the read and the position", "before any device work", "PHMM_ECAPACITY",
            "N > 2^30 - 1", "2^31 - 2 row entries", "NO READS", "a handle of 0 rows", "WORKSPACE", "STATISTICS",
            "Index 2 of phmm_last_call_stats", "cells = list entries", "has no knob of its own"):
        assert word in text, word


def test_library_exports_it():
    lib = _ffi_pileup.lib()
    for name in SIGNATURES:
        assert hasattr(lib, name), name
    # NULL model / reads / mappings: refused, nothing dereferenced
    assert lib.phmm_run_with_mapping_pileup(None, None, None, None, None, None) == _ffi.PHMM_EINVAL


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_pileup", None)
    assert callable(fn)
    sig = inspect.signature(fn).parameters
    assert list(sig) == ["self", "reads", "mappings", "want_rows", "want_totals"]
    assert sig["want_rows"].default is True and sig["want_totals"].default is True
    for word in ("include/phmm_amd_pileup.h", "run_with_mapping_states", "Pileup", "4 * node + base", "A 0, C 1, G 2, T 3",
                 "want_rows", "want_totals"):
        assert word in fn.__doc__, word
    for method in ("arrays", "row", "reads_of", "depth", "consensus", "disagreements", "error_profile", "from_arrays"):
        assert callable(getattr(D.Pileup, method, None)), method
    for prop in ("totals", "match_counts", "ins_counts", "del_counts"):
        assert isinstance(getattr(D.Pileup, prop, None), property), prop
    assert callable(D.formats.write_pileup) and callable(D.formats.read_pileup)


def test_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "phmm_run_with_mapping_pileup" in _read(doc), doc
    assert "Pileup over the lists" in _read("DESIGN.md")
    assert "phmm_run_with_mapping_pileup" in _read("integration", "rust", "amd_sys.rs")
    assert os.path.exists(os.path.join(ROOT, "tools", "pileup_time.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "pileup.txt"))
    assert "pileup.hip" in _read("dbgphmm_amd", "csrc", "Makefile")
