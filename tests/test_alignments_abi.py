"""Alignment records (phmm_run_with_mapping_alignments and the phmm_alignments handle) are part of the ABI: declared in
include/phmm_amd_align.h (the sixth companion header of phmm_amd.h, whose own symbol table is closed) with the record,
its invariants and the alignment index written out, exported by the library, bound in dbgphmm_amd/_ffi_align.py (the
tables of _ffi.py stay as they are), named in the documents.  No GPU needed."""
import inspect
import os
import re

import dbgphmm_amd as D
from dbgphmm_amd import _ffi, _ffi_align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "phmm_amd_align.h"
SIGNATURES = {
    "phmm_run_with_mapping_alignments": ("int", ["phmm_model *m", "const phmm_reads *reads", "const phmm_mappings *mappings",
                                                 "uint32_t n_samples", "uint64_t seed", "double *out_logp",
                                                 "double *out_path_logp", "uint32_t *out_counts", "phmm_alignments **out"]),
    "phmm_alignments_count": ("uint64_t", ["const phmm_alignments *a"]),
    "phmm_alignments_total_ops": ("uint64_t", ["const phmm_alignments *a"]),
    "phmm_alignments_total_runs": ("uint64_t", ["const phmm_alignments *a"]),
    "phmm_alignments_export": ("int", ["const phmm_alignments *a", "uint64_t *op_off", "uint32_t *ops", "uint64_t *run_off",
                                       "uint32_t *run_node", "uint32_t *run_len"]),
    "phmm_alignments_destroy": ("void", ["phmm_alignments *a"]),
}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_the_six_symbols():
    src = _read("include", HEADER)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, (res, want) in SIGNATURES.items():
        decl = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want, name
    assert '#include "phmm_amd.h"' in src and re.search(r"typedef\s+struct\s+phmm_alignments\s+phmm_alignments\s*;", code)
    for name, value in (("PHMM_ALN_INS", 1), ("PHMM_ALN_DEL", 2), ("PHMM_ALN_EQ", 7), ("PHMM_ALN_DIFF", 8)):  # BAM's
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", src), name
    declared = sorted(set(re.findall(r"\b(phmm_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(SIGNATURES) == sorted(_ffi_align.ALIGN_SYMBOLS[HEADER])
    assert list(_ffi_align.ALIGN_SYMBOLS) == [HEADER]


def test_the_closed_tables_stay_closed():
    new = set(SIGNATURES)
    assert not new & set(_ffi.DECLARED_SYMBOLS)
    assert not new & {s for syms in _ffi.EXTENSION_SYMBOLS.values() for s in syms}
    assert HEADER not in _ffi.EXTENSION_SYMBOLS


def test_record_is_written_out_in_the_header():
    doc = _read("include", HEADER)
    decl = doc.index("int phmm_run_with_mapping_alignments")
    text = " ".join(doc[:decl].replace("\n *", " ").split())
    for word in ("THE RECORD.", "(len << 4) | op", "(run_node, run_len)", "node id plus one", "INVARIANTS", "sum to L",
                 "out_counts[..][0..3]", "LOSSLESS.", "InsBegin", "ALIGNMENT INDEX.", "a = r * S' + s", "S' = max(n_samples, 1)",
                 "self-loop taken twice is two runs of length 1", "0 CIGAR words and 0 walk runs", "out == NULL",
                 "*out left as it was", "has no knob"):
        assert word in text, word


def test_library_exports_them():
    lib = _ffi_align.lib()
    for name in SIGNATURES:
        assert hasattr(lib, name), name
    # NULL model / reads / mappings: refused, nothing dereferenced; NULL handles are empty
    assert lib.phmm_run_with_mapping_alignments(None, None, None, 0, 1, None, None, None, None) == _ffi.PHMM_EINVAL
    assert lib.phmm_alignments_count(None) == 0 and lib.phmm_alignments_total_ops(None) == 0
    assert lib.phmm_alignments_total_runs(None) == 0
    assert lib.phmm_alignments_export(None, None, None, None, None, None) == _ffi.PHMM_EINVAL
    lib.phmm_alignments_destroy(None)
    assert (_ffi_align.PHMM_ALN_INS, _ffi_align.PHMM_ALN_DEL, _ffi_align.PHMM_ALN_EQ, _ffi_align.PHMM_ALN_DIFF) == (1, 2, 7, 8)


def test_python_binding():
    fn = getattr(D.PHMMModel, "run_with_mapping_alignments", None)
    assert callable(fn)
    sig = inspect.signature(fn).parameters
    assert list(sig) == ["self", "reads", "mappings", "n_samples", "seed"]
    assert sig["n_samples"].default == 0 and sig["seed"].default == 0
    for word in ("best path", "sampled", "path_logp", "counts", "Alignments"):
        assert word in fn.__doc__, word
    for method in ("arrays", "cigar", "cigar_string", "walk", "nodes", "states"):
        assert callable(getattr(D.Alignments, method, None)), method
    assert callable(D.formats.write_alignments) and callable(D.formats.read_alignments)
    assert list(inspect.signature(D.formats.write_alignments).parameters)[1:] == ["alignments", "logp", "names"]


def test_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "phmm_run_with_mapping_alignments" in _read(doc), doc
    assert "Alignment records over the lists" in _read("DESIGN.md")
    rust = _read("integration", "rust", "amd_sys.rs")
    for name in SIGNATURES:
        assert name in rust, name
    assert os.path.exists(os.path.join(ROOT, "tools", "alignments_time.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "alignments.txt"))
