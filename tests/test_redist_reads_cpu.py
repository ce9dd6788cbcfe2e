"""Each read's redistributed label without a GPU: utree_redist_reads_format (csrc/redist.c) against tests/redist_reads_ref.py on label sets built
with utree_ctr_from_memory, the ABI surface, the request's new field and its argument checks, and redist_reads_ref itself against figures
fixed beforehand so that the GPU tests (tests/test_gpu_redist_reads.py) compare against something pinned."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import redist_reads_ref
import util
from test_coverage_cpu import db_with
from test_redist_cpu import reference_sets
from test_search_request_cpu import CTR, DEV, PRM, run
from utree_amd import lib

NONE = 0xFFFFFFFF
LABELS = [b"k__A;p__B;c__C", b"", b"k__Q x", b";k__Z"]
FAIL = C.c_size_t(-1).value


def fmt(names, label, ncand, labels=LABELS, cap=None, slack=64):
    """utree_redist_reads_format on hand-made rows; label: index or None.  -> (return value, output with `slack` guard bytes behind cap, want)"""
    db = db_with(labels)
    name_len = np.array([len(n) for n in names], dtype=np.uint32)
    name_off = np.concatenate([[0], np.cumsum(name_len.astype(np.uint64))[:-1]]).astype(np.uint64)
    hb = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
    lab = np.array([NONE if l is None else l for l in label], dtype=np.uint32)
    nc = np.array(ncand, dtype=np.uint32)
    want = redist_reads_ref.reads_file(names, [l if l is not None and l < len(labels) else None for l in label], ncand, labels)
    if cap is None:
        cap = len(want)
    out = np.full(cap + slack, 0xA5, dtype=np.uint8)
    r = lib.load().utree_redist_reads_format(db._h, hb.ctypes.data, name_off.ctypes.data, name_len.ctypes.data, lab.ctypes.data, nc.ctypes.data,
                                             len(names), out.ctypes.data, cap)
    return r, out, want


NAMES = [b"read/1", b"two words", b"skipped", b"r4", b"", b"last"]
LABEL = [0, 2, None, 1, 3, 0]
NCAND = [1, 15, 0, 2, 4294967295, 3]


def test_format_equals_the_reference():
    r, out, want = fmt(NAMES, LABEL, NCAND)
    assert want == (b"read/1\tk__A;p__B;c__C\t1\n" b"two words\tk__Q x\t15\n" b"r4\t\t2\n" b"\t;k__Z\t4294967295\n" b"last\tk__A;p__B;c__C\t3\n")
    assert r == len(want) and out[:r].tobytes() == want             # cap exactly enough
    assert (out[r:] == 0xA5).all()
    assert b"skipped" not in want                                   # label 0xFFFFFFFF: no line
    assert want.split(b"\n")[2] == b"r4\t\t2"                       # an empty label text is a whole label text


def test_format_nothing_to_print():
    r, out, want = fmt([b"a", b"b"], [None, None], [0, 0])
    assert r == 0 and want == b""
    r, out, want = fmt([], [], [])
    assert r == 0


def test_format_refuses_a_label_the_database_does_not_have():
    for bad in (len(LABELS), len(LABELS) + 7, 0xFFFFFFFE):
        r, out, _ = fmt([b"a", b"b"], [0, bad], [1, 1], cap=4096)
        assert r == FAIL
        assert (out[4096:] == 0xA5).all()


def test_format_cap_too_small_writes_nothing_behind_cap():
    _, _, want = fmt(NAMES, LABEL, NCAND)
    for cap in list(range(0, 40)) + [len(want) - 1]:
        r, out, _ = fmt(NAMES, LABEL, NCAND, cap=cap)
        assert r == FAIL, cap
        assert (out[cap:] == 0xA5).all(), cap
    r, out, _ = fmt(NAMES, LABEL, NCAND, cap=len(want) + 1)
    assert r == len(want)


# ---- the ABI surface ------------------------------------------------------------------------------------------------------------------
NEW = ("utree_redist_classify_batch_keys", "utree_redist_assign", "utree_redist_reads_format")


def test_abi_surface():
    header = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SYMBOLS and getattr(L, name) is not None, name
    assert "#define UTREE_ABI_VERSION 4\n" in header and L.utree_abi_version() == 4
    assert re.search(r"#define\s+UTREE_REDIST_KEY_NONE\s+0xFFFFFFFFu", header) and lib.REDIST_KEY_NONE == NONE
    assert lib.SearchRequest._fields_[-1][0] == "redistribute_reads_path"


# ---- the request ----------------------------------------------------------------------------------------------------------------------
READS = dict(redistribute_reads_path=b"/nonexistent/q.tsv")
ALIGN = C.alignment(lib.SearchRequest)
OLD_SIZE = (lib.SearchRequest.redistribute_reads_path.offset + ALIGN - 1) // ALIGN * ALIGN


def test_request_sizes():
    assert C.sizeof(lib.SearchRequest) == 128 and OLD_SIZE == 120     # this target's: the header's comment names them


@pytest.mark.parametrize("case", [dict(rank=C.pointer(PRM), **READS), dict(max_passes=1001, **READS),
                                  dict(rank=C.pointer(PRM), max_passes=5, **READS)])
def test_request_refusals_come_before_the_handles(case):
    assert run(**case) == lib.E_ARG


def test_old_size_request_is_accepted_and_checked():
    """a caller built before the field: its size passes, and the checks behind the size check run on its fields"""
    for bad in (dict(mates_path=b"/nonexistent/m.fa", interleaved=1), dict(input_format=-1), dict(redistribute_path=b"/nonexistent/r.tsv", max_passes=1001),
                dict(n_dev=0)):
        assert run(size=OLD_SIZE, **bad) == lib.E_ARG
    for size in (OLD_SIZE - 8, OLD_SIZE + 4, OLD_SIZE - 1):
        assert run(size=size) == lib.E_ARG
    # the old layout's bytes end in front of the field: what stands behind them is not read as a path
    req = lib.SearchRequest(reads_path=None, out_path=b"/nonexistent/out.txt", rank=C.pointer(PRM), **READS)
    req.size = OLD_SIZE
    arr = (C.c_void_p * 1)(C.addressof(DEV))
    assert lib.load().utree_search_run(C.addressof(CTR), arr, 1, C.byref(req), None) == lib.E_ARG     # (reads_path NULL)


# ---- the yardstick itself, pinned ---------------------------------------------------------------------------------------------------
# fixture, RC, reads -> reads whose redistributed label text (at convergence) is not column 2 of the reference's output line
MOVED = {("toy", 0, 4000): 1899, ("vote", 0, 4000): 2720}
_ASSIGN = {}


def reference_assign(name, rc, n, max_passes):
    """(labels, ncand, texts) of a fixture's first n reads as redist_reads_ref gives them (cached: the GPU tests use them too)"""
    key = (name, rc, n, max_passes)
    if key not in _ASSIGN:
        sets, texts = reference_sets(name, rc, n)
        labels, ncand, _ = redist_reads_ref.assign(sets, n, max_passes)
        _ASSIGN[key] = (labels, ncand, texts)
    return _ASSIGN[key]


@pytest.mark.parametrize("name,rc,n", sorted(MOVED))
def test_yardstick_is_pinned(name, rc, n):
    labels, ncand, texts = reference_assign(name, rc, n, 100)
    names = util.parse_fasta(util.fixture_bytes(name + "_reads.fa.gz"))[0][:n]
    out = util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
    col2 = {line.split(b"\t")[0]: line.split(b"\t")[1] for line in out.split(b"\n") if line}
    # a read has a label exactly when the reference prints a line for it
    assert all((l is not None) == (nm in col2) for nm, l in zip(names, labels))
    moved = sum(1 for nm, l in zip(names, labels) if l is not None and texts[l] != col2[nm])
    assert moved == MOVED[(name, rc, n)] > 0
    assert all((c == 0) == (l is None) for l, c in zip(labels, ncand))
    # after 1 pass, after 3 passes and at convergence: three different per-read results (else the pass-cap tests would show nothing)
    by = [reference_assign(name, rc, n, mp)[0] for mp in (1, 3, 100)]
    assert by[0] != by[1] and by[1] != by[2] and by[0] != by[2]


def test_reads_file_of_the_reference():
    labels, ncand, texts = reference_assign("toy", 0, 4000, 100)
    names = util.parse_fasta(util.fixture_bytes("toy_reads.fa.gz"))[0][:4000]
    f = redist_reads_ref.reads_file(names, labels, ncand, texts)
    lines = f.split(b"\n")
    assert lines[-1] == b"" and len(lines) - 1 == sum(l is not None for l in labels) == 3402
    assert all(len(line.split(b"\t")) == 3 for line in lines[:-1])
