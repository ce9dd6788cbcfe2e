"""utree_redist_write (csrc/redist.c) against the contract in tests/redist_ref.py, without a GPU: entries as utree_redist_solve gives them, on
label sets built with utree_ctr_from_memory.  The ABI surface.  And redist_ref itself against figures fixed beforehand -- reads classified,
ambiguous, distinct sets, passes and every pass's `changes` of the fixtures' first reads -- so that the GPU tests compare against something
pinned."""
import hashlib
import os
import re

import numpy as np
import pytest

import redist_ref
import util
from test_coverage_cpu import LABELS, db_with, fixture_seqs
from utree_amd import lib
from utree_amd.search import REDIST_ENTRY_DTYPE, write_redistribution

HEAD2 = b"# taxon\tassigned\tunique\tclade_assigned\tclade_unique\n"


def check(tmp_path, labels, figures, n_reads, ambiguous, passes, I=2, extra=()):
    """figures: {label index: (assigned, unique)}; extra: further entries (label, assigned, unique) as a second solve would add them"""
    db = db_with(labels, I)
    rows = [(l, 0, a, u) for l, (a, u) in sorted(figures.items())] + [(l, 0, a, u) for l, a, u in extra]
    path = tmp_path / "r.tsv"
    write_redistribution(db, np.array(rows, dtype=REDIST_ENTRY_DTYPE), n_reads, ambiguous, passes, str(path))
    assigned, unique = {}, {}
    for l, _, a, u in rows:
        assigned[l] = assigned.get(l, 0) + a
        unique[l] = unique.get(l, 0) + u
    want = redist_ref.redist_file(assigned, unique, labels, n_reads, ambiguous, passes)
    assert path.read_bytes() == want
    return want


def test_header_rows_and_a_label_that_is_a_prefix_of_another(tmp_path):
    got = check(tmp_path, LABELS, {0: (10, 4), 3: (7, 7), 6: (5, 1), 1: (0, 0)}, 30, 9, 6)
    lines = got.split(b"\n")
    assert lines[0] == b"# reads\t30\tclassified\t22\tunclassified\t8\tambiguous\t9\tpasses\t6" and lines[1] + b"\n" == HEAD2
    assert lines[2:7] == [b"k__A\t0\t0\t22\t12", b"k__A;p__B\t7\t7\t22\t12", b"k__A;p__B;c__C\t10\t4\t15\t5", b"k__A;p__B;c__C;o__\t5\t1\t5\t1", b""]


def test_rows_are_keyed_on_assigned(tmp_path):
    # a label that lost all its ambiguous reads has no row of its own, and none for its prefixes
    got = check(tmp_path, LABELS, {0: (10, 4), 7: (0, 0), 4: (0, 0)}, 10, 6, 2)
    assert b"k__Q" not in got and b"Streptomyces" not in got and got.count(b"\n") == 2 + 3


def test_entries_of_equal_text_are_one_row(tmp_path):
    # the same label from a second device, or two indices with one text: added up when the file is written
    got = check(tmp_path, LABELS, {0: (10, 2), 7: (11, 5)}, 40, 3, 1, extra=[(0, 10, 1), (7, 0, 1)])
    assert got.count(b"\nk__A;p__B;c__C\t") == 1 and b"\nk__A;p__B;c__C\t20\t3\t20\t3\n" in got
    assert b"\nk__Q\t11\t6\t11\t6\n" in got
    assert got.startswith(b"# reads\t40\tclassified\t31\tunclassified\t9\tambiguous\t3\tpasses\t1\n")


def test_label_that_starts_with_a_semicolon_and_nothing_assigned(tmp_path):
    got = check(tmp_path, LABELS, {5: (4, 3)}, 4, 1, 2)
    lines = got.split(b"\n")
    assert lines[2] == b"\t0\t0\t4\t3" and lines[3] == b";k__Z\t0\t0\t4\t3" and lines[4] == b";k__Z;p__Y\t4\t3\t4\t3" and lines[5] == b""
    got = check(tmp_path, LABELS, {}, 1234, 0, 1)
    assert got == b"# reads\t1234\tclassified\t0\tunclassified\t1234\tambiguous\t0\tpasses\t1\n" + HEAD2


def test_u32_labels_and_counts_beyond_32_bits(tmp_path):
    labels = [b"k__L%d;p__M%d;c__N%d" % (i % 7, i % 3, i) for i in range(300)]
    rng = np.random.default_rng(5)
    big = (1 << 32) + 5
    fig = {}
    for i in range(300):
        u = int(rng.integers(0, 1000)) if i % 3 else 0
        fig[i] = (u + (int(rng.integers(0, 50)) * big if i % 4 == 0 else 0), u)
    got = check(tmp_path, labels, fig, 10_000 * big, 77 * big, 100, I=4)
    assert got.startswith(b"# reads\t%d\tclassified\t%d\t" % (10_000 * big, sum(a for a, _ in fig.values())))


def test_bad_label_and_unwritable_path(tmp_path):
    db = db_with(LABELS)
    with pytest.raises(lib.UtreeError) as e:
        write_redistribution(db, np.array([(len(LABELS), 0, 1, 1)], dtype=REDIST_ENTRY_DTYPE), 1, 0, 1, str(tmp_path / "c"))
    assert e.value.code == lib.E_ARG
    for path in (str(tmp_path / "no" / "such" / "dir"), "/dev/full"):        # a path that cannot be created, a file that takes no bytes
        with pytest.raises(lib.UtreeError) as e:
            write_redistribution(db, np.array([(0, 0, 1, 1)], dtype=REDIST_ENTRY_DTYPE), 1, 0, 1, path)
        assert e.value.code == lib.E_IO


# ---- the ABI surface ------------------------------------------------------------------------------------------------------------------
NAMES = ("utree_redist_create", "utree_redist_reset", "utree_redist_free", "utree_redist_classify_batch", "utree_redist_read",
         "utree_redist_merge", "utree_redist_solve", "utree_redist_write", "utree_search_file_redistribute")


def test_abi_surface():
    header = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SYMBOLS and getattr(L, name) is not None, name
    assert "#define UTREE_ABI_VERSION 4\n" in header and L.utree_abi_version() == 4
    assert L.utree_strerror(15) == b"unknown error"                     # no new error code: the redistribution's failure is UTREE_E_PROFILE
    assert lib.E_PROFILE == 12


# ---- the yardstick itself, pinned ---------------------------------------------------------------------------------------------------
# fixture, RC, reads -> classified, ambiguous, distinct multi-label sets, largest set, passes, every pass's changes
PINNED = {
    ("toy", 0, 4000): (3402, 1252, 1179, 15, 6, [3559, 198, 42, 14, 2, 0]),
    ("toy", 1, 4000): (3473, 1277, 1202, 15, 6, [3651, 196, 40, 18, 6, 0]),
    ("vote", 0, 4000): (4000, 991, 857, 5, 7, [1218, 104, 34, 14, 10, 2, 0]),
    ("k64", 0, 3000): (2369, 101, 90, 4, 2, [112, 0]),
    ("ix32", 1, 3000): (2628, 629, 532, 12, 5, [1247, 96, 12, 2, 0]),
    ("k64ix32", 1, 3000): (2444, 143, 123, 7, 2, [161, 0]),
    ("k16", 1, 3000): (2704, 58, 55, 3, 2, [60, 0]),
}
_SETS = {}


def reference_sets(name, rc, n=4000):
    """(per-read candidate sets, label texts) of a fixture's first n reads as redist_ref gives them (cached: the GPU tests use them too)"""
    if (name, rc, n) not in _SETS:
        _SETS[(name, rc, n)] = redist_ref.candidate_sets(util.fixture_ctr(name), fixture_seqs(name)[:n], rc)
    return _SETS[(name, rc, n)]


@pytest.mark.parametrize("name,rc,n", sorted(PINNED))
def test_yardstick_is_pinned(name, rc, n):
    classified, ambiguous, multi, largest, passes, changes = PINNED[(name, rc, n)]
    sets, texts = reference_sets(name, rc, n)
    assert len(sets) == n
    ms = redist_ref.multiset(sets)
    assert sum(ms.values()) == classified and sum(1 for s in ms if len(s) > 1) == multi and max(map(len, ms)) == largest
    a, u, p, amb, ch = redist_ref.solve(sets, n)
    assert (p, amb, ch) == (passes, ambiguous, changes)
    assert sum(a.values()) == classified and sum(u.values()) == classified - ambiguous
    # ties the figure to the reference, not to this project: the reads with a candidate are the reads the reference prints a line for
    out = util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
    names = util.parse_fasta(util.fixture_bytes(name + "_reads.fa.gz"))[0][:n]
    printed = {line.split(b"\t")[0] for line in out.split(b"\n") if line}
    assert len(set(names)) == n and sum(1 for nm in names if nm in printed) == classified


@pytest.mark.parametrize("name", ["toy", "vote"])
def test_the_pass_cap_changes_the_table(name):
    """after 1 pass, after 3 passes and at convergence: three different tables (else the pass-cap tests would show nothing)"""
    sets, texts = reference_sets(name, 0)
    tables = [redist_ref.solve(sets, len(sets), mp)[0] for mp in (1, 3, 100)]
    assert tables[0] != tables[1] and tables[1] != tables[2] and tables[0] != tables[2]
    assert [redist_ref.solve(sets, len(sets), mp)[2] for mp in (1, 3, 100)] == [1, 3, PINNED[(name, 0, 4000)][4]]


def test_ix32_differs_after_one_pass_only():
    sets, texts = reference_sets("ix32", 1, 3000)
    tables = [redist_ref.solve(sets, len(sets), mp)[0] for mp in (1, 3, 100)]
    assert tables[0] != tables[1] and tables[1] == tables[2]


def test_tie_break_and_final_evaluation():
    """win: the smallest file-order index among equal tallies; assigned is one more evaluation under T_P, not T_P itself"""
    sets = [(2, 5)] * 3 + [(5,)] * 1 + [(2,)] * 1 + [()] * 2
    a, u, p, amb, ch = redist_ref.solve(sets, len(sets), 1)
    assert (dict(a), dict(u), p, amb) == ({2: 4, 5: 1}, {5: 1, 2: 1}, 1, 3) and ch == [3]          # T0 = {2: 4, 5: 4}: the tie goes to 2
    sets = [(7, 3)] * 2 + [(7,)] * 5 + [(3,)] * 5
    assert dict(redist_ref.solve(sets, len(sets))[0]) == {3: 7, 7: 5}
