"""utree_profile_write (csrc/profile.c) against the contract in tests/profile_ref.py, without a GPU: entries as the device read-back
gives them, (label, cut, reads), on label sets built with utree_ctr_from_memory."""
import numpy as np
import pytest

from utree_amd import lib
from utree_amd.search import CtrDB, PROFILE_ENTRY_DTYPE, write_profile
from profile_ref import profile_from_taxa

_DBS = {}


def db_with(labels, I=2):
    key = (tuple(labels), I)
    if key not in _DBS:
        text = b"".join(l + b"\t1\n" for l in labels)
        binix = np.zeros((1 << 24) + 1, dtype=np.uint64)
        binix[-1] = 1                                            # one node: the labels are what matters here
        _DBS[key] = CtrDB.from_memory(8, I, 1, binix, None, text)
    return _DBS[key]


def text_of(labels, label, cut):
    lab = labels[label]
    return b"" if cut == -1 else lab if cut < 0 else lab[:cut]


def check(tmp_path, labels, entries, n_reads, I=2):
    db = db_with(labels, I)
    e = np.array(entries, dtype=PROFILE_ENTRY_DTYPE)
    path = tmp_path / "p.tsv"
    write_profile(db, e, n_reads, str(path))
    taxa = [text_of(labels, l, c) for l, c, r in entries for _ in range(r)]
    want = profile_from_taxa(taxa, n_reads)
    assert path.read_bytes() == want
    return want


LABELS = [b"k__A;p__B;c__C", b"k__A;p__B;c__D", b"k__A;p__E", b"k__A;p__B", b"k__A;p__Streptomyces;g__x", b";k__Z;p__Y",
          b"k__A;p__B;c__C;o__"]


def test_shared_prefixes(tmp_path):
    got = check(tmp_path, LABELS, [(0, -2, 5), (1, -2, 3), (2, -2, 2), (3, -2, 7)], 20)
    assert b"k__A\t0\t17\n" in got and b"k__A;p__B\t7\t15\n" in got
    assert got.startswith(b"# reads\t20\tclassified\t17\tunclassified\t3\n# taxon\tassigned\tclade\n")


def test_mid_word_cuts(tmp_path):
    got = check(tmp_path, LABELS, [(4, len(b"k__A;p__Strepto"), 4), (4, -2, 1), (0, 6, 2)], 9)
    assert b"k__A;p__Strepto\t4\t4\n" in got and b"k__A;p\t2\t2\n" in got


def test_cut_at_full_length_merges_with_whole_label(tmp_path):
    got = check(tmp_path, LABELS, [(0, len(LABELS[0]), 3), (0, -2, 4), (0, 1000, 1), (3, 9, 2)], 10)
    assert b"k__A;p__B;c__C\t8\t8\n" in got
    # label 3 cut to 9 bytes is "k__A;p__B" = label 3's whole text: one row
    assert got.count(b"\nk__A;p__B\t") == 1


def test_empty_taxon(tmp_path):
    got = check(tmp_path, LABELS, [(0, -1, 6), (2, -1, 1), (0, 0, 2), (1, -2, 1)], 12)
    lines = got.split(b"\n")
    assert lines[2] == b"\t9\t9"                                 # the empty taxon sorts first and prints as a line that begins with a TAB


def test_label_that_starts_with_a_semicolon(tmp_path):
    got = check(tmp_path, LABELS, [(5, -2, 3), (5, 5, 1)], 4)
    assert b"\n\t0\t4\n" in got and b"\n;k__Z\t1\t4\n" in got


def test_u32_labels(tmp_path):
    labels = [b"k__L%d;p__M%d;c__N%d" % (i % 7, i % 3, i) for i in range(300)]
    entries = [(i, -2, i % 5 + 1) for i in range(0, 300, 3)] + [(i, 8, 2) for i in range(1, 300, 11)]
    check(tmp_path, labels, entries, 10_000, I=4)


def test_entries_split_across_devices(tmp_path):
    rng = np.random.default_rng(5)
    entries = []
    for dev in range(4):                                         # the same keys from every device, and device-only ones
        for l in range(len(LABELS)):
            entries.append((l, -2, int(rng.integers(1, 50))))
            entries.append((l, int(rng.integers(0, 20)), int(rng.integers(1, 9))))
        entries.append((dev, -1, 3))
    n = sum(r for _, _, r in entries) + 77
    check(tmp_path, LABELS, entries, n)


def test_zero_classified_reads(tmp_path):
    got = check(tmp_path, LABELS, [], 1234)
    assert got == b"# reads\t1234\tclassified\t0\tunclassified\t1234\n# taxon\tassigned\tclade\n"
    got = check(tmp_path, LABELS, [], 0)
    assert got.startswith(b"# reads\t0\t")


def test_bad_label_and_unwritable_path(tmp_path):
    db = db_with(LABELS)
    with pytest.raises(lib.UtreeError):
        write_profile(db, np.array([(len(LABELS), -2, 1)], dtype=PROFILE_ENTRY_DTYPE), 1, str(tmp_path / "p"))
    with pytest.raises(lib.UtreeError):
        write_profile(db, np.array([(0, -2, 1)], dtype=PROFILE_ENTRY_DTYPE), 1, str(tmp_path / "no" / "such" / "dir"))
