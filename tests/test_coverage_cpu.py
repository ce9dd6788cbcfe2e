"""utree_coverage_write (csrc/coverage.c) against the contract in tests/coverage_ref.py, without a GPU: entries as the device read-back
gives them, one (label, db_kmers, covered, hits) per label, on label sets built with utree_ctr_from_memory.  And coverage_ref itself
against figures fixed beforehand -- the totals of every GG fixture, the sum of the third column of the genuine reference's committed
output, the SHA-256 of every coverage file -- so that the GPU tests compare against something pinned."""
import hashlib

import numpy as np
import pytest

import coverage_ref
import util
from utree_amd import lib
from utree_amd.search import COVERAGE_ENTRY_DTYPE, CtrDB, write_coverage

_DBS = {}


def db_with(labels, I=2):
    key = (tuple(labels), I)
    if key not in _DBS:
        text = b"".join(l + b"\t1\n" for l in labels)
        binix = np.zeros((1 << 24) + 1, dtype=np.uint64)
        binix[-1] = 1                                            # one node: the labels are what matters here
        _DBS[key] = CtrDB.from_memory(8, I, 1, binix, None, text)
    return _DBS[key]


def check(tmp_path, labels, figures, n_reads, I=2, extra=()):
    """figures: {label index: (db_kmers, covered, hits)}; every label gets an entry, as utree_coverage_read gives them.  extra: further
    entries (label, db, cov, hits) as a second device would add them."""
    db = db_with(labels, I)
    rows = [(i, 0) + tuple(figures.get(i, (0, 0, 0))) for i in range(len(labels))] + [(l, 0, a, b, c) for l, a, b, c in extra]
    e = np.array(rows, dtype=COVERAGE_ENTRY_DTYPE)
    path = tmp_path / "c.tsv"
    write_coverage(db, e, n_reads, str(path))
    tot = [[0, 0, 0] for _ in labels]
    for l, _, a, b, c in rows:
        tot[l][0] += a; tot[l][1] += b; tot[l][2] += c
    want = coverage_ref.coverage_file(*(np.array([t[q] for t in tot], dtype=object) for q in range(3)), labels, n_reads)
    assert path.read_bytes() == want
    return want


LABELS = [b"k__A;p__B;c__C", b"k__A;p__B;c__D", b"k__A;p__E", b"k__A;p__B", b"k__A;p__Streptomyces;g__x", b";k__Z;p__Y",
          b"k__A;p__B;c__C;o__", b"k__Q"]
HEAD2 = b"# taxon\tdb_kmers\tcovered\thits\tclade_db_kmers\tclade_covered\tclade_hits\n"


def test_unhit_siblings_show_in_clade_db_kmers_only(tmp_path):
    got = check(tmp_path, LABELS, {0: (100, 40, 900), 1: (50, 0, 0), 2: (30, 0, 0), 3: (7, 0, 0), 6: (5, 0, 0), 7: (11, 0, 0)}, 20)
    lines = got.split(b"\n")
    assert lines[0] == b"# reads\t20\thits\t900\tcovered\t40\tdb_kmers\t203" and lines[1] + b"\n" == HEAD2
    # rows: the hit label and its prefixes only; k__A counts every label below it, k__A;p__B is a prefix AND an unhit label's text
    assert lines[2:6] == [b"k__A\t0\t0\t0\t192\t40\t900", b"k__A;p__B\t7\t0\t0\t162\t40\t900", b"k__A;p__B;c__C\t100\t40\t900\t105\t40\t900", b""]


def test_label_that_is_a_prefix_of_another(tmp_path):
    got = check(tmp_path, LABELS, {0: (10, 2, 3), 3: (7, 7, 70), 6: (5, 1, 1)}, 9)
    assert b"\nk__A;p__B\t7\t7\t70\t22\t10\t74\n" in got and b"\nk__A;p__B;c__C\t10\t2\t3\t15\t3\t4\n" in got
    assert b"\nk__A;p__B;c__C;o__\t5\t1\t1\t5\t1\t1\n" in got


def test_labels_with_equal_text_are_one_row(tmp_path):
    # entries of equal text -- the same label from two devices (a .ctr's label lines of equal text are one label) -- are added up
    got = check(tmp_path, LABELS, {0: (10, 2, 3), 7: (11, 5, 6)}, 9, extra=[(0, 10, 1, 2), (7, 0, 1, 1)])
    assert got.count(b"\nk__A;p__B;c__C\t") == 1 and b"\nk__A;p__B;c__C\t20\t3\t5\t20\t3\t5\n" in got
    assert b"\nk__Q\t11\t6\t7\t11\t6\t7\n" in got


def test_label_that_starts_with_a_semicolon(tmp_path):
    got = check(tmp_path, LABELS, {5: (4, 3, 8), 7: (11, 0, 0)}, 4)
    lines = got.split(b"\n")
    assert lines[2] == b"\t0\t0\t0\t4\t3\t8"                       # the empty prefix sorts first: a line that begins with a TAB
    assert lines[3] == b";k__Z\t0\t0\t0\t4\t3\t8" and lines[4] == b";k__Z;p__Y\t4\t3\t8\t4\t3\t8" and lines[5] == b""


def test_no_hits_at_all(tmp_path):
    got = check(tmp_path, LABELS, {0: (10, 0, 0), 1: (3, 0, 0)}, 1234)
    assert got == b"# reads\t1234\thits\t0\tcovered\t0\tdb_kmers\t13\n" + HEAD2
    got = check(tmp_path, LABELS, {}, 0)
    assert got == b"# reads\t0\thits\t0\tcovered\t0\tdb_kmers\t0\n" + HEAD2


def test_counts_beyond_32_bits(tmp_path):
    big = (1 << 32) + 5
    got = check(tmp_path, LABELS, {0: (3 * big, big, 7 * big), 1: (big, big - 1, big)}, 9 * big)
    assert b"\nk__A;p__B\t0\t0\t0\t%d\t%d\t%d\n" % (4 * big, 2 * big - 1, 8 * big) in got
    assert got.startswith(b"# reads\t%d\thits\t%d\t" % (9 * big, 8 * big))


def test_u32_labels(tmp_path):
    labels = [b"k__L%d;p__M%d;c__N%d" % (i % 7, i % 3, i) for i in range(300)]
    rng = np.random.default_rng(3)
    fig = {}
    for i in range(300):
        db = int(rng.integers(1, 1000))
        cov = int(rng.integers(0, db + 1)) if i % 3 else 0
        fig[i] = (db, cov, cov * int(rng.integers(1, 9)))
    check(tmp_path, labels, fig, 10_000, I=4)


def test_bad_label_and_unwritable_path(tmp_path):
    db = db_with(LABELS)
    with pytest.raises(lib.UtreeError):
        write_coverage(db, np.array([(len(LABELS), 0, 1, 1, 1)], dtype=COVERAGE_ENTRY_DTYPE), 1, str(tmp_path / "c"))
    with pytest.raises(lib.UtreeError):
        write_coverage(db, np.array([(0, 0, 1, 1, 1)], dtype=COVERAGE_ENTRY_DTYPE), 1, str(tmp_path / "no" / "such" / "dir"))
    with pytest.raises(lib.UtreeError):                                   # a file that takes no bytes
        write_coverage(db, np.array([(0, 0, 1, 1, 1)], dtype=COVERAGE_ENTRY_DTYPE), 1, "/dev/full")
    assert lib.E_COVERAGE == 13 and b"coverage" in lib.load().utree_strerror(13)


# ---- the yardstick itself, pinned ---------------------------------------------------------------------------------------------------
# fixture, RC -> reads, n_nodes, hits (= the sum of column 3 of the reference's output), covered, rows, bytes, SHA-256 of the coverage file
PINNED = {
    ("toy", 0): (10000, 24117, 35457, 12822, 1751, 111577, "0d65e0183556df096f42b25cc8c183906ee54378be92ca178a89c716be970f1a"),
    ("toy", 1): (10000, 24117, 36211, 12978, 1752, 111684, "197b287ac3d58cc72000a0f3805db17c09d002c50b886871a7f77d934229f0d2"),
    ("k64", 0): (3000, 9364, 9613, 5845, 523, 30561, "c7c5926f5d62641e0a3c2753f46fff3b75e9a8c8673fa6845dd35149057e2d85"),
    ("k64", 1): (3000, 9364, 9829, 5936, 523, 30569, "72a8a8c024b1c76be2a9445cd232a2d25b7f0ca9f2ae00457fa6f92e652b7250"),
    ("ix32", 0): (3000, 6060, 10938, 4364, 517, 30163, "6755c955a5ddb268ae9b018784bcff1b25e7f315767792eb0b2f4cc907dee7de"),
    ("ix32", 1): (3000, 6060, 11189, 4411, 517, 30167, "fc1082108a75007b9e0f4d07dd4a676ebbd89dbd210379c5de6b22c03a2019e3"),
    ("k64ix32", 0): (3000, 9913, 10442, 6184, 503, 29275, "07553ef565d73bc70ca62f255ecc0b08d1c3986d83dcec03ed764b3ff0ca6aae"),
    ("k64ix32", 1): (3000, 9913, 10629, 6254, 503, 29280, "3e166bbcaade0d2f4bd33bd762d85ad7ccb32ef99d0b826c9103f3ca740a21a6"),
    ("k16", 0): (3000, 38217, 95902, 32886, 439, 27023, "40ef927d1be30ba30ebe6096ceaea5e0a49ce856a07923c7e165c8dbf0ec4275"),
    ("k16", 1): (3000, 38217, 97529, 33040, 439, 27025, "ad3a31e1ecacce0770d4da4436bb620dd34e0f44a6768034e970e42e516cfbba"),
    ("vote", 0): (4021, 780, 34488, 528, 202, 13031, "b9a95a743f17dcffb9f280c54b7527fecb30e35dd42ec99a5d69435daf59f2fd"),
    ("kat", 0): (7040, 1408, 1418, 1408, 41, 1336, "84567c19f06f900bd36129acfb436faa11455fe0dd49ee0fccb7989fd41a673c"),
    ("katq", 0): (7050, 1409, 1419, 1409, 41, 1336, "3714702349cae74cf53042675af145327be7ca21e14ad74a7350813994acaa7b"),
    ("katq2", 0): (162, 50, 49, 49, 22, 627, "c6e05a8ab2c505944c62b11d75d00a471d889f138eaf1e5a4f91e0ae9c7ad153"),
    ("generic", 0): (7040, 1408, 1383, 1373, 41, 1336, "f5ff0e777b378936f7c4c3fd58d4efc8c47ce76ef6159eecf12be3605053139c"),
}
_FILES = {}


def fixture_seqs(name):
    data = util.fixture_bytes(util.READS_OF.get(name, name) + "_reads.fa.gz")
    _, off, ln = util.parse_fasta(data)
    return [data[int(o):int(o) + int(l)] for o, l in zip(off, ln)]


def reference_file(name, rc):
    """(coverage file bytes, db, cov, hits) of a fixture as coverage_ref gives them (cached: the GPU tests use them too)"""
    if (name, rc) not in _FILES:
        seqs = fixture_seqs(name)
        db, cov, hits, texts = coverage_ref.coverage_counts(util.fixture_ctr(name), seqs, rc)
        _FILES[(name, rc)] = (coverage_ref.coverage_file(db, cov, hits, texts, len(seqs)), db, cov, hits)
    return _FILES[(name, rc)]


def reference_output_found(name, rc):
    """the sum of the third column of the genuine reference's committed per-read output"""
    out = util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
    return sum(int(line.split(b"\t")[2]) for line in out.split(b"\n") if line)


@pytest.mark.parametrize("name,rc", sorted(PINNED))
def test_yardstick_is_pinned(name, rc):
    reads, n_nodes, hits, covered, rows, size, sha = PINNED[(name, rc)]
    data, db, cov, h = reference_file(name, rc)
    assert len(fixture_seqs(name)) == reads
    assert int(db.sum()) == n_nodes and int(h.sum()) == hits and int(cov.sum()) == covered
    assert (cov <= db).all() and (cov <= h).all()
    assert reference_output_found(name, rc) == hits                         # ties the figure to the reference, not to this project
    assert data.count(b"\n") - 2 == rows and len(data) == size and hashlib.sha256(data).hexdigest() == sha
    assert data.startswith(b"# reads\t%d\thits\t%d\tcovered\t%d\tdb_kmers\t%d\n" % (reads, hits, covered, n_nodes) + HEAD2)
