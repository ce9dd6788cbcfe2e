"""The per-sample taxon table without a GPU: the contract's own invariants (tests/samples_ref.py) on the GG golden outputs under synthetic
read names, and utree_samples_write (csrc/samples.c) on hand-made read-backs of several "devices" against that contract."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import util
from utree_amd import lib
from utree_amd.search import CtrDB, SAMPLES_CELL_DTYPE, SamplesReadback, write_samples
from profile_ref import fasta_names, profile_ref
import samples_ref as sr

GG = [("toy", 0), ("toy", 1), ("k64", 0), ("k64", 1), ("ix32", 0), ("ix32", 1), ("k64ix32", 0), ("k64ix32", 1), ("k16", 0), ("k16", 1),
      ("vote", 0), ("kat", 0), ("katq", 0), ("katq2", 0), ("generic", 0)]


@pytest.mark.parametrize("name,rc", GG)
@pytest.mark.parametrize("deal", ["round_robin", "blocks"])
def test_ref_invariants_on_golden_outputs(name, rc, deal):
    data = util.fixture_bytes(util.READS_OF.get(name, name) + "_reads.fa.gz")
    out = util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
    old = fasta_names(data)
    new = (sr.round_robin_names if deal == "round_robin" else sr.block_names)(len(old), sr.SEVEN)
    data2, out2 = sr.rename_reads(data, out, old, new)
    assert fasta_names(data2) == new and out2.count(b"\n") == out.count(b"\n")
    tab = sr.samples_ref(out2, new, len(new))
    N, G, S, ids, n, u, rows = sr.check_invariants(tab)
    assert N == len(new) and G == out.count(b"\n") and S == 7 and ids == sorted(sr.SEVEN)
    # a row sums to the taxon's `assigned` in the profile of the same run (the names do not reach the taxa: the original output's profile)
    prof = profile_ref(out, old, len(old)).split(b"\n")[2:-1]
    assigned = {}
    for ln in prof:
        f = ln.rsplit(b"\t", 2)
        if int(f[1]):
            assigned[f[0]] = int(f[1])
    assert {t: sum(r) for t, r in rows.items()} == assigned


_DBS = {}


def db_with(labels, I=2):
    key = (tuple(labels), I)
    if key not in _DBS:
        text = b"".join(l + b"\t1\n" for l in labels)
        binix = np.zeros((1 << 24) + 1, dtype=np.uint64)
        binix[-1] = 1                                            # one node: the labels are what matters here
        _DBS[key] = CtrDB.from_memory(8, I, 1, binix, None, text)
    return _DBS[key]


LABELS = [b"k__A;p__B;c__C", b"k__A;p__B;c__D", b"k__A;p__E", b"k__A;p__B", b"k__A;p__Streptomyces;g__x", b";k__Z;p__Y"]


def text_of(label, cut):
    lab = LABELS[label]
    return b"" if cut == -1 else lab if cut < 0 else lab[:cut]


def readback(ids, uncl, cells):
    """a device's read-back: ids in ITS order, its unclassified reads per sample, cells [(sample, label, cut, reads)]"""
    reads = list(uncl)
    for s, _, _, r in cells:
        reads[s] += r
    c = np.array([(s, l, cut, 0, r) for s, l, cut, r in cells], dtype=SAMPLES_CELL_DTYPE)
    return SamplesReadback(ids, reads, uncl, c, sum(reads))


def want_of(readbacks):
    """the contract on the reads those read-backs stand for"""
    ids, cls = [], []
    for rb in readbacks:
        for s, u in enumerate(rb.unclassified):
            ids += [rb.ids[s]] * int(u)
        for s, l, cut, _, r in rb.cells.tolist():
            for _ in range(r):
                cls.append((len(ids), text_of(l, cut)))
                ids.append(rb.ids[s])
    return sr.table_from(ids, cls, len(ids))


def test_write_merges_two_devices_by_text(tmp_path):
    # the same ids under other numbers; (label, cut) keys that print the same text; the empty id; ids with TAB, CR and backslash; the empty taxon
    a = readback([b"s2", b"", b"a\tb", b"s1"], [1, 0, 2, 0],
                 [(0, 0, -2, 5), (0, 3, -2, 2), (1, 0, 9, 1), (2, 2, -1, 3), (3, 0, len(LABELS[0]), 4), (3, 5, -2, 1), (1, 4, 15, 2)])
    b = readback([b"s1", b"c\\d\r", b"s2", b"ab", b"abc", b"a"], [0, 3, 1, 0, 0, 0],
                 [(0, 0, -2, 7), (0, 3, 9, 2), (2, 0, 1000, 1), (1, 1, -1, 2), (3, 2, -2, 1), (4, 2, -2, 2), (5, 2, 4, 3), (2, 5, 0, 4)])
    path = tmp_path / "t.tsv"
    write_samples(db_with(LABELS), [a, b], str(path))
    got = path.read_bytes()
    assert got == want_of([a, b])
    N, G, S, ids, n, u, rows = sr.check_invariants(got)
    assert ids == [b"", b"a", b"a\\tb", b"ab", b"abc", b"c\\\\d\\r", b"s1", b"s2"]        # bytewise, shorter first, escaped in print only
    assert got.split(b"\n")[4].startswith(b"\t")                                           # the empty taxon: a line that begins with the TAB
    assert rows[LABELS[0]][ids.index(b"s1")] == 11 and rows[b"k__A;p__B"][ids.index(b"s2")] == 2 and rows[b"k__A;p__B"][ids.index(b"s1")] == 2
    assert not any(b";k__Z" == t for t in rows)                                            # no ';'-prefix rows: only what a line prints


def test_write_one_device_and_order_of_taxa(tmp_path):
    a = readback([b"z", b"y"], [0, 0], [(0, 4, -2, 1), (0, 4, 4, 1), (1, 4, 15, 1), (1, 0, -2, 1)])
    path = tmp_path / "t.tsv"
    write_samples(db_with(LABELS), [a], str(path))
    got = path.read_bytes()
    assert got == want_of([a])
    assert [ln.split(b"\t")[0] for ln in got.split(b"\n")[4:-1]] == [b"k__A", b"k__A;p__B;c__C", b"k__A;p__Strepto", LABELS[4]]


def test_write_no_samples(tmp_path):
    path = tmp_path / "t.tsv"
    write_samples(db_with(LABELS), [readback([], [], [])], str(path))
    assert path.read_bytes() == b"# reads\t0\tclassified\t0\tunclassified\t0\tsamples\t0\n# taxon\n# reads\n# unclassified\n"
    write_samples(db_with(LABELS), [], str(path))
    assert path.read_bytes() == b"# reads\t0\tclassified\t0\tunclassified\t0\tsamples\t0\n# taxon\n# reads\n# unclassified\n"
    only_u = readback([b"q"], [9], [])
    write_samples(db_with(LABELS), [only_u, readback([], [], [])], str(path))
    assert path.read_bytes() == b"# reads\t9\tclassified\t0\tunclassified\t9\tsamples\t1\n# taxon\tq\n# reads\t9\n# unclassified\t9\n"


def test_write_refuses_figures_that_contradict_each_other(tmp_path):
    db = db_with(LABELS)
    good = readback([b"a"], [1], [(0, 0, -2, 2)])
    for spoil in ("reads", "n_reads", "label", "sample", "path"):
        rb = readback([b"a"], [1], [(0, 0, -2, 2)])
        path = tmp_path / "t.tsv"
        if spoil == "reads":
            rb.reads[0] += 1; rb.n_reads += 1                    # the sample's reads are not its unclassified reads plus its cells
        elif spoil == "n_reads":
            rb.n_reads += 1
        elif spoil == "label":
            rb.cells["label"][0] = len(LABELS)
        elif spoil == "sample":
            rb.cells["sample"][0] = 1
        else:
            path = tmp_path / "no" / "such" / "dir"
        with pytest.raises(lib.UtreeError):
            write_samples(db, [good, rb], str(path))
        assert not path.exists()


def test_header_declares_the_calls_and_the_abi_stays():
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in ("utree_samples_create", "utree_samples_add", "utree_samples_reset", "utree_samples_free", "utree_samples_read",
                 "utree_samples_write", "utree_search_file_samples", "utree_rank_search_file_samples"):
        assert name in lib.SYMBOLS and hasattr(L, name) and re.search(r"\b%s\(" % name, hdr), name
    assert re.search(r"#define\s+UTREE_ABI_VERSION\s+4\b", hdr) and L.utree_abi_version() == 4
    assert re.search(r"typedef struct \{ uint32_t sample, label; int32_t cut; uint32_t pad; uint64_t reads; \} utree_samples_cell;", hdr)
    assert C.sizeof(lib.SamplesCell) == 24 == SAMPLES_CELL_DTYPE.itemsize and C.sizeof(lib.SamplesTable) == 64
    assert "no ';'-prefix rows" in hdr.lower() or "NO ';'-prefix rows" in hdr
    assert L.utree_samples_create(None, 16, 16, ord("_"), C.byref(C.c_void_p())) == lib.E_ARG


def test_python_takes_the_path():
    import inspect
    from utree_amd.search import DeviceTree, search_gg, search_rank
    for f in (search_gg, search_rank):
        assert "samples" in inspect.signature(f).parameters and "sample_delim" in inspect.signature(f).parameters
    assert callable(DeviceTree.samples)
