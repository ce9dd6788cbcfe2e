"""The per-sample redistribution without a GPU: tests/sample_redist_ref.py against figures fixed beforehand (so that the GPU tests compare
against something pinned, and something that differs from the pooled redistribution), utree_sredist_write (csrc/sredist.c) on hand-made
figures against that contract, and the ABI surface."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import redist_ref
import sample_redist_ref as srr
import util
from samples_ref import sample_id
from test_coverage_cpu import LABELS, db_with
from test_redist_cpu import reference_sets
from utree_amd import lib
from utree_amd.search import SREDIST_CELL_DTYPE, SREDIST_ENTRY_DTYPE, write_sample_redistribution

# fixture, RC, reads, deal -> passes of the three samples (in the order of sample_redist_ref.THREE)
PINNED = {
    ("toy", 0, 4000, "block"): (5, 4, 4),
    ("toy", 0, 4000, "rr"): (5, 4, 5),
    ("toy", 1, 4000, "block"): (5, 5, 4),
    ("toy", 1, 4000, "rr"): (5, 4, 6),
    ("vote", 0, 4000, "block"): (4, 5, 5),
    ("vote", 0, 4000, "rr"): (4, 7, 4),
    ("ix32", 1, 3000, "block"): (4, 5, 4),
    ("ix32", 1, 3000, "rr"): (4, 3, 4),
}
_DEALT = {}


def dealt(name, rc, n, deal):
    """(candidate sets, label texts, names, sample ids) of a fixture's first n reads dealt to three samples (cached: the GPU tests use them)"""
    key = (name, rc, n, deal)
    if key not in _DEALT:
        sets, texts = reference_sets(name, rc, n)
        names = srr.deal_names(len(sets), deal)                      # (a fixture may hold fewer reads than n)
        _DEALT[key] = (sets, texts, names, [sample_id(nm) for nm in names])
    return _DEALT[key]


@pytest.mark.parametrize("name,rc,n,deal", sorted(PINNED))
def test_yardstick_is_pinned(name, rc, n, deal):
    sets, texts, names, ids = dealt(name, rc, n, deal)
    solved = srr.solve(sets, ids)
    assert tuple(solved[s][2] for s in srr.THREE) == PINNED[(name, rc, n, deal)]
    assert sum(v[4] for v in solved.values()) == n and sorted(v[4] for v in solved.values())[0] >= n // 3
    tab = srr.table_bytes(solved, texts)
    N, G, A, S, pids, nj, uj, aj, P, rows = srr.check_invariants(tab)
    assert (N, S) == (n, 3) and pids == sorted(srr.THREE) and G == sum(1 for s in sets if s)
    # the table differs from the one that assigns each read under the pooled final tally: else the GPU tests would show nothing
    pooled, _ = srr.pooled_assignment(sets, ids)
    differ = sum(1 for s in solved for l in set(solved[s][0]) | set(pooled[s]) if solved[s][0].get(l, 0) != pooled[s].get(l, 0))
    assert differ > 0
    pooled_tab = srr.table_bytes({s: (pooled[s], solved[s][1], solved[s][2], solved[s][3], solved[s][4]) for s in solved}, texts)
    assert pooled_tab != tab


@pytest.mark.parametrize("name,rc,n", [("toy", 1, 4000), ("vote", 0, 4000)])
def test_one_sample_is_the_redistribution(name, rc, n):
    """a file that holds one sample: the column is the `assigned` column of the redistribution's file, `# passes` its passes"""
    sets, texts = reference_sets(name, rc, n)
    tab = srr.file_from_sets(sets, texts, [b"only_%d" % i for i in range(n)])
    N, G, A, S, ids, nj, uj, aj, P, rows = srr.check_invariants(tab)
    a, u, p, amb, _ = redist_ref.solve(sets, n)
    red = redist_ref.redist_file(a, u, texts, n, amb, p).split(b"\n")
    head = red[0].split(b"\t")
    assert (N, G, A, S, ids, P) == (n, int(head[3]), int(head[7]), 1, [b"only"], [int(head[9])])
    want = {}
    for ln in red[2:-1]:
        f = ln.rsplit(b"\t", 4)
        if int(f[1]):
            want[f[0]] = [int(f[1])]
    assert rows == want


PAD = 1_200_000      # unclassified reads added to a sample: N_s / 100000 = 12 and more, while the changes stay what they were


def test_solve_multiset_is_solve_and_the_threshold_matters():
    """solve_multiset is redist_ref.solve.  With every count times 1000 the threshold is above 0 (N_s >= 100 000) but the changes grow with it;
    with PAD unclassified reads added instead, N_s alone grows and some sample stops earlier."""
    sets, texts, names, ids = dealt("vote", 0, 4000, "rr")
    earlier = 0
    for i, ss in srr.by_sample(sets, ids).items():
        ms = redist_ref.multiset(ss)
        a, u, p, amb, _ = redist_ref.solve(ss, len(ss))
        assert srr.solve_multiset(ms, len(ss)) == (a, u, p, amb)
        a2, u2, p2, amb2 = srr.solve_multiset({s: 1000 * c for s, c in ms.items()}, 1000 * len(ss))
        assert 1000 * len(ss) // 100000 >= 10 and p2 <= p and amb2 == 1000 * amb
        a3, u3, p3, amb3 = srr.solve_multiset(ms, len(ss) + PAD)
        assert p3 <= p and amb3 == amb
        earlier += p3 < p
    assert earlier > 0


# ---- utree_sredist_write ----------------------------------------------------------------------------------------------------------------
def write(tmp_path, labels, samples, n_reads=None, I=2, name="t.tsv", split=()):
    """samples: [(id, reads, unclassified, passes, ambiguous, {label index: (assigned, unique)})] in the order a device numbered them;
    split: (sample, label) pairs whose figures are given as two entries (a .ctr's label lines of equal text are one label, so entries of equal
    text are entries of one label: they are added up when the file is written).  Returns (bytes written, the contract's bytes)"""
    db = db_with(labels, I)
    rows = []
    for s, smp in enumerate(samples):
        for l, (a, u) in sorted(smp[5].items()):
            rows += [(s, l, a - a // 2, u), (s, l, a // 2, 0)] if (s, l) in split else [(s, l, a, u)]
    e = np.array(rows, dtype=SREDIST_ENTRY_DTYPE)
    path = tmp_path / name
    write_sample_redistribution(db, [s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples], [s[3] for s in samples],
                                [s[4] for s in samples], e, sum(s[1] for s in samples) if n_reads is None else n_reads, str(path))
    solved = {s[0]: ({l: a for l, (a, u) in s[5].items()}, {l: u for l, (a, u) in s[5].items()}, s[3], s[4], s[1]) for s in samples}
    return path.read_bytes(), srr.table_bytes(solved, labels)


def test_write_merges_entries_of_equal_text_and_orders_ids(tmp_path):
    labels, twin = LABELS, 7
    samples = [(b"s2", 20, 3, 4, 6, {0: (10, 2), twin: (5, 5), 3: (2, 0)}),
               (b"", 7, 0, 1, 0, {5: (7, 7)}),                       # the empty id
               (b"a\tb", 5, 5, 1, 0, {}),                            # a sample with only unclassified reads; an id that is escaped
               (b"c\\d\r", 9, 1, 7, 8, {twin: (8, 0), 2: (0, 0)}),
               (b"s1", 4, 0, 2, 1, {0: (1, 0), 1: (3, 3)})]
    got, want = write(tmp_path, labels, samples, split=[(0, 0), (3, twin), (4, 1)])
    assert got == want
    N, G, A, S, ids, n, u, a, P, rows = srr.check_invariants(got)
    assert ids == [b"", b"a\\tb", b"c\\\\d\\r", b"s1", b"s2"] and P == [1, 1, 7, 2, 4] and a == [0, 0, 8, 1, 6] and u == [0, 5, 1, 0, 3]
    assert rows[LABELS[0]] == [0, 0, 0, 1, 10] and rows[LABELS[twin]] == [0, 0, 8, 0, 5] and LABELS[2] not in rows            # assigned 0 everywhere: no row
    assert not any(t == b";k__Z" for t in rows)                                     # no ';'-prefix rows
    assert got.split(b"\n")[0] == b"# reads\t45\tclassified\t36\tunclassified\t9\tambiguous\t15\tsamples\t5"


def test_write_no_samples(tmp_path):
    got, want = write(tmp_path, LABELS, [])
    assert got == want == b"# reads\t0\tclassified\t0\tunclassified\t0\tambiguous\t0\tsamples\t0\n# taxon\n# reads\n# unclassified\n# ambiguous\n# passes\n"


def test_write_u32_labels_and_counts_beyond_32_bits(tmp_path):
    labels = [b"k__L%d;p__M%d;c__N%d" % (i % 7, i % 3, i) for i in range(300)]
    big = (1 << 32) + 5
    rng = np.random.default_rng(9)
    samples = []
    for s in range(4):
        fig = {}
        for l in rng.choice(300, 40, replace=False).tolist():
            uq = int(rng.integers(0, 1000))
            fig[l] = (uq + int(rng.integers(0, 50)) * big, uq)
        g = sum(a for a, _ in fig.values())
        samples.append((b"big%d" % s, g + 3 * big, 3 * big, 100, g - sum(q for _, q in fig.values()), fig))
    got, want = write(tmp_path, labels, samples, I=4)
    assert got == want
    assert int(got.split(b"\t")[1]) > 1 << 40
    srr.check_invariants(got)


def test_write_refuses_figures_that_contradict_each_other(tmp_path):
    good = [(b"a", 6, 1, 2, 2, {0: (3, 1), 1: (2, 2)}), (b"b", 2, 2, 1, 0, {})]
    got, want = write(tmp_path, LABELS, good)
    assert got == want
    spoiled = {
        "column": [(b"a", 7, 1, 2, 2, {0: (3, 1), 1: (2, 2)}), good[1]],             # assigned does not sum to reads - unclassified
        "unclassified": [(b"a", 6, 7, 2, 2, {0: (3, 1), 1: (2, 2)}), good[1]],
        "ambiguous": [(b"a", 6, 1, 2, 6, {0: (3, 1), 1: (2, 2)}), good[1]],          # more ambiguous than classified reads
        "label": [(b"a", 6, 1, 2, 2, {0: (3, 1), len(LABELS): (2, 2)}), good[1]],
        "passes": [(b"a", 6, 1, 0, 2, {0: (3, 1), 1: (2, 2)}), good[1]],
        "twice": [good[0], (b"a", 2, 2, 1, 0, {})],                                  # two samples with one id
    }
    for why, samples in spoiled.items():
        with pytest.raises(lib.UtreeError) as e:
            write(tmp_path, LABELS, samples, name=why)
        assert e.value.code == lib.E_ARG and not (tmp_path / why).exists(), why
    with pytest.raises(lib.UtreeError) as e:
        write(tmp_path, LABELS, good, n_reads=9, name="n")                           # the samples' reads are not the reads
    assert e.value.code == lib.E_ARG
    db = db_with(LABELS)
    with pytest.raises(lib.UtreeError) as e:                                         # an entry that names no sample
        write_sample_redistribution(db, [b"a"], [1], [0], [1], [0], np.array([(1, 0, 1, 1)], dtype=SREDIST_ENTRY_DTYPE), 1, str(tmp_path / "s"))
    assert e.value.code == lib.E_ARG
    for path in (str(tmp_path / "no" / "such" / "dir"), "/dev/full"):                # a path that cannot be created, a file that takes no bytes
        with pytest.raises(lib.UtreeError) as e:
            write_sample_redistribution(db, [b"a"], [1], [0], [1], [0], np.array([(0, 0, 1, 1)], dtype=SREDIST_ENTRY_DTYPE), 1, path)
        assert e.value.code == lib.E_IO


# ---- the ABI surface --------------------------------------------------------------------------------------------------------------------
NAMES = ("utree_sredist_create", "utree_sredist_reset", "utree_sredist_free", "utree_sredist_classify_batch", "utree_sredist_read",
         "utree_sredist_insert", "utree_sredist_merge", "utree_sredist_solve", "utree_sredist_write", "utree_search_file_sample_redistribute")


def test_abi_surface():
    header = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SYMBOLS and getattr(L, name) is not None, name
    assert "#define UTREE_ABI_VERSION 4\n" in header and L.utree_abi_version() == 4
    assert L.utree_strerror(15) == b"unknown error"                     # no new error code: the report's failure is UTREE_E_PROFILE
    assert re.search(r"typedef struct \{ uint32_t sample, n; uint64_t first, reads; \} utree_sredist_cell;", header)
    assert re.search(r"typedef struct \{ uint32_t sample, label; uint64_t assigned, unique; \} utree_sredist_entry;", header)
    assert C.sizeof(lib.SredistCell) == 24 == SREDIST_CELL_DTYPE.itemsize and C.sizeof(lib.SredistEntry) == 24 == SREDIST_ENTRY_DTYPE.itemsize
    assert L.utree_sredist_create(None, 16, 16, 16, ord("_"), C.byref(C.c_void_p())) == lib.E_ARG


def test_python_takes_the_path():
    from utree_amd.search import DeviceTree, search_gg, search_rank
    assert "sample_redistribute" in inspect.signature(search_gg).parameters
    assert "sample_redistribute" not in inspect.signature(search_rank).parameters      # GG search only
    assert callable(DeviceTree.sample_redistribution)
