"""The database inspection without a GPU: the surface of the ABI, the argument checks (which come before any file, and files before any
device), the host-only writer utree_inspect_write pinned byte for byte to tests/inspect_ref.py, and inspect_ref's own invariants."""
import ctypes as C
import os
import re

import pytest

import inspect_ref as R
import merge_ref as M
import util
from utree_amd import lib, search

DESC = ("some dir/db.ctr", ".ctr", 8, 4)
G = M.G
SP_A, SP_B = G + b";s__a", G + b";s__b"
ODD = b"k__\xc3\x84 \xff;p__two words;c__x"                         # bytes above 0x7F and spaces
LABELS = [G, SP_A, SP_B, b"k__A;p__B", b"k__A;p__Bx", b"k__Z", ODD]


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------------------
def test_names_are_declared_bound_and_exported():
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in ("utree_inspect_file", "utree_inspect_write"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in lib.SYMBOLS and hasattr(L, name)
    for t in ("utree_inspect_stats", "utree_inspect_entry", "utree_inspect_pair"):
        assert "} %s;" % t in hdr
    assert lib.INSPECT_CLI_PATH.endswith("utree-inspect") and callable(search.inspect)
    for text in ("w ^ (d << 2p)", "kmers = isolated + same + lineage + conflict", "pairs(t, t') = pairs(t', t)", "Only substitutions",
                 "a sample of its k-mers", "compared as stored", "UTREE_INSPECT_PAIRS"):
        assert text in hdr, "the header states the definition, the invariants and the limits"


def test_the_stats_layout_is_the_headers():
    """eight 64-bit figures, six 32-bit ones, two doubles: 104 bytes, fields in the header's order"""
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    body = hdr[:hdr.index("} utree_inspect_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {"):], flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        parts = decl.replace(",", " ").split()
        names += parts[1:]
    assert names == [f[0] for f in lib.InspectStats._fields_]
    assert C.sizeof(lib.InspectStats) == 8 * 8 + 6 * 4 + 2 * 8 == 104
    assert C.sizeof(lib.InspectEntry) == 48 and C.sizeof(lib.InspectPair) == 16


def test_nothing_else_moved():
    L = lib.load()
    assert L.utree_abi_version() == 4
    assert C.sizeof(lib.SearchRequest) == 128 and lib.SearchRequest._fields_[-1][0] == "redistribute_reads_path"
    assert C.sizeof(lib.MergeStats) == 72 and C.sizeof(lib.MergeInput) == 32 and C.sizeof(lib.CompareStats) == 120


def test_argument_checks_come_before_any_file(tmp_path):
    L = lib.load()
    rep, prs = str(tmp_path / "never.tsv").encode(), str(tmp_path / "never_pairs.tsv").encode()
    missing = str(tmp_path / "missing.ubt").encode()
    st = lib.InspectStats()
    assert L.utree_inspect_file(None, rep, prs, 0, C.byref(st)) == lib.E_ARG
    assert L.utree_inspect_file(missing, None, prs, 0, C.byref(st)) == lib.E_ARG
    assert L.utree_inspect_file(missing, rep, prs, 0, None) == lib.E_ARG
    assert L.utree_inspect_file(missing, rep, prs, 0, C.byref(st)) == lib.E_IO                   # only now is a file looked for
    assert b"missing.ubt" in L.utree_last_hip_error()
    short = str(tmp_path / "short.ubt")
    open(short, "wb").write(M.db_file(M.Db(8, 2, [(5, b"k__A;p__B")]))[:-2])
    assert L.utree_inspect_file(short.encode(), rep, None, 12345, C.byref(st)) == lib.E_FORMAT    # ... and the file before any device
    assert not os.path.exists(rep) and not os.path.exists(prs)
    with pytest.raises(lib.UtreeError) as e:
        search.inspect(missing.decode(), rep.decode())
    assert e.value.code == lib.E_IO and "cannot open" in e.value.detail


# ---- 2. the writer against the definition --------------------------------------------------------------------------------------------------
def write(tmp_path, fig, pairs, desc=DESC, with_pairs=True, repeat=False, totals=(0, 0)):
    """utree_inspect_write on inspect_ref's figures: (code, report bytes, pairs bytes or None, stats).  repeat: every entry is given
    twice, split in two, to be added up by text."""
    texts = list(fig)
    pos = {t: i for i, t in enumerate(texts)}
    ent = [(t, [fig[t][k] for k in R.CLASSES]) for t in texts]
    if repeat:
        ent = [(t, [v // 2 for v in f]) for t, f in ent] + [(t, [v - v // 2 for v in f]) for t, f in ent]
    keep = [C.create_string_buffer(t, len(t) + 1) for t, _ in ent]
    E = (lib.InspectEntry * max(len(ent), 1))()
    for i, (t, f) in enumerate(ent):
        E[i].text, E[i].len = C.cast(keep[i], C.c_char_p), len(t)
        E[i].isolated, E[i].same, E[i].lineage, E[i].conflict = f
    pr = list(pairs.items())
    P = (lib.InspectPair * max(len(pr), 1))()
    for i, ((f, t), n) in enumerate(pr):
        P[i].from_, P[i].to, P[i].pairs = pos[f], pos[t] + (len(texts) if repeat else 0), n
    ins = lib.CompareInput(path=desc[0].encode(), is_ctr=int(desc[1] == ".ctr"), W=desc[2], I=desc[3])
    rep, prs = str(tmp_path / "report.tsv"), str(tmp_path / "pairs.tsv")
    st = lib.InspectStats()
    code = lib.load().utree_inspect_write(C.byref(ins), E, len(ent), P, len(pr), totals[0], totals[1], rep.encode(),
                                          prs.encode() if with_pairs else None, C.byref(st))
    read = lambda p: open(p, "rb").read() if os.path.exists(p) else None
    return code, read(rep), read(prs), st


def agree(tmp_path, db, **kw):
    fig, pairs, st = R.inspect(db)
    R.check_invariants(fig, pairs, st)
    desc = (DESC[0], DESC[1], db.W, db.I)
    want_rep, want_prs = R.files(fig, pairs, st, desc)
    code, rep, prs, got = write(tmp_path, fig, pairs, desc=desc, **kw)
    assert code == lib.OK and rep == want_rep and prs == want_prs
    assert {k: getattr(got, k) for k in st} == st and got.n_passes == 0 and got.is_ctr == 1
    return fig, pairs, st, rep, prs


def star(W, w, label_of):
    """w and all its 3k neighbours; label_of(j): the label of the j-th neighbour"""
    return [(w, label_of(-1))] + [(v, label_of(j)) for j, v in enumerate(R.neighbours(W, w))]


def test_writer_matches_the_definition_on_a_hand_made_database(tmp_path):
    x, y, z, q = 0x1111 << 20, 0x2222 << 36, 0x3333 << 44, 0x77 << 50
    db = M.Db(8, 4, sorted([
        (x, SP_A), (x ^ 1, SP_A), (x ^ (2 << 10), G), (x ^ (3 << 62), SP_B),      # conflict: a same, an ancestor and a sibling
        (y, G), (y ^ (1 << 2), SP_A), (y ^ (2 << 2), SP_B),                       # lineage: descendants only (which are each other's conflict)
        (z, b"k__A;p__B"), (z ^ 3, b"k__A;p__Bx"),                                # a longer text that is no descendant: conflict
        (q, ODD), (q ^ (1 << 40), ODD),                                           # same
        (0x5 << 58, b"k__Z"),                                                     # isolated
    ]))
    fig, pairs, st, rep, prs = agree(tmp_path, db)
    assert (st["isolated"], st["same"], st["lineage"], st["conflict"]) == (1, 3, 2, 6) and st["clean"] == 0
    kinds = {(f, t): R.kind(f, t) for f, t in pairs}
    assert kinds[(SP_A, G)] == "ancestor" and kinds[(G, SP_A)] == "descendant" and kinds[(SP_A, SP_B)] == "conflict"
    assert kinds[(b"k__A;p__B", b"k__A;p__Bx")] == "conflict" and pairs[(G, SP_A)] == 2
    lines = rep.split(b"\n")
    assert lines[0] == b"# db\tsome dir/db.ctr\t.ctr\t8\t4\t12\t7"
    assert lines[1] == b"# kmers\t12\tisolated\t1\tsame\t3\tlineage\t2\tconflict\t6\tpair_events\t%d\tdistinct_pairs\t%d" % (st["pair_events"], len(pairs))
    assert lines[2] == b"# taxon\tkmers\tisolated\tsame\tlineage\tconflict\tclade_kmers\tclade_conflict"
    rows = {l.split(b"\t")[0]: [int(v) for v in l.split(b"\t")[1:]] for l in lines[3:-1]}
    assert [l.split(b"\t")[0] for l in lines[3:-1]] == sorted(rows), "rows in bytewise order"
    assert rows[b"k__A;p__B"] == [1, 0, 0, 0, 1, 8, 5], "a label that is a prefix of others; k__A;p__Bx is not in its clade"
    assert rows[b"k__A"] == [0, 0, 0, 0, 0, 9, 6], "a pure prefix: zero own figures"
    assert rows[G] == [2, 0, 0, 2, 0, 7, 4] and rows[ODD] == [2, 0, 2, 0, 0, 2, 0]
    assert prs.split(b"\n")[0] == b"# from\tto\tpairs\tkind"
    # entries of equal text (two label lines) are added up, and so are their pairs
    code, rep2, prs2, _ = write(tmp_path, fig, pairs, repeat=True)
    assert code == lib.OK and (rep2, prs2) == (rep, prs)
    # without a pairs file the two totals are the arguments', and the pairs are not looked at
    os.unlink(str(tmp_path / "pairs.tsv"))
    code, rep3, prs3, got = write(tmp_path, fig, {}, with_pairs=False, totals=(st["pair_events"], st["distinct_pairs"]))
    assert code == lib.OK and rep3 == rep and prs3 is None and got.distinct_pairs == st["distinct_pairs"]


def test_writer_empty_database_empty_label_and_a_full_star(tmp_path):
    fig, pairs, st, rep, prs = agree(tmp_path, M.Db(8, 2, []))
    assert rep.count(b"\n") == 3 and prs == b"# from\tto\tpairs\tkind\n" and st["clean"] == 1
    # the empty text is a label like any other: by the literal rule it is an ancestor of ";x" and of nothing else
    db = M.Db(8, 2, sorted([(8, b""), (9, b";x"), (10, b"k__A"), (1 << 40, b""), (1 << 50, b"")]))
    fig, pairs, st, rep, prs = agree(tmp_path, db)
    assert R.kind(b";x", b"") == "ancestor" and R.kind(b"", b"k__A") == "conflict"
    assert b"\n\t3\t2\t0\t0\t1\t4\t2\n" in rep, "the empty taxon's row: its clade holds ;x"
    assert b"\n\t;x\t1\tdescendant\n" in prs and b"\n;x\t\t1\tancestor\n" in prs
    for W in (4, 8, 16):
        w = M.random_words(M.rng(W, 99), W, 1)[0]
        fig, pairs, st, _, _ = agree(tmp_path, M.Db(W, 2, sorted(star(W, w, lambda j: LABELS[(j + 1) % 3]))))
        assert st["kmers"] == 3 * R.bases(W) + 1 == {4: 49, 8: 97, 16: 193}[W] and st["isolated"] == 0


def test_writer_refuses_what_does_not_add_up(tmp_path):
    db = M.Db(8, 2, [(16, SP_A), (17, G), (18, SP_B)])
    fig, pairs, st = R.inspect(db)
    for broken in ({(SP_A, G): 1}, {**pairs, (SP_A, G): 2}, {**pairs, (SP_A, SP_A): 1}):
        code, rep, prs, _ = write(tmp_path, fig, broken)
        assert code == lib.E_ARG and rep is None and prs is None
    L = lib.load()
    ins = lib.CompareInput(path=b"x", W=8, I=2)
    assert L.utree_inspect_write(None, None, 0, None, 0, 0, 0, b"r", None, None) == lib.E_ARG
    assert L.utree_inspect_write(C.byref(ins), None, 0, None, 0, 0, 0, None, None, None) == lib.E_ARG
    assert L.utree_inspect_write(C.byref(ins), None, 1, None, 0, 0, 0, str(tmp_path / "r").encode(), None, None) == lib.E_ARG
    assert L.utree_inspect_write(C.byref(ins), None, 0, None, 1, 0, 0, str(tmp_path / "r").encode(), str(tmp_path / "p").encode(), None) == lib.E_ARG
    assert not os.path.exists(str(tmp_path / "r")) and not os.path.exists(str(tmp_path / "p"))
    code, rep, prs, _ = write(tmp_path / "no_such_dir", fig, pairs)
    assert code == lib.E_IO and rep is None and prs is None


# ---- 3. the definition's own invariants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,n", [(4, 200), (8, 513), (16, 150)])
def test_invariants_on_random_planted_inputs(W, n, tmp_path):
    db = R.planted(W, 2, n, 1, LABELS)
    fig, pairs, st, _, _ = agree(tmp_path, db)
    assert st["kmers"] == n and st["isolated"] < n and st["pair_events"] > 0
    assert all(len(set(R.neighbours(W, w))) == 3 * R.bases(W) for w, _ in db.nodes[:5])
