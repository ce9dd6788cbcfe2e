"""utree_inspect_file on the GPU (inspect_kernels.hip: the directory, the neighbour pass, the pair table; merge_kernels.hip: the passes that
fill the resident arrays): every report, every pairs file and every figure of the stats is compared with tests/inspect_ref.py, the
definition in plain Python.  All figures are integers: nothing is tolerated.  Random words have no neighbours, so every test plants them."""
import os
import subprocess

import numpy as np
import pytest

import inspect_ref as R
import merge_ref as M
import util
from utree_amd import ctrfile, lib, search

pytestmark = pytest.mark.gpu
ONES = {4: (1 << 32) - 1, 8: (1 << 64) - 1, 16: (1 << 128) - 1}
Db = M.Db
G = M.G
SP_A, SP_B = G + b";s__a", G + b";s__b"
LABELS = [G, SP_A, SP_B, b"k__A;p__B", b"k__A;p__Bx", b"k__Z", b"k__\xc3\x84 \xff;p__two words;c__x"]


def as_ctr(db, path):
    labs = M.parse_labels(M.db_file(db)[32 + len(db.nodes) * (db.W + db.I):])
    ix = np.array([labs.index(l) for _, l in db.nodes], dtype=np.uint32)
    hi = np.array([w >> 64 for w, _ in db.nodes], dtype=np.uint64)
    lo = np.array([w & 0xFFFFFFFFFFFFFFFF for w, _ in db.nodes], dtype=np.uint64)
    ctrfile.write_ctr(path, db.W, db.I, hi, lo, ix, [l.decode("latin-1") for l in labs])


def write_db(tmp_path, db, name, ctr=False):
    p = str(tmp_path / name)
    if ctr:
        as_ctr(db, p)
    else:
        open(p, "wb").write(M.db_file(db))
    return p


def check(tmp_path, monkeypatch, db, pass_nodes=None, path=None, ctr=False, tag="i", pairs=True, cap=None):
    """inspect db on the device; both files and every figure must be inspect_ref's.  Returns (stats, report, pairs file or None)."""
    for name, v in (("UTREE_TEST_MERGE_PASS_NODES", pass_nodes), ("UTREE_INSPECT_PAIRS", cap)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)
    p = path or write_db(tmp_path, db, tag + ".db", ctr)
    rep, prs = str(tmp_path / (tag + "_report.tsv")), str(tmp_path / (tag + "_pairs.tsv"))
    st = search.inspect(p, rep, prs if pairs else None)
    fig, want_pairs, ws = R.inspect(db)
    R.check_invariants(fig, want_pairs, ws)
    want_rep, want_prs = R.files(fig, want_pairs, ws, (p, ".ctr" if ctr else ".ubt", db.W, db.I))
    got_rep = open(rep, "rb").read()
    assert got_rep == want_rep
    got_prs = None
    if pairs:
        got_prs = open(prs, "rb").read()
        assert got_prs == want_prs
    else:
        assert not os.path.exists(prs)
    assert {k: getattr(st, k) for k in ws} == ws
    assert st.is_ctr == int(ctr) and st.n_passes >= (1 if db.nodes else 0) and st.seconds > 0
    return st, got_rep, got_prs


def fails(tmp_path, p, code, says=None, pairs=True):
    rep, prs = str(tmp_path / "refused.tsv"), str(tmp_path / "refused_pairs.tsv")
    with pytest.raises(lib.UtreeError) as e:
        search.inspect(p, rep, prs if pairs else None)
    assert e.value.code == code, e.value
    assert says is None or says in e.value.detail, e.value.detail
    assert not os.path.exists(rep) and not os.path.exists(prs), "a failed call leaves neither output file behind"
    return e.value


def labelled(words, key, labels=LABELS):
    r = M.rng(key)
    return [(w, labels[int(r.integers(0, len(labels)))]) for w in words]


def star(W, w, label_of):
    """w and all its 3k neighbours; label_of(j): the label of the j-th neighbour (-1: of w)"""
    return [(w, label_of(-1))] + [(v, label_of(j)) for j, v in enumerate(R.neighbours(W, w))]


def merged(*parts):
    d = {}
    for part in parts:
        for w, l in part:
            d.setdefault(w, l)
    return sorted(d.items())


# ---- input sizes: the wavefront and block edges of the decode, the append and the neighbour pass -----------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_sizes(n, tmp_path, monkeypatch):
    db = R.planted(8, 2, n, 1, LABELS)
    st, _, _ = check(tmp_path, monkeypatch, db)
    assert st.kmers == n and st.n_passes == 1
    assert (st.isolated < n and st.pair_events > 0) or n == 1


# ---- word widths: where a substitution stands --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 8, 16])
def test_lowest_and_highest_base_and_the_extreme_words(W, tmp_path, monkeypatch):
    k = R.bases(W)
    mid = [w for w in M.random_words(M.rng(2, W), W, 200) if 0 < w < ONES[W]]
    a, b, c = mid[10], mid[90], mid[150]
    plant = [(a, SP_A), (R.mutate(W, a, 0, 1), G),                  # the lowest base: next to the node
             (b, SP_A), (R.mutate(W, b, k - 1, 2), SP_B),           # the highest base: the other end of the database
             (c, G), (R.mutate(W, c, k // 2 - 1, 3), G), (R.mutate(W, c, k // 2, 1), SP_A),      # W = 16: positions 31 and 32, the halves' boundary
             (0, SP_A), (1, SP_B), (3 << (2 * k - 2), SP_A),        # word 0: a neighbour next to it and one in the last cell
             (ONES[W], G), (ONES[W] ^ 2, SP_A), (ONES[W] ^ (1 << (2 * k - 1)), b"k__Z")]
    db = Db(W, 2, merged(plant, labelled(mid, 21)))
    st, _, prs = check(tmp_path, monkeypatch, db)
    assert st.conflict >= 5 and st.lineage >= 3 and st.same >= 1 and st.isolated > 150
    assert SP_A + b"\t" + SP_B + b"\t" in prs and G + b"\t" + b"k__Z\t1\tconflict\n" in prs
    check(tmp_path, monkeypatch, db, pass_nodes=64, tag="p")
    check(tmp_path, monkeypatch, Db(W, 4, db.nodes), ctr=W != 4, tag="ix4")


@pytest.mark.parametrize("W", [4, 8, 16])
def test_full_star(W, tmp_path, monkeypatch):
    """one word and all its 3k neighbours: 48 for W = 4 (a word differing only above bit 32 cannot exist), 96, 192.  The centre sees them
    all; two neighbours see each other exactly when they differ from the centre at the same base."""
    w = M.random_words(M.rng(3, W), W, 1)[0]
    k = R.bases(W)
    db = Db(W, 2, sorted(star(W, w, lambda j: SP_A)))
    st, _, prs = check(tmp_path, monkeypatch, db)
    assert st.kmers == 3 * k + 1 == {4: 49, 8: 97, 16: 193}[W] and st.same == st.kmers and st.pair_events == 0
    mixed = Db(W, 2, sorted(star(W, w, lambda j: G if j < 0 else LABELS[j % len(LABELS)])))
    st, _, prs = check(tmp_path, monkeypatch, mixed, tag="mixed")
    centre_events = sum(LABELS[j % len(LABELS)] != G for j in range(3 * k))
    assert st.isolated == 0 and int(prs.split(G + b"\t" + SP_A + b"\t")[1].split(b"\t")[0]) > 0
    assert st.pair_events >= 2 * centre_events and st.conflict > 0
    # one off-lineage neighbour among many of the node's own text
    one = Db(W, 2, sorted(star(W, w, lambda j: b"k__Z" if j == 3 * k - 1 else SP_A)))
    st, _, _ = check(tmp_path, monkeypatch, one, tag="one")
    assert (st.conflict, st.same, st.pair_events, st.distinct_pairs) == (4, 3 * k - 3, 6, 2)   # the centre, k__Z and its two base-mates


def test_complete_block(tmp_path, monkeypatch):
    """256 words that share all but their last four bases, among unrelated ones: each has 12 neighbours in the block"""
    W = 8
    base = M.random_words(M.rng(4), W, 1)[0] & ~0xFF
    block = [(base | v, LABELS[(v * 7 // 16) % 3]) for v in range(256)]
    db = Db(W, 2, merged(block, labelled(M.random_words(M.rng(5), W, 300), 41)))
    st, _, _ = check(tmp_path, monkeypatch, db)
    assert st.kmers == 556 and st.isolated == 300 and st.pair_events > 0
    st, _, _ = check(tmp_path, monkeypatch, Db(W, 2, [(w, SP_A) for w, _ in block]), tag="alone")
    assert (st.same, st.kmers, st.pair_events) == (256, 256, 0)


# ---- the directory -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 8, 16])
def test_directory_edges(W, tmp_path, monkeypatch):
    """neighbours inside the first and the last cell of the top 24 bits, and across a cell edge (the lowest base of the top 24 bits)"""
    shift = {4: 8, 8: 40, 16: 104}[W]
    low = (1 << shift) - 1
    r = M.rng(6, W)
    rnd = lambda: int.from_bytes(r.bytes(W), "little") & low
    first, last, edge = rnd(), (0xFFFFFF << shift) | rnd(), (0x123454 << shift) | rnd()
    plant = [(first, SP_A), (first ^ 1, SP_B), (first ^ (1 << (shift - 1)), G),
             (last, SP_A), (last ^ 2, SP_A), (last ^ (1 << (shift - 2)), b"k__Z"),
             (edge, G), (edge ^ (1 << shift), SP_A), (edge ^ (3 << shift), SP_B), (edge ^ 1, G),        # cells 0x123455 and 0x123457
             (first ^ (2 << shift), G), (last ^ (3 << (shift + 22)), SP_A)]                             # out of the first cell, into the last
    db = Db(W, 2, merged(plant, labelled(M.random_words(M.rng(7, W), W, 120), 61)))
    st, _, _ = check(tmp_path, monkeypatch, db)
    assert st.isolated >= 100 and st.conflict >= 6
    check(tmp_path, monkeypatch, db, pass_nodes=16, tag="p")


@pytest.mark.parametrize("at", [255, 256])
def test_only_neighbour_in_another_block(at, tmp_path, monkeypatch):
    """the node at sorted position 255 / 256 (the last and the first lane of a block) has its one neighbour two blocks on"""
    W = 8
    words = M.random_words(M.rng(8), W, 600)
    w = words[at]
    v = R.mutate(W, w, 31, (w >> 62) ^ 3)                          # its top base becomes T: the far end
    nodes = merged([(w, SP_A), (v, SP_B)], [(x, G) for x in words])
    where = [x for x, _ in nodes]
    assert where.index(w) == at and where.index(v) >= 512
    st, _, prs = check(tmp_path, monkeypatch, Db(W, 2, nodes))
    assert (st.conflict, st.isolated, st.pair_events) == (2, 599, 2)
    assert prs == b"# from\tto\tpairs\tkind\n" + SP_A + b"\t" + SP_B + b"\t1\tconflict\n" + SP_B + b"\t" + SP_A + b"\t1\tconflict\n"


# ---- every class and every kind ----------------------------------------------------------------------------------------------------------------
def test_every_class_and_every_kind(tmp_path, monkeypatch):
    W = 8
    x, y, z, q, e = 0x1111 << 20, 0x2222 << 36, 0x3333 << 44, 0x77 << 50, 0x99 << 54
    db = Db(W, 2, sorted([
        (x, SP_A), (x ^ 1, SP_A), (x ^ (2 << 10), SP_A),                          # only same-text neighbours
        (y, SP_B), (y ^ (1 << 2), G),                                             # only an ancestor / only a descendant
        (z, b"k__A;p__B"), (z ^ 3, b"k__A;p__Bx"),                                # a longer text that is no descendant: conflict
        (q, b";p__E"), (q ^ (1 << 40), b";p__E;c__F"),                            # texts whose first cut is the empty taxon
        (e, b"k__Z"),                                                             # isolated
    ]))
    st, rep, prs = check(tmp_path, monkeypatch, db)
    assert (st.isolated, st.same, st.lineage, st.conflict, st.clean) == (1, 3, 4, 2, 0)
    assert SP_B + b"\t" + G + b"\t1\tancestor\n" in prs and G + b"\t" + SP_B + b"\t1\tdescendant\n" in prs
    assert b"k__A;p__B\tk__A;p__Bx\t1\tconflict\n" in prs and b";p__E;c__F\t;p__E\t1\tancestor\n" in prs
    assert b"\n\t0\t0\t0\t0\t0\t2\t0\n" in rep, "the empty taxon's row: a pure prefix"
    clean = Db(W, 2, [n for n in db.nodes if n[1] != b"k__A;p__Bx"])
    st, _, _ = check(tmp_path, monkeypatch, clean, tag="clean")
    assert st.clean == 1 and st.conflict == 0 and st.lineage == 4
    # a label line with an empty text: the merge's reader refuses the file, and so does this one
    raw = np.array([W, 0, 2, 1], dtype="<u8").tobytes() + M.word_bytes(W, 5) + (0).to_bytes(2, "little") + b"\t1\n"
    p = str(tmp_path / "empty_label.ubt")
    open(p, "wb").write(raw)
    fails(tmp_path, p, lib.E_FORMAT)
    with pytest.raises(lib.UtreeError) as err:
        search.merge_probe(p)
    assert err.value.code == lib.E_FORMAT


# ---- input forms -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [8, 16])
def test_ctr_and_ubt_give_the_same_report(W, tmp_path, monkeypatch):
    db = R.planted(W, 2, 300, 9, LABELS)
    _, rep_u, prs_u = check(tmp_path, monkeypatch, db, tag="u")
    _, rep_c, prs_c = check(tmp_path, monkeypatch, db, ctr=True, tag="c")
    assert rep_u.split(b"\n", 1)[1] == rep_c.split(b"\n", 1)[1] and prs_u == prs_c
    _, rep_4, prs_4 = check(tmp_path, monkeypatch, Db(W, 4, db.nodes), ctr=True, pass_nodes=50, tag="c4")
    assert rep_4.split(b"\n", 1)[1] == rep_u.split(b"\n", 1)[1] and prs_4 == prs_u


def test_label_lines_no_node_carries_and_repeated_lines(tmp_path, monkeypatch):
    W, I = 8, 2
    w = 0xABCDEF << 20
    # line 0 = SP_B, line 1 = SP_A, line 2 = SP_B again (as the loader reads it: the text of index 0), line 3 a text no node carries
    recs = b"".join(M.word_bytes(W, x) + ix.to_bytes(I, "little") for x, ix in ((w, 1), (w ^ 1, 0), (w ^ 2, 1), (w ^ (1 << 50), 0)))
    raw = np.array([W, 0, I, 4], dtype="<u8").tobytes() + recs + SP_B + b"\t2\n" + SP_A + b"\t2\n" + SP_B + b"\t0\n" + b"k__Never;p__Seen\t0\n"
    p = str(tmp_path / "lines.ubt")
    open(p, "wb").write(raw)
    db = Db(W, I, [(w, SP_A), (w ^ 1, SP_B), (w ^ 2, SP_A), (w ^ (1 << 50), SP_B)])
    st, rep, _ = check(tmp_path, monkeypatch, db, path=p)
    assert (st.labels, st.conflict, st.distinct_pairs, st.pair_events) == (2, 4, 2, 6) and b"k__Never" not in rep


def test_passes(tmp_path, monkeypatch):
    """513 nodes in passes of 64: the one-pass result, with neighbours across the passes' boundaries (every tenth node has a neighbour at
    its highest base, a quarter of the database away)"""
    W = 8
    db0 = R.planted(W, 2, 460, 10, LABELS)
    far = [(R.mutate(W, w, 31, 1 + j % 3), LABELS[j % 5]) for j, (w, _) in enumerate(db0.nodes[::10])]
    db = Db(W, 2, merged(db0.nodes, far)[:513])
    assert len(db.nodes) >= 500
    one, rep1, prs1 = check(tmp_path, monkeypatch, db, tag="one")
    p = str(tmp_path / "one.db")
    many, rep2, prs2 = check(tmp_path, monkeypatch, db, pass_nodes=64, path=p, tag="many")
    assert one.n_passes == 1 and many.n_passes >= 8 and rep2 == open(str(tmp_path / "one_report.tsv"), "rb").read() and prs2 == prs1


def test_words_of_one_prefix_stay_in_one_pass(tmp_path, monkeypatch):
    W = 8
    words = [(0xABCDEF << 40) | v for v in range(0, 600, 2)]
    st, _, _ = check(tmp_path, monkeypatch, Db(W, 2, labelled(words, 51)), pass_nodes=64)
    assert st.n_passes == 1 and st.isolated == 0


# ---- the pair table ----------------------------------------------------------------------------------------------------------------------------
def pair_db(n_labels):
    """a chain of n_labels words, each the neighbour of the next, under n_labels different sibling labels: 2 (n_labels - 1) distinct pairs"""
    w = 0x5A5A5A << 30
    return Db(8, 2, sorted((w ^ (j << 60), b"k__A;p__P;c__%d" % j) if j < 4 else ((w ^ (3 << 60)) ^ ((j - 3) << 20), b"k__A;p__P;c__%d" % j)
                           for j in range(n_labels)))


def test_pair_capacity(tmp_path, monkeypatch):
    db = pair_db(4)                                                # four words at one base: every pair of them, 12 distinct ordered pairs
    fig, pairs, ws = R.inspect(db)
    assert ws["distinct_pairs"] == 12
    p = write_db(tmp_path, db, "pairs.ubt")
    monkeypatch.setenv("UTREE_INSPECT_PAIRS", "4")
    e = fails(tmp_path, p, lib.E_NOMEM, says="UTREE_INSPECT_PAIRS=4")
    monkeypatch.setenv("UTREE_INSPECT_PAIRS", "11")
    fails(tmp_path, p, lib.E_NOMEM, says="UTREE_INSPECT_PAIRS=11")
    st, rep12, _ = check(tmp_path, monkeypatch, db, path=p, cap=12, tag="exact")           # exactly the capacity
    st, rep, _ = check(tmp_path, monkeypatch, db, path=p, tag="default")
    assert st.distinct_pairs == 12 and rep12.split(b"\n", 1)[1] == rep.split(b"\n", 1)[1]
    st, rep4, _ = check(tmp_path, monkeypatch, db, path=p, cap=4, pairs=False, tag="nopairs")   # no pairs file: the capacity does not bind
    assert rep4.split(b"\n", 1)[1] == rep.split(b"\n", 1)[1] and st.distinct_pairs == 12
    monkeypatch.setenv("UTREE_INSPECT_PAIRS", "many")
    fails(tmp_path, p, lib.E_ARG, says="UTREE_INSPECT_PAIRS")


def test_many_pairs(tmp_path, monkeypatch):
    """some thousands of distinct pairs, most of them met once, a few thousands of times from every block"""
    W = 8
    r = M.rng(11)
    labs = [b"k__A;p__P%d;c__c%d" % (i % 7, i) for i in range(300)]
    nodes = {}
    for w in M.random_words(r, W, 1500):
        nodes[w] = labs[int(r.integers(0, 300))]
        nodes.setdefault(R.mutate(W, w, int(r.integers(0, 32)), int(r.integers(1, 4))), labs[int(r.integers(0, 300))])
    hot = 0x0F0F << 40
    for v in range(1024):                                           # a block of 1024 words in two labels: the same two pairs from every lane
        nodes[hot | v] = SP_A if (v ^ (v >> 2) ^ (v >> 4)) & 1 else SP_B
    st, _, _ = check(tmp_path, monkeypatch, Db(W, 4, sorted(nodes.items())))
    # the label is the parity of the low bits of bases 0, 1, 2: substitutions 1 and 3 at those bases change it, six per word
    assert st.distinct_pairs > 2000 and st.pair_events > 1024 * 6 + 2000


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refused_inputs_leave_no_file(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    monkeypatch.delenv("UTREE_INSPECT_PAIRS", raising=False)
    W = 8
    good = write_db(tmp_path, R.planted(W, 2, 300, 12, LABELS), "good.ubt")
    fails(tmp_path, util.fixture_ctr("toy"), lib.E_UNSUPPORTED, says="first-bin quirk")
    raw, rec = open(good, "rb").read(), W + 2
    x, y = 32 + 100 * rec, 32 + 101 * rec
    swapped = str(tmp_path / "swapped.ubt")
    open(swapped, "wb").write(raw[:x] + raw[y:y + rec] + raw[x:y] + raw[y + rec:])          # two neighbours exchanged: the device finds it
    fails(tmp_path, swapped, lib.E_FORMAT, says="not strictly ascending")
    beyond = bytearray(raw)
    beyond[32 + 299 * rec + W] = len(LABELS)                                                # indices 0 .. len(LABELS) - 1
    open(swapped, "wb").write(bytes(beyond))
    fails(tmp_path, swapped, lib.E_FORMAT, says="names no label line")
    fails(tmp_path, str(tmp_path / "missing.ubt"), lib.E_IO)
    open(swapped, "wb").write(raw[:-2])
    fails(tmp_path, swapped, lib.E_FORMAT)
    with pytest.raises(lib.UtreeError) as e:                                               # a report that cannot be created
        search.inspect(good, str(tmp_path / "no_such_dir" / "r.tsv"), str(tmp_path / "pairs.tsv"))
    assert e.value.code == lib.E_IO and not os.path.exists(str(tmp_path / "pairs.tsv"))


# ---- the command line, and the loop closed with the other tools ----------------------------------------------------------------------------------
def test_command_line(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    monkeypatch.delenv("UTREE_INSPECT_PAIRS", raising=False)
    db = R.planted(8, 2, 200, 13, LABELS)
    p = write_db(tmp_path, db, "db.ctr", ctr=True)
    rep, prs = str(tmp_path / "report.tsv"), str(tmp_path / "pairs.tsv")
    fig, pairs, ws = R.inspect(db)
    want_rep, want_prs = R.files(fig, pairs, ws, (p, ".ctr", 8, 2))
    for args in ([p, rep], [p, rep, prs]):
        for f in (rep, prs):
            if os.path.exists(f):
                os.unlink(f)
        r = subprocess.run([lib.INSPECT_CLI_PATH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.decode().splitlines()
        assert lines[0].startswith("This is UTree")
        assert lines[1] == "%s: .ctr, %d nodes [%d labels]" % (p, len(db.nodes), ws["labels"])
        assert lines[2] == "K-mers: %d, isolated %d, same %d, lineage %d, conflict %d" % tuple(ws[k] for k in R.FIGURES)
        assert lines[3:] == ["conflicts"] and b"[utree_amd] inspect" in r.stderr
        assert open(rep, "rb").read() == want_rep
        assert (open(prs, "rb").read() == want_prs) if len(args) == 3 else not os.path.exists(prs)
    clean = write_db(tmp_path, Db(8, 2, [(w, G) for w, _ in db.nodes]), "clean.ubt")
    r = subprocess.run([lib.INSPECT_CLI_PATH, clean, rep], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout.decode().splitlines()[-1] == "clean"
    os.unlink(rep)
    r = subprocess.run([lib.INSPECT_CLI_PATH, str(tmp_path / "missing.ubt"), rep], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and not os.path.exists(rep) and b"ERROR" in r.stderr
    bad = str(tmp_path / "bad.ubt")
    open(bad, "wb").write(open(clean, "rb").read()[:-2])
    r = subprocess.run([lib.INSPECT_CLI_PATH, bad, rep], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and not os.path.exists(rep)
    os.unlink(prs)                                                 # (an earlier run's)
    r = subprocess.run([lib.INSPECT_CLI_PATH, write_db(tmp_path, pair_db(4), "pairs.ubt"), rep, prs], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, UTREE_INSPECT_PAIRS="4"))
    assert r.returncode == 3 and b"UTREE_INSPECT_PAIRS" in r.stderr and not os.path.exists(rep) and not os.path.exists(prs)
    for args in ([], [p], [p, rep, prs, "more"]):
        r = subprocess.run([lib.INSPECT_CLI_PATH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and b"usage: utree-inspect db.{ubt,ctr} report.tsv [pairs.tsv]" in r.stdout


def test_a_built_database_against_the_compare(tmp_path, monkeypatch):
    """utree-buildGG on the related references of tests/golden, then this tool and `utree-compare db db`: one k-mer count per taxon"""
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    monkeypatch.delenv("UTREE_INSPECT_PAIRS", raising=False)
    fa, mp, ubt = (str(tmp_path / ("rel." + e)) for e in ("fa", "map", "ubt"))
    open(fa, "wb").write(util.fixture_bytes("build_rel.fa.gz"))
    open(mp, "wb").write(util.fixture_bytes("build_rel.map.gz"))
    r = subprocess.run([lib.BUILD_GG_CLI_PATH, fa, mp, ubt, "1", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stdout[-300:]
    db = M.read_ubt(ubt)
    st, rep, _ = check(tmp_path, monkeypatch, db, path=ubt)
    crep = str(tmp_path / "compare.tsv")
    cs = search.compare(ubt, ubt, crep)
    rows = lambda text, first: {l.split(b"\t")[0]: int(l.split(b"\t")[1]) for l in text.split(b"\n")[first:-1]}
    assert rows(rep, 3) == rows(open(crep, "rb").read(), 4) and cs.a == st.kmers == len(db.nodes) > 1000
    assert st.same > 0, "references that are mutated copies of one another hold k-mers one substitution apart"
