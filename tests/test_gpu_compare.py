"""utree_compare_files on the GPU (merge_kernels.hip: compare_runs_k and the move aggregation): every report, every moves file and every
figure of the stats is compared with tests/compare_ref.py, the definition in plain Python.  All figures are integers: nothing is tolerated."""
import os
import subprocess

import numpy as np
import pytest

import build_inputs as B
import compare_ref as R
import merge_edit_ref as E
import merge_ref as M
import util
from utree_amd import ctrfile, lib, search

pytestmark = pytest.mark.gpu
ONES = {4: (1 << 32) - 1, 8: (1 << 64) - 1, 16: (1 << 128) - 1}
Db = M.Db
LA, LB, LX = B.LA.encode(), B.LB.encode(), B.LX.encode()


def as_ctr(db, path, **kw):
    labs = M.parse_labels(M.db_file(db)[32 + len(db.nodes) * (db.W + db.I):])
    ix = np.array([labs.index(l) for _, l in db.nodes], dtype=np.uint32)
    hi = np.array([w >> 64 for w, _ in db.nodes], dtype=np.uint64)
    lo = np.array([w & 0xFFFFFFFFFFFFFFFF for w, _ in db.nodes], dtype=np.uint64)
    ctrfile.write_ctr(path, db.W, db.I, hi, lo, ix, [l.decode("latin-1") for l in labs], **kw)


def write_db(tmp_path, db, name, ctr=False):
    p = str(tmp_path / name)
    if ctr:
        as_ctr(db, p)
    else:
        open(p, "wb").write(M.db_file(db))
    return p


def check(tmp_path, monkeypatch, a, b, pass_nodes=None, paths=None, ctr=(False, False), tag="c"):
    """compare a with b on the device; both files and every figure must be compare_ref's.  Returns (stats, report, moves)."""
    if pass_nodes:
        monkeypatch.setenv("UTREE_TEST_MERGE_PASS_NODES", str(pass_nodes))
    else:
        monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    pa, pb = paths or (write_db(tmp_path, a, tag + "_a.db", ctr[0]), write_db(tmp_path, b, tag + "_b.db", ctr[1]))
    rep, mov = str(tmp_path / (tag + "_report.tsv")), str(tmp_path / (tag + "_moves.tsv"))
    st = search.compare(pa, pb, rep, mov)
    fig, moves, ws = R.compare(a, b)
    R.check_invariants(fig, moves, ws)
    lay = lambda c: ".ctr" if c else ".ubt"
    want_rep, want_mov = R.files(fig, moves, ws, (pa, lay(ctr[0]), a.W, a.I), (pb, lay(ctr[1]), b.W, b.I))
    got_rep, got_mov = open(rep, "rb").read(), open(mov, "rb").read()
    assert got_rep == want_rep
    assert got_mov == want_mov
    assert {k: getattr(st, k) for k in ws} == ws
    assert st.n_passes >= (1 if a.nodes or b.nodes else 0) and st.seconds > 0
    return st, got_rep, got_mov


def fails(tmp_path, pa, pb, code, says=None):
    rep, mov = str(tmp_path / "refused.tsv"), str(tmp_path / "refused_moves.tsv")
    with pytest.raises(lib.UtreeError) as e:
        search.compare(pa, pb, rep, mov)
    assert e.value.code == code, e.value
    assert says is None or says in e.value.detail, e.value.detail
    assert not os.path.exists(rep) and not os.path.exists(mov), "a failed call leaves neither output file behind"


def labelled(words, key, n_labels=5, stem=b"k__A;p__B;c__L"):
    r = M.rng(key)
    return [(w, stem + b"%d" % int(r.integers(0, n_labels))) for w in words]


# ---- input sizes: the wavefront and block edges of the decode and of compare_runs_k ----------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_sizes(n, tmp_path, monkeypatch):
    W = 8
    words = M.random_words(M.rng(1, n), W, 2 * n)
    a = Db(W, 2, labelled(words[0::2], 11))
    st, _, _ = check(tmp_path, monkeypatch, a, Db(W, 2, labelled(words[1::2], 12)), tag="disjoint")
    assert (st.only_a, st.only_b, st.both, st.identical) == (n, n, 0, 0)
    # all words shared under equal texts: B numbers the texts in another order and stores 4-byte indices
    texts = sorted(set(l for _, l in a.nodes), reverse=True)
    pb = str(tmp_path / "renumbered.ubt")
    open(pb, "wb").write(M.ubt_file(W, 4, a.nodes, {t: i for i, t in enumerate(texts)}))
    st, _, mov = check(tmp_path, monkeypatch, a, Db(W, 4, a.nodes), paths=(write_db(tmp_path, a, "a.ubt"), pb), tag="equal")
    assert st.identical == 1 and st.same == n == st.words and mov.count(b"\n") == 1
    st, _, _ = check(tmp_path, monkeypatch, a, Db(W, 2, [(w, l + b";o__x") for w, l in a.nodes]), tag="all")
    assert st.left == n == st.arrived and st.same == 0 and st.identical == 0
    pa = write_db(tmp_path, a, "self.ubt")
    st, _, _ = check(tmp_path, monkeypatch, a, a, paths=(pa, pa), tag="self")                 # a file against itself
    assert st.identical == 1 and st.same == n


# ---- where a run stands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 8, 16])
def test_shared_first_and_last_word(W, tmp_path, monkeypatch):
    mid = [w for w in M.random_words(M.rng(2, W), W, 300) if 0 < w < ONES[W]]
    a = Db(W, 2, sorted([(0, LA)] + labelled(mid[:150], 21) + [(ONES[W], LB)]))
    b = Db(W, 4, sorted([(0, LB)] + labelled(mid[100:], 22) + [(ONES[W], LA)]))
    st, _, mov = check(tmp_path, monkeypatch, a, b)
    assert st.both == 52 and LA + b"\t" + LB + b"\t1\tmoved\n" in mov and LB + b"\t" + LA + b"\t1\tmoved\n" in mov
    check(tmp_path, monkeypatch, a, b, pass_nodes=64, tag="p")
    check(tmp_path, monkeypatch, b, a, ctr=(True, False) if W != 4 else (False, False), tag="rev")


def test_run_across_a_block_edge(tmp_path, monkeypatch):
    """the one shared word stands at positions 255 and 256 of the sorted sequence: the run's head is the last thread of a block"""
    W = 8
    words = M.random_words(M.rng(3), W, 400)
    x = words[255]
    a = Db(W, 2, sorted(labelled(words[0:255:2], 30) + [(x, LA)] + labelled(words[256::2], 40)))
    b = Db(W, 2, sorted(labelled(words[1:255:2], 31) + [(x, LB)] + labelled(words[257::2], 41)))
    st, _, _ = check(tmp_path, monkeypatch, a, b)
    assert st.both == 1 and st.left == 1
    st, _, _ = check(tmp_path, monkeypatch, a, Db(W, 2, [(w, LA if w == x else l) for w, l in b.nodes]), tag="same")
    assert st.both == 1 and st.same == 1


# ---- passes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pass_nodes", [64, 100])
def test_passes(pass_nodes, tmp_path, monkeypatch):
    """every fourth word is in both inputs, so whichever nodes a pass ends on, runs stand at both sides of its boundary"""
    W = 8
    words = M.random_words(M.rng(4), W, 500)
    a = Db(W, 2, labelled(words[0::2], 51, 3))
    b = Db(W, 2, labelled([w for j, w in enumerate(words) if j % 2 == 1 or j % 4 == 0], 52, 3))
    one, rep1, mov1 = check(tmp_path, monkeypatch, a, b, tag="one")
    assert one.n_passes == 1 and one.both == 125
    for ctr in ((False, False), (True, True), (True, False)):
        pa, pb = write_db(tmp_path, a, "pa.db", ctr[0]), write_db(tmp_path, b, "pb.db", ctr[1])
        st, _, mov = check(tmp_path, monkeypatch, a, b, pass_nodes=pass_nodes, paths=(pa, pb), ctr=ctr, tag="many")
        assert st.n_passes > 1 and mov == mov1                                             # the moves add up across the passes
        if ctr == (False, False):
            same_names, _, _ = check(tmp_path, monkeypatch, a, b, paths=(pa, pb), tag="again")
            assert open(str(tmp_path / "many_report.tsv"), "rb").read() == open(str(tmp_path / "again_report.tsv"), "rb").read()


def test_words_of_one_prefix_stay_in_one_pass(tmp_path, monkeypatch):
    W = 8
    words = [(0xABCDEF << 40) | v for v in range(0, 600, 2)]
    st, _, _ = check(tmp_path, monkeypatch, Db(W, 2, labelled(words, 51)), Db(W, 2, labelled(words[::3], 52)), pass_nodes=64)
    assert st.n_passes == 1 and st.both == 100


def test_many_moves(tmp_path, monkeypatch):
    """some thousands of distinct (label in A, label in B) pairs: the key sort and the run-length encoding at more than one block, and, in
    passes of 256 nodes, the accumulation of one pair over many passes"""
    W = 8
    r = M.rng(6)
    words = M.random_words(r, W, 2400)
    la = [b"k__A;p__P%d;c__a%d" % (i % 7, i) for i in range(300)]
    lb = [b"k__A;p__P%d;c__b%d" % (i % 5, i) for i in range(300)]
    a = Db(W, 2, [(w, la[int(r.integers(0, 300))]) for w in words[:2000]])
    b = Db(W, 4, [(w, lb[int(r.integers(0, 300))]) for w in words[400:]])
    st, rep, mov = check(tmp_path, monkeypatch, a, b)
    assert st.n_passes == 1 and st.both == 1600 == st.left and 1000 < st.n_moves <= 1600 and st.a + st.b == 4000
    many, rep2, mov2 = check(tmp_path, monkeypatch, a, b, pass_nodes=256, paths=(str(tmp_path / "c_a.db"), str(tmp_path / "c_b.db")), tag="p")
    assert many.n_passes > 8 and mov2 == mov and many.n_moves == st.n_moves


def test_k64_halves(tmp_path, monkeypatch):
    """W = 16 sorts its halves one after the other: words equal in the high half and different in the low, and the reverse"""
    r = M.rng(5)
    H = [int.from_bytes(r.bytes(8), "little") for _ in range(8)]
    Lo = [int.from_bytes(r.bytes(8), "little") for _ in range(8)]
    words = sorted((h << 64) | l for h in H for l in Lo)
    a = Db(16, 2, [(w, LA) for w in words[:48]])
    b = Db(16, 2, [(w, LB if j % 2 else LA) for j, w in enumerate(words) if j >= 16])
    st, _, _ = check(tmp_path, monkeypatch, a, b)
    assert (st.only_a, st.both, st.only_b, st.left) == (16, 32, 16, 16)


# ---- layouts --------------------------------------------------------------------------------------------------------------------------------
def fixture_nodes(name):
    """a fixture database's nodes from the first prefix on that holds two nodes (what stands in front of it xtree-compress's first-bin quirk
    leaves addressable only under a wrong prefix, and a first prefix of one node would make our own xtree-compress write such a file)"""
    if name == "w8":
        return 8, 2, labelled(M.random_words(M.rng(7), 8, 300, spread=False), 71)          # all under prefix 0
    d = util.load_db_fixture(name)
    nodes = M.read_ctr(util.fixture_ctr(name)).nodes
    shift = {4: 8, 8: 40, 16: 104}[d.W]
    s = 0
    while nodes[s + 1][0] <= nodes[s][0] or (nodes[s + 1][0] >> shift) != (nodes[s][0] >> shift):
        s += 1
    return d.W, d.I, nodes[s:]


@pytest.mark.parametrize("name", ["k64", "k16", "w8"])
def test_ubt_against_its_ctr_is_identical(name, tmp_path, monkeypatch):
    W, I, nodes = fixture_nodes(name)
    db = Db(W, I, nodes)
    ubt, ctr = write_db(tmp_path, db, name + ".ubt"), str(tmp_path / (name + ".ctr"))
    code, _ = search.compress(ubt, ctr)
    assert code == lib.OK and search.merge_probe(ctr).is_ctr == 1
    st, _, _ = check(tmp_path, monkeypatch, db, db, paths=(ubt, ctr), ctr=(False, True))
    assert st.identical == 1 and st.same == len(nodes)
    st, _, _ = check(tmp_path, monkeypatch, db, db, paths=(ctr, ubt), ctr=(True, False), pass_nodes=1000, tag="rev")
    assert st.identical == 1
    # a `.ctr` against a `.ctr`: every seventh word under a deeper label
    other = Db(W, I, [(w, l + b";x__y") if j % 7 == 0 else (w, l) for j, (w, l) in enumerate(nodes)])
    oc = str(tmp_path / "other.ctr")
    assert search.compress(write_db(tmp_path, other, "other.ubt"), oc)[0] == lib.OK
    st, _, mov = check(tmp_path, monkeypatch, db, other, paths=(ctr, oc), ctr=(True, True), tag="cc")
    assert st.left == (len(nodes) + 6) // 7 and mov.count(b"\tlowered\n") == st.n_moves


def test_label_lines_no_node_carries_and_repeated_lines(tmp_path, monkeypatch):
    W, I = 8, 2
    words = M.random_words(M.rng(9), W, 6)
    a = Db(W, I, [(words[0], LA), (words[2], LB)])
    # b: line 0 = LB, line 1 = LA, line 2 = LB again (as the loader reads it: the text of index 0), line 3 a text no node carries
    recs = b"".join(M.word_bytes(W, w) + ix.to_bytes(I, "little") for w, ix in ((words[1], 1), (words[2], 0), (words[4], 1)))
    raw = np.array([W, 0, I, 3], dtype="<u8").tobytes() + recs + LB + b"\t1\n" + LA + b"\t1\n" + LB + b"\t0\n" + b"k__Never;p__Seen\t1\n"
    pb = str(tmp_path / "b.ubt")
    open(pb, "wb").write(raw)
    pa = str(tmp_path / "a.ubt")
    open(pa, "wb").write(M.db_file(a, extra_labels=[b"k__Unused;p__Line"]))
    b = Db(W, I, [(words[1], LA), (words[2], LB), (words[4], LA)])
    st, rep, _ = check(tmp_path, monkeypatch, a, b, paths=(pa, pb))
    assert (st.a_labels, st.b_labels, st.same) == (2, 2, 1) and b"k__Never" not in rep and b"k__Unused" not in rep


# ---- against the merge, end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_way_cut", "genus_to_family", "bad_stays_bad", "plain_build", "order_021"])
def test_what_a_merge_did(name, tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    inputs, gg = M.fold_cases()[name]
    paths = [write_db(tmp_path, db, "in%d.ubt" % i) for i, db in enumerate(inputs)]
    out = str(tmp_path / "merged.ubt")
    ms = search.merge(paths, out, gg=gg)
    merged = M.read_ubt(out)
    tree, _, _ = M.fold(inputs, gg)
    for i, db in enumerate(inputs):
        st, _, mov = check(tmp_path, monkeypatch, db, merged, paths=(paths[i], out), tag="m%d" % i)
        assert st.only_a == sum(tree[w] is M.BAD for w, _ in db.nodes), "what an input loses is what the fold dropped as BAD"
        assert mov.count(b"\tlifted\n") == st.n_moves, "the fold only ever lifts"
        assert st.b == ms.n_nodes and st.a == len(db.nodes)


def test_what_a_subtraction_did(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    W = 8
    words = M.random_words(M.rng(14), W, 600)
    a = Db(W, 2, labelled(words[:500], 81))
    m = Db(W, 2, [(w, b"k__Host") for w in words[450:]])
    pa, pm, out = write_db(tmp_path, a, "a.ubt"), write_db(tmp_path, m, "m.ubt"), str(tmp_path / "clean.ubt")
    _, es = search.merge_edit([pa], out, minus=[pm])
    st, _, _ = check(tmp_path, monkeypatch, a, M.read_ubt(out), paths=(pa, out))
    assert st.only_a == es.n_nodes_subtracted == 50 and (st.left, st.only_b, st.same) == (0, 0, 450)


def test_what_a_rename_did(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    W = 8
    a = Db(W, 2, labelled(M.random_words(M.rng(15), W, 400), 82))
    old, new = b"k__A;p__B;c__L2", b"k__A;p__Bacillota;c__L2"
    rn = str(tmp_path / "rename.tsv")
    open(rn, "wb").write(E.rule_file([(old, new)]))
    pa, out = write_db(tmp_path, a, "a.ubt"), str(tmp_path / "renamed.ubt")
    search.merge_edit([pa], out, rename=rn)
    n_old = sum(l == old for _, l in a.nodes)
    st, _, mov = check(tmp_path, monkeypatch, a, M.read_ubt(out), paths=(pa, out))
    assert mov == b"# from\tto\tkmers\tkind\n" + old + b"\t" + new + b"\t%d\tmoved\n" % n_old, "every change is the rename"
    assert (st.only_a, st.only_b, st.left) == (0, 0, n_old) and n_old > 0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refused_inputs_leave_no_file(tmp_path):
    W = 8
    good = write_db(tmp_path, Db(W, 2, labelled(M.random_words(M.rng(12), W, 300), 61)), "good.ubt")
    other_w = write_db(tmp_path, Db(16, 2, [(5, b"k__A;p__B")]), "w16.ubt")
    fails(tmp_path, good, other_w, lib.E_UNSUPPORTED, says="word size differs")
    fails(tmp_path, other_w, good, lib.E_UNSUPPORTED, says="word size differs")
    fails(tmp_path, good, util.fixture_ctr("toy"), lib.E_UNSUPPORTED, says="first-bin quirk")
    fails(tmp_path, util.fixture_ctr("toy"), good, lib.E_UNSUPPORTED, says="first-bin quirk")
    z = np.load(os.path.join(util.GOLD, "cq_unsorted_ubt.npz"))
    unsorted = str(tmp_path / "unsorted.ubt")
    ctrfile.write_ubt(unsorted, 8, 2, np.zeros_like(z["lo"]), z["lo"], z["ix"], z["tail"].tobytes())
    fails(tmp_path, good, unsorted, lib.E_FORMAT)                                          # (its tail does not count its nodes: the reader stops there)
    fails(tmp_path, unsorted, good, lib.E_FORMAT)
    raw, rec = open(good, "rb").read(), W + 2
    x, y = 32 + 100 * rec, 32 + 101 * rec
    swapped = str(tmp_path / "swapped.ubt")
    open(swapped, "wb").write(raw[:x] + raw[y:y + rec] + raw[x:y] + raw[y + rec:])          # two neighbours exchanged: the device finds it
    fails(tmp_path, good, swapped, lib.E_FORMAT, says="not strictly ascending")
    fails(tmp_path, swapped, swapped, lib.E_FORMAT, says="not strictly ascending")
    beyond = bytearray(raw)
    beyond[32 + 299 * rec + W] = 5                                                          # five labels: indices 0 .. 4
    open(swapped, "wb").write(bytes(beyond))
    fails(tmp_path, swapped, good, lib.E_FORMAT, says="names no label line")
    fails(tmp_path, good, str(tmp_path / "missing.ubt"), lib.E_IO)
    with pytest.raises(lib.UtreeError) as e:                                               # a report that cannot be created
        search.compare(good, good, str(tmp_path / "no_such_dir" / "r.tsv"), str(tmp_path / "moves.tsv"))
    assert e.value.code == lib.E_IO and not os.path.exists(str(tmp_path / "moves.tsv"))


# ---- the command lines ----------------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    (a, b), _ = M.fold_cases()["two_way_cut"]
    pa, pb = write_db(tmp_path, a, "old.ubt"), write_db(tmp_path, b, "new.ctr", ctr=True)
    rep, mov = str(tmp_path / "report.tsv"), str(tmp_path / "moves.tsv")
    fig, moves, ws = R.compare(a, b)
    want_rep, want_mov = R.files(fig, moves, ws, (pa, ".ubt", 8, 2), (pb, ".ctr", 8, 2))
    for args in ([pa, pb, rep], [pa, pb, rep, mov]):
        for f in (rep, mov):
            if os.path.exists(f):
                os.unlink(f)
        p = subprocess.run([lib.COMPARE_CLI_PATH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.decode().splitlines()
        assert lines[0].startswith("This is UTree")
        assert lines[1] == "%s: .ubt, %d nodes [%d labels]" % (pa, len(a.nodes), ws["a_labels"])
        assert lines[2] == "%s: .ctr, %d nodes [%d labels]" % (pb, len(b.nodes), ws["b_labels"])
        assert lines[3] == "Words: %d, both %d, same %d, changed %d, only in old %d, only in new %d" % (
            ws["words"], ws["both"], ws["same"], ws["left"], ws["only_a"], ws["only_b"])
        assert lines[4:] == ["different"] and b"[utree_amd] compare" in p.stderr
        assert open(rep, "rb").read() == want_rep
        assert (open(mov, "rb").read() == want_mov) if len(args) == 4 else not os.path.exists(mov)
    p = subprocess.run([lib.COMPARE_CLI_PATH, pa, pa, rep], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and p.stdout.decode().splitlines()[-1] == "identical"
    os.unlink(rep)
    p = subprocess.run([lib.COMPARE_CLI_PATH, pa, str(tmp_path / "missing.ubt"), rep], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and not os.path.exists(rep) and b"ERROR" in p.stderr
    bad = str(tmp_path / "bad.ubt")
    open(bad, "wb").write(open(pa, "rb").read()[:-2])
    p = subprocess.run([lib.COMPARE_CLI_PATH, pa, bad, rep], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 2 and not os.path.exists(rep)
    for args in ([], [pa, pb], [pa, pb, rep, mov, "more"]):
        p = subprocess.run([lib.COMPARE_CLI_PATH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and b"usage: utree-compare old.{ubt,ctr} new.{ubt,ctr} report.tsv [moves.tsv]" in p.stdout


def test_the_other_command_lines_are_unchanged(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    monkeypatch.delenv("UTREE_IXTYPE", raising=False)
    inputs, gg = M.fold_cases()["two_way_cut"]
    paths = [write_db(tmp_path, db, "in%d.ubt" % i) for i, db in enumerate(inputs)]
    out = str(tmp_path / "cli.ubt")
    p = subprocess.run([lib.MERGE_GG_CLI_PATH, out] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    want, ws = M.merge(inputs, True)
    assert p.returncode == 0 and open(out, "rb").read() == want
    assert p.stdout.decode().splitlines()[3:] == ["Total nodes in tree: %d [%d labels]" % (ws["n_nodes"], ws["n_labels"]), "Tree written."]
    fa, txt = str(tmp_path / "reads.fa"), str(tmp_path / "out.txt")
    open(fa, "wb").write(util.fixture_bytes("toy_reads.fa.gz")[:200000].rsplit(b">", 1)[0])
    p = subprocess.run([lib.CLI_PATH, util.fixture_ctr("toy"), fa, txt, "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    got = open(txt, "rb").read()
    assert got and util.fixture_bytes("toy_out.txt.gz").startswith(got)
