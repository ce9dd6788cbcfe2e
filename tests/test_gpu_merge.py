"""utree_merge_files on the GPU (merge_kernels.hip): every output file is compared byte for byte with tests/merge_ref.py, the definition in
plain Python that test_merge_cpu.py pins to the genuine builder; a few cases are compared with the genuine builder right here."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import build_inputs as B
import merge_ref as M
import util
from oracle import orc
from utree_amd import ctrfile, lib, search

pytestmark = pytest.mark.gpu
REF = os.path.join(util.ROOT, "oracle", "_ref")
ONES = {4: (1 << 32) - 1, 8: (1 << 64) - 1, 16: (1 << 128) - 1}
Db = M.Db


def write_inputs(tmp_path, inputs, tag="in"):
    paths = []
    for i, db in enumerate(inputs):
        p = str(tmp_path / ("%s%d.ubt" % (tag, i)))
        open(p, "wb").write(M.db_file(db))
        paths.append(p)
    return paths


def check(tmp_path, monkeypatch, inputs, gg=True, I=0, pass_nodes=None, paths=None, tag="in"):
    """merge the inputs on the device; the file and the counters must be merge_ref's.  Returns the stats."""
    if pass_nodes:
        monkeypatch.setenv("UTREE_TEST_MERGE_PASS_NODES", str(pass_nodes))
    else:
        monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    paths = paths or write_inputs(tmp_path, inputs, tag)
    out = str(tmp_path / (tag + "_out.ubt"))
    st = search.merge(paths, out, gg=gg, I=I)
    want, ws = M.merge(inputs, gg, I)
    assert open(out, "rb").read() == want
    assert {k: getattr(st, k) for k in ws} == ws
    assert (st.W, st.I, st.n_inputs) == (inputs[0].W, I or max(d.I for d in inputs), len(inputs)) and st.n_passes >= (1 if ws["n_in_nodes"] else 0)
    assert not os.path.exists(out + ".log") and not os.path.exists(out + ".gg.log")
    return st


def fails(tmp_path, paths, code, gg=True, I=0, says=None):
    out = str(tmp_path / "refused.ubt")
    with pytest.raises(lib.UtreeError) as e:
        search.merge(paths, out, gg=gg, I=I)
    assert e.value.code == code, e.value
    assert says is None or says in e.value.detail, e.value.detail
    assert not os.path.exists(out), "a failed call leaves no output file behind"


def labelled(words, key, n_labels=5, stem=b"k__A;p__B;c__L"):
    r = M.rng(key)
    return [(w, stem + b"%d" % int(r.integers(0, n_labels))) for w in words]


# ---- input sizes: the decode and fold kernels' wavefront and block edges --------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_sizes(n, tmp_path, monkeypatch):
    W, I = 8, 2
    words = M.random_words(M.rng(1, n), W, 2 * n)
    a = Db(W, I, labelled(words[0::2], 11))
    b = Db(W, I, labelled(words[1::2], 12))
    check(tmp_path, monkeypatch, [a, b], tag="disjoint")                                   # no shared word
    c = Db(W, I, [(w, l + b";o__x") for w, l in a.nodes])
    st = check(tmp_path, monkeypatch, [a, c], tag="all")                                   # all words shared, every one relabelled
    assert st.n_shared == n == st.n_nodes
    st = check(tmp_path, monkeypatch, [a, a], paths=write_inputs(tmp_path, [a]) * 2, tag="self")   # an input merged with itself
    assert st.n_shared == n and st.n_relabelled == 0 and st.n_dropped == 0


# ---- where a shared run stands --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 8, 16])
def test_shared_first_and_last_word(W, tmp_path, monkeypatch):
    LA, LB = B.LA.encode(), B.LB.encode()
    mid = [w for w in M.random_words(M.rng(2, W), W, 300) if 0 < w < ONES[W]]
    a = Db(W, 2, [(0, LA)] + labelled(mid[:150], 21) + [(ONES[W], LB)])
    b = Db(W, 2, [(0, LB)] + labelled(mid[150:], 22) + [(ONES[W], LA)])
    b = Db(W, 2, sorted(b.nodes))
    a = Db(W, 2, sorted(a.nodes))
    st = check(tmp_path, monkeypatch, [a, b])
    assert st.n_shared == 2 and st.n_relabelled == 2
    check(tmp_path, monkeypatch, [a, b], pass_nodes=64, tag="p")


def test_run_across_a_block_edge(tmp_path, monkeypatch):
    """three equal words at indices 254, 255, 256 of the sorted sequence: the run's head is the last but one thread of a block"""
    W, I = 8, 2
    words = M.random_words(M.rng(3), W, 400)
    x = words[254]
    lab = (B.LA.encode(), B.LB.encode(), B.LX.encode())
    ins = [Db(W, I, sorted(labelled(words[i:254:3], 30 + i) + [(x, lab[i])] + labelled(words[255 + i::3], 40 + i))) for i in range(3)]
    st = check(tmp_path, monkeypatch, ins)
    assert st.n_shared == 1 and st.n_relabelled == 1
    check(tmp_path, monkeypatch, ins[::-1], tag="rev")


@pytest.mark.parametrize("pass_nodes", [64, 100])
def test_run_at_a_pass_boundary(pass_nodes, tmp_path, monkeypatch):
    """every fourth word is shared by both inputs, so whichever nodes a pass ends on, runs stand at both sides of its boundary"""
    W, I = 8, 2
    words = M.random_words(M.rng(4), W, 500)
    a = Db(W, I, [(w, B.LA.encode()) for w in words[0::2]])
    b = Db(W, I, [(w, B.LB.encode()) for j, w in enumerate(words) if j % 2 == 1 or j % 4 == 0])
    st = check(tmp_path, monkeypatch, [a, b], pass_nodes=pass_nodes)
    assert st.n_passes > 1 and st.n_shared == 125 and st.n_relabelled == 125
    one = check(tmp_path, monkeypatch, [a, b], tag="one")
    assert one.n_passes == 1
    # the same through `.ctr` inputs: a pass's slice is then a range of bins
    ctrs = []
    for i, db in enumerate((a, b)):
        p = str(tmp_path / ("c%d.ctr" % i))
        as_ctr(db, p)
        ctrs.append(p)
    st = check(tmp_path, monkeypatch, [a, b], pass_nodes=pass_nodes, paths=ctrs, tag="ctr")
    assert st.n_passes > 1


def test_words_of_one_prefix_stay_in_one_pass(tmp_path, monkeypatch):
    """passes cut between 24-bit prefixes: words that share one are one pass however small the cap"""
    W, I = 8, 2
    words = [(0xABCDEF << 40) | v for v in range(0, 600, 2)]
    a = Db(W, I, labelled(words, 51))
    b = Db(W, I, labelled(words[::3], 52))
    st = check(tmp_path, monkeypatch, [a, b], pass_nodes=64)
    assert st.n_passes == 1


# ---- the fold -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.fold_cases()))
def test_fold(name, tmp_path, monkeypatch):
    inputs, gg = M.fold_cases()[name]
    st = check(tmp_path, monkeypatch, inputs, gg=gg)
    if name == "all_dropped":
        assert st.n_nodes == 0 and st.n_dropped == 2 and st.n_labels == 3                   # N = 0 is written, and the call is UTREE_OK


def test_the_order_of_the_inputs_matters(tmp_path, monkeypatch):
    outs = set()
    for perm in itertools.permutations(range(3)):
        inputs, gg = M.fold_cases()["order_%d%d%d" % perm]
        outs.add(M.merge(inputs, gg)[0])
    assert len(outs) > 1


# ---- widths ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,I", [(4, 2), (4, 4), (16, 2), (16, 4), (8, 4)])
@pytest.mark.parametrize("name", ["two_way_cut", "genus_to_family", "order_021", "plain_build"])
def test_fold_other_widths(W, I, name, tmp_path, monkeypatch):
    inputs, gg = M.fold_cases(W, I)[name]
    check(tmp_path, monkeypatch, inputs, gg=gg)
    check(tmp_path, monkeypatch, inputs, gg=gg, pass_nodes=64, tag="p")


def test_k64_halves(tmp_path, monkeypatch):
    """W = 16 sorts its halves one after the other: words equal in the high half and different in the low, and the reverse"""
    r = M.rng(5)
    H = [int.from_bytes(r.bytes(8), "little") for _ in range(8)]
    Lo = [int.from_bytes(r.bytes(8), "little") for _ in range(8)]
    words = sorted((h << 64) | l for h in H for l in Lo)
    lab = (B.LA.encode(), B.LB.encode(), B.LX.encode())
    ins = [Db(16, 2, [(w, lab[i]) for w in words]) for i in range(3)]
    st = check(tmp_path, monkeypatch, ins)                                                  # LA, LB, LX in this order: every word at "k__A;p__B"
    assert st.n_nodes == 64 and st.n_relabelled == 64
    st = check(tmp_path, monkeypatch, [ins[0], ins[2], ins[1]], tag="bad")                  # any other order ends BAD
    assert st.n_dropped == 64


@pytest.mark.parametrize("Ia,Ib,I", [(2, 2, 0), (4, 4, 0), (2, 4, 0), (4, 2, 0), (2, 2, 4), (4, 4, 2), (2, 4, 2)])
def test_index_widths(Ia, Ib, I, tmp_path, monkeypatch):
    a, b = M.fold_cases(8, 2)["two_way_cut"][0]
    st = check(tmp_path, monkeypatch, [Db(8, Ia, a.nodes), Db(8, Ib, b.nodes)], I=I)
    assert st.I == (I or max(Ia, Ib))


def test_too_many_labels_for_two_bytes(tmp_path, monkeypatch):
    """65 535 distinct labels: index 65 534 would be EMPTY_IX"""
    W = 8
    words = M.random_words(M.rng(6), W, 65535)
    a = Db(W, 2, [(w, b"k__A;p__%d" % j) for j, w in enumerate(words[:40000])])
    b = Db(W, 2, [(w, b"k__A;p__%d" % (40000 + j)) for j, w in enumerate(words[40000:])])
    paths = write_inputs(tmp_path, [a, b])
    fails(tmp_path, paths, lib.E_UNSUPPORTED, says="4-byte index")
    fails(tmp_path, paths, lib.E_UNSUPPORTED, I=2, says="UTREE_IXTYPE=32")
    st = check(tmp_path, monkeypatch, [a, b], I=4, paths=paths)
    assert st.n_labels == 65535
    b2 = Db(W, 2, b.nodes[:-1])                                                             # 65 534 labels fit
    st = check(tmp_path, monkeypatch, [a, b2], tag="fit")
    assert st.n_labels == 65534 and st.I == 2


def test_hostile_label_bytes(tmp_path, monkeypatch):
    """every byte a label line can hold (0x01-0x7F without TAB and LF) inside label tokens, also next to the ';' the cut looks for"""
    alpha = bytes(b for b in B.HOSTILE if b not in (9, 0x3B))
    r = M.rng(7)
    words = M.random_words(r, 8, 120)

    def tok():
        return bytes(alpha[int(c)] for c in r.integers(0, len(alpha), int(r.integers(1, 9))))
    stems = [b";".join([b"k__" + tok(), tok(), tok()]) for _ in range(6)]
    lab = lambda: stems[int(r.integers(0, 6))] + b";" + tok() + (b";" + tok() if r.random() < 0.5 else b"")
    a = Db(8, 2, [(w, lab()) for w in words[:80]])
    b = Db(8, 2, [(w, lab()) for w in words[40:]])
    c = Db(8, 2, [(w, lab()) for w in words[20:100]])
    st = check(tmp_path, monkeypatch, [a, b, c])
    assert st.n_shared == 80 and st.n_relabelled > 0
    check(tmp_path, monkeypatch, [c, b, a], gg=False, tag="plain")


def test_eight_inputs(tmp_path, monkeypatch):
    r = M.rng(8)
    words = M.random_words(r, 8, 400)
    labs = [s for s in M.SIBLINGS] + [B.LA.encode(), B.LB.encode(), B.LX.encode(), B.LC.encode(), B.LD.encode()]
    ins = []
    for i in range(8):
        pick = sorted(set(int(j) for j in r.integers(0, 400, 150)))
        ins.append(Db(8, 2 if i % 2 else 4, [(words[j], labs[int(r.integers(0, len(labs)))]) for j in pick]))
    st = check(tmp_path, monkeypatch, ins)
    assert st.n_inputs == 8 and st.n_dropped > 0 and st.n_relabelled > 0
    check(tmp_path, monkeypatch, ins, pass_nodes=100, tag="p")


def test_label_lines_no_node_carries_and_repeated_lines(tmp_path, monkeypatch):
    W, I = 8, 2
    words = M.random_words(M.rng(9), W, 6)
    LA, LB = B.LA.encode(), B.LB.encode()
    a = Db(W, I, [(words[0], LA), (words[2], LB)])
    # input b: line 0 = LB, line 1 = LA, line 2 = LB again (as the loader reads it: the text of index 0), line 3 a text no node carries;
    # its nodes use the distinct texts' indices 0 (LB) and 1 (LA)
    recs = b"".join(M.word_bytes(W, w) + ix.to_bytes(I, "little") for w, ix in ((words[1], 1), (words[2], 0), (words[4], 1)))
    raw = np.array([W, 0, I, 3], dtype="<u8").tobytes() + recs + LB + b"\t1\n" + LA + b"\t1\n" + LB + b"\t0\n" + b"k__Never;p__Seen\t1\n"
    pb = str(tmp_path / "b.ubt")
    open(pb, "wb").write(raw)
    b = Db(W, I, [(words[1], LA), (words[2], LB), (words[4], LA)])
    pa = write_inputs(tmp_path, [a])[0]
    st = check(tmp_path, monkeypatch, [a, b], paths=[pa, pb])
    assert st.n_labels == 2                                                                 # the unused line is not carried over


# ---- against the genuine builder, right here --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,I,gg", [(8, 2, True), (8, 2, False), (16, 2, True), (16, 2, False), (4, 2, True), (4, 2, False), (8, 4, True), (16, 4, True)])
def test_output_is_the_genuine_builders(W, I, gg, tmp_path, monkeypatch):
    """one case per (W, I, mode) the reference ships a builder for: the product's file = the builder's `.ubt` on the imagined FASTA
    (oracle/_ref's binary where it has been compiled, the oracle's restatement of it everywhere)"""
    r = M.rng(10, W, I, gg)
    words = M.random_words(r, W, 300)
    labs = [s for s in M.SIBLINGS] + [B.LA.encode(), B.LB.encode(), B.LX.encode(), B.LC.encode(), B.LD.encode(), B.LE.encode(), B.LF.encode()]
    ins = []
    for i in range(3):
        pick = sorted(set(int(j) for j in r.integers(0, 300, 150)))
        ins.append(Db(W, I, [(words[j], labs[int(r.integers(0, len(labs)))]) for j in pick]))
    check(tmp_path, monkeypatch, ins, gg=gg)
    got = open(str(tmp_path / "in_out.ubt"), "rb").read()
    fa, mp = M.imagined(ins)
    fa_p, mp_p = str(tmp_path / "im.fa"), str(tmp_path / "im.map")
    open(fa_p, "wb").write(fa)
    open(mp_p, "wb").write(mp)
    code, _, _, _, err = orc.build_file(fa_p, mp_p, str(tmp_path / "orc.ubt"), W=W, I=I, complevel=0, gg=gg)
    assert code == 0, err
    assert got == open(str(tmp_path / "orc.ubt"), "rb").read()
    exe = os.path.join(REF, M.reference_binary(W, I, gg))
    if os.path.exists(exe):
        p = subprocess.run([exe, fa_p, mp_p, str(tmp_path / "ref.ubt"), "1", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stdout[-300:]
        assert got == open(str(tmp_path / "ref.ubt"), "rb").read()


# ---- `.ctr` inputs --------------------------------------------------------------------------------------------------------------------------
def as_ctr(db, path, **kw):
    labs = M.parse_labels(M.db_file(db)[32 + len(db.nodes) * (db.W + db.I):])
    ix = np.array([labs.index(l) for _, l in db.nodes], dtype=np.uint32)
    hi = np.array([w >> 64 for w, _ in db.nodes], dtype=np.uint64)
    lo = np.array([w & 0xFFFFFFFFFFFFFFFF for w, _ in db.nodes], dtype=np.uint64)
    ctrfile.write_ctr(path, db.W, db.I, hi, lo, ix, [l.decode("latin-1") for l in labs], **kw)


def fixture_ubt(name, tmp_path):
    """A fixture database as a `.ubt`: its words rebuilt from the bins, from the first prefix on that holds two nodes -- xtree-compress's
    first-bin quirk leaves what stands in front of that addressable only under a wrong prefix (toy: node 0; the file itself is refused,
    test_refused_inputs_leave_no_file), and a first prefix of one node would make our own xtree-compress write such a file again."""
    nodes = M.read_ctr(util.fixture_ctr(name)).nodes
    shift = {4: 8, 8: 40, 16: 104}[util.load_db_fixture(name).W]          # a word's top 24 bits
    s = 0
    while nodes[s + 1][0] <= nodes[s][0] or (nodes[s + 1][0] >> shift) != (nodes[s][0] >> shift):
        s += 1
    d = util.load_db_fixture(name)
    p = str(tmp_path / (name + ".ubt"))
    open(p, "wb").write(M.db_file(Db(d.W, d.I, nodes[s:])))
    return p


@pytest.mark.parametrize("name", ["toy", "k64", "k16"])
def test_ctr_input_merges_as_its_ubt(name, tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    ubt = fixture_ubt(name, tmp_path)
    ctr = str(tmp_path / (name + ".ctr"))
    code, _ = search.compress(ubt, ctr)
    assert code == lib.OK
    assert search.merge_probe(ctr).is_ctr == 1 and search.merge_probe(ubt).is_ctr == 0
    db = M.read_ubt(ubt)
    want, ws = M.merge([db], True)
    outs = []
    for tag, src in (("u", ubt), ("c", ctr)):
        out = str(tmp_path / (tag + ".ubt"))
        st = search.merge([src], out)
        assert st.n_nodes == ws["n_nodes"] == len(db.nodes) and st.n_shared == 0
        outs.append(open(out, "rb").read())
    assert outs[0] == want and outs[1] == want
    # one `.ctr` in, compressed again: the same (word, label text) set and bin table as the original (the inverse of xtree-compress)
    back = str(tmp_path / "back.ctr")
    code, _ = search.compress(str(tmp_path / "c.ubt"), back)
    assert code == lib.OK
    d0, d1 = ctrfile.read_ctr(ctr), ctrfile.read_ctr(back)
    assert np.array_equal(d0.binix, d1.binix)
    assert M.read_ctr(ctr).nodes == M.read_ctr(back).nodes
    # the `.ctr` against a second input, in many passes
    other = Db(db.W, db.I, [(w, l + b";x__y") for w, l in db.nodes[::7]])
    po = write_inputs(tmp_path, [other], tag="other")[0]
    monkeypatch.setenv("UTREE_TEST_MERGE_PASS_NODES", "1000")
    out = str(tmp_path / "two.ubt")
    st = search.merge([ctr, po], out)
    assert open(out, "rb").read() == M.merge([db, other], True)[0] and st.n_shared == len(other.nodes)


def test_refused_inputs_leave_no_file(tmp_path):
    W, I = 8, 2
    db = Db(W, I, labelled(M.random_words(M.rng(12), W, 300), 61))
    good = write_inputs(tmp_path, [db])[0]
    raw = M.db_file(db)
    rec = W + I

    def variant(name, data):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        return p
    a, b = 32 + 100 * rec, 32 + 101 * rec
    swapped = variant("swapped.ubt", raw[:a] + raw[b:b + rec] + raw[a:b] + raw[b + rec:])
    fails(tmp_path, [good, swapped], lib.E_FORMAT, says="not strictly ascending")
    twice = variant("twice.ubt", raw[:b] + raw[a:b] + raw[b + rec:])                        # a word repeated is not strictly ascending either
    fails(tmp_path, [twice], lib.E_FORMAT, says="not strictly ascending")
    beyond = bytearray(raw)
    beyond[32 + 299 * rec + W] = 5                                                          # five labels: indices 0 .. 4
    fails(tmp_path, [variant("beyond.ubt", bytes(beyond)), good], lib.E_FORMAT, says="names no label line")
    fails(tmp_path, [good, variant("cut.ubt", raw[:-3])], lib.E_FORMAT)                     # a truncated tail
    fails(tmp_path, [good, str(tmp_path / "missing.ubt")], lib.E_IO)
    other_w = write_inputs(tmp_path, [Db(16, I, [(5, b"k__A;p__B")])], tag="w16")[0]
    fails(tmp_path, [good, other_w], lib.E_UNSUPPORTED, says="word size differs")
    # `.ctr`: a table made non-monotone, and xtree-compress's first-bin quirk with a single node under the first prefix
    pref = ctrfile.word_prefix(W, np.zeros(300, dtype=np.uint64), np.array([w for w, _ in db.nodes], dtype=np.uint64))
    bins = ctrfile.binix_exact(pref, 300)
    nz = np.flatnonzero(np.diff(bins.astype(np.int64)) > 0)
    bins[nz[10] + 1] = bins[nz[10]]
    bins[nz[10]] += np.uint64(1)
    p = str(tmp_path / "nonmono.ctr")
    as_ctr(db, p, binix=bins)
    fails(tmp_path, [good, p], lib.E_UNSUPPORTED, says="cannot be reconstructed")
    q = Db(W, I, [((3 << 40) | 0xF0F0F0F0F0, b"k__A;p__B")] + [((0x2345 << 40) | (v << 8), b"k__A;p__B") for v in range(1, 30)])
    p = str(tmp_path / "quirk.ctr")
    as_ctr(q, p, like_compress=True)                                                        # node 0 is then addressable only under prefix 0x2345
    fails(tmp_path, [p], lib.E_UNSUPPORTED, says="first-bin quirk")
    fails(tmp_path, [util.fixture_ctr("toy")], lib.E_UNSUPPORTED, says="first-bin quirk")   # the genuine xtree-compress wrote this one
    out = str(tmp_path / "quirk.ubt")
    p2 = str(tmp_path / "no_quirk.ctr")
    as_ctr(q, p2)
    search.merge([p2], out)
    assert open(out, "rb").read() == M.merge([q])[0]


# ---- the chain: build shards, merge, compress, search ---------------------------------------------------------------------------------------
def test_shards_built_merged_compressed_and_searched(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    r = M.rng(13)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    root = r.integers(0, 4, 3000, dtype=np.uint8)
    refs = []
    for i in range(24):                                                                     # related references: mutated stretches of one root
        s = root[int(r.integers(0, 1000)):][:int(r.integers(600, 2000))].copy()
        m = r.random(len(s)) < 0.02
        s[m] = r.integers(0, 4, int(m.sum()), dtype=np.uint8)
        refs.append((b"ref%d" % i, b"k__A;p__B;c__C%d;o__D%d;f__F%d" % (i % 2, i % 4, i), acgt[s].tobytes()))
    shards = []
    for k, part in enumerate((refs[:12], refs[12:])):
        fa, mp, ubt = (str(tmp_path / ("s%d.%s" % (k, e))) for e in ("fa", "map", "ubt"))
        open(fa, "wb").write(b"".join(b">" + n + b"\n" + s + b"\n" for n, _, s in part))
        open(mp, "wb").write(b"".join(n + b"\t" + l + b"\n" for n, l, _ in part))
        p = subprocess.run([lib.BUILD_GG_CLI_PATH, fa, mp, ubt, "1", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stdout[-300:]
        shards.append(ubt)
    merged, ctr = str(tmp_path / "merged.ubt"), str(tmp_path / "merged.ctr")
    st = search.merge(shards, merged)
    assert st.n_shared > 100 and st.n_relabelled > 0
    assert open(merged, "rb").read() == M.merge([M.read_ubt(p) for p in shards])[0]
    p = subprocess.run([lib.COMPRESS_CLI_PATH, merged, ctr], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stdout[-300:]
    reads = []
    for i in range(3000):
        _, _, s = refs[int(r.integers(0, len(refs)))]
        a = int(r.integers(0, len(s) - 120))
        reads.append(b">q%d\n" % i + s[a:a + int(r.integers(40, 120))] + b"\n")
    rd = str(tmp_path / "reads.fa")
    open(rd, "wb").write(b"".join(reads))
    ours = str(tmp_path / "ours.txt")
    p = subprocess.run([lib.CLI_PATH, ctr, rd, ours, "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stdout[-300:] + p.stderr[-300:]
    got = open(ours, "rb").read()
    assert got.count(b"\n") > 1000
    o = orc.OracleDB.load(ctr)                                                              # the merged file is a database the reference reads
    code, _, _, err = o.search_file(rd, str(tmp_path / "orc.txt"), threads=1)
    assert code == 0, err
    assert got == open(str(tmp_path / "orc.txt"), "rb").read()
    exe = os.path.join(REF, "xtree-searchGG")
    if os.path.exists(exe):
        p = subprocess.run([exe, ctr, rd, str(tmp_path / "ref.txt"), "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stdout[-300:]
        assert got == open(str(tmp_path / "ref.txt"), "rb").read()


# ---- the command lines ----------------------------------------------------------------------------------------------------------------------
def test_command_lines(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    monkeypatch.delenv("UTREE_IXTYPE", raising=False)
    inputs, _ = M.fold_cases()["two_way_cut"]
    paths = write_inputs(tmp_path, inputs)
    c = str(tmp_path / "in1.ctr")
    as_ctr(inputs[1], c)
    paths[1] = c
    for exe, gg in ((lib.MERGE_GG_CLI_PATH, True), (lib.MERGE_CLI_PATH, False)):
        out = str(tmp_path / "cli.ubt")
        p = subprocess.run([exe, out] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr
        want, ws = M.merge(inputs, gg)
        assert open(out, "rb").read() == want
        lines = p.stdout.decode().splitlines()
        assert lines[0].startswith("This is UTree")
        n_labels = [len(set(l for _, l in db.nodes)) for db in inputs]
        assert lines[1] == "%s: .ubt, %d nodes [%d labels]" % (paths[0], len(inputs[0].nodes), n_labels[0])
        assert lines[2] == "%s: .ctr, %d nodes [%d labels]" % (paths[1], len(inputs[1].nodes), n_labels[1])
        assert lines[3:] == ["Total nodes in tree: %d [%d labels]" % (ws["n_nodes"], ws["n_labels"]), "Tree written."]
        err = p.stderr.decode()
        assert "[utree_amd] merge" in err and "%d shared, %d relabelled, %d dropped" % (ws["n_shared"], ws["n_relabelled"], ws["n_dropped"]) in err
    out = str(tmp_path / "wide.ubt")
    p = subprocess.run([lib.MERGE_GG_CLI_PATH, out] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, UTREE_IXTYPE="32"))
    assert p.returncode == 0 and open(out, "rb").read() == M.merge(inputs, True, 4)[0]
    out = str(tmp_path / "none.ubt")
    p = subprocess.run([lib.MERGE_GG_CLI_PATH, out, paths[0], str(tmp_path / "missing.ubt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and not os.path.exists(out)
    bad = str(tmp_path / "bad.ubt")
    open(bad, "wb").write(open(paths[0], "rb").read()[:-2])
    p = subprocess.run([lib.MERGE_GG_CLI_PATH, out, paths[0], bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 2 and not os.path.exists(out) and b"ERROR" in p.stderr
    p = subprocess.run([lib.MERGE_GG_CLI_PATH, str(tmp_path / "no_such_dir" / "o.ubt"), paths[0]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1
    p = subprocess.run([lib.MERGE_GG_CLI_PATH, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"usage: utree-mergeGG output.ubt input1 [input2" in p.stdout
