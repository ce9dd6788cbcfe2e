"""utree_merge_files_edit on the GPU (merge_kernels.hip): every output file is compared byte for byte with tests/merge_edit_ref.py -- the
definition in plain Python that test_merge_edit_cpu.py pins to the genuine builder -- and both stats structs with its figures."""
import os
import subprocess

import numpy as np
import pytest

import build_inputs as B
import merge_edit_ref as E
import merge_ref as M
import util
from oracle import orc
from utree_amd import ctrfile, lib, search

pytestmark = pytest.mark.gpu
Db = M.Db
LA, LB, LC, LD = (getattr(B, n).encode() for n in ("LA", "LB", "LC", "LD"))


def write_inputs(tmp_path, inputs, tag="in"):
    paths = []
    for i, db in enumerate(inputs):
        p = str(tmp_path / ("%s%d.ubt" % (tag, i)))
        open(p, "wb").write(M.db_file(db))
        paths.append(p)
    return paths


def as_ctr(db, path):
    labs = E.label_lines_of(db)
    ix = np.array([labs.index(l) for _, l in db.nodes], dtype=np.uint32)
    hi = np.array([w >> 64 for w, _ in db.nodes], dtype=np.uint64)
    lo = np.array([w & 0xFFFFFFFFFFFFFFFF for w, _ in db.nodes], dtype=np.uint64)
    ctrfile.write_ctr(path, db.W, db.I, hi, lo, ix, [l.decode("latin-1") for l in labs])
    return path


def rule_paths(tmp_path, r, tag):
    out = {}
    for which in ("drop", "keep", "rename"):
        lines = getattr(r, which)
        if lines is not None:
            out[which] = str(tmp_path / ("%s_%s.rules" % (tag, which)))
            open(out[which], "wb").write(E.rule_file(lines))
    return out


def check(tmp_path, monkeypatch, inputs, r=E.rules(), minus=(), gg=True, I=0, pass_nodes=None, paths=None, minus_paths=None, tag="in"):
    """merge with the edit on the device; the file and both sets of figures must be merge_edit_ref's.  Returns (stats, edit stats)."""
    if pass_nodes:
        monkeypatch.setenv("UTREE_TEST_MERGE_PASS_NODES", str(pass_nodes))
    else:
        monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    paths = paths or write_inputs(tmp_path, inputs, tag)
    minus_paths = minus_paths if minus_paths is not None else write_inputs(tmp_path, minus, tag + "_minus")
    out = str(tmp_path / (tag + "_out.ubt"))
    st, es = search.merge_edit(paths, out, gg=gg, I=I, ranks=r.ranks, minus=minus_paths, **rule_paths(tmp_path, r, tag))
    want, ws, wes = E.merge(inputs, r, minus, gg, I)
    got = open(out, "rb").read()
    assert got == want
    assert {k: getattr(st, k) for k in ws} == ws
    assert {k: getattr(es, k) for k in wes} == wes
    fed = st.n_in_nodes - es.n_nodes_dropped - es.n_nodes_subtracted
    assert fed == sum(len(d.nodes) for d in E.edited(inputs, r, minus))
    tail = got[32 + st.n_nodes * (st.W + st.I):]
    assert sum(int(l.split(b"\t")[1]) for l in tail.split(b"\n")[:-1]) == st.n_nodes          # the label tail's counts sum to n_nodes
    assert (st.W, st.I, st.n_inputs) == (inputs[0].W, I or max(d.I for d in inputs), len(inputs))
    return st, es


def fails(tmp_path, paths, code, says=None, **kw):
    out = str(tmp_path / "refused.ubt")
    with pytest.raises(lib.UtreeError) as e:
        search.merge_edit(paths, out, **kw)
    assert e.value.code == code, e.value
    assert says is None or says in e.value.detail, e.value.detail
    assert not os.path.exists(out), "a failed call leaves no output file behind"


def seven(words, stem=b"k__A;p__B;c__L"):
    """node j under label number j % 7"""
    return [(w, stem + b"%d" % (j % 7)) for j, w in enumerate(words)]


DROP_THIRDS = E.rules(drop=[b"k__A;p__B;c__L0", b"k__A;p__B;c__L3", b"k__A;p__B;c__L6"])


# ---- input sizes: the wavefront and block edges of decode, select and pack ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_sizes(n, tmp_path, monkeypatch):
    """every third label dropped, every fifth word in a MINUS input; a second input shares every word under a deeper label"""
    W, I = 8, 2
    words = M.random_words(M.rng(101, n), W, n + 5)
    a = Db(W, I, seven(words[:n]))
    b = Db(W, I, [(w, l + b";o__x") for w, l in a.nodes])
    minus = Db(W, I, sorted([(w, b"k__Host") for w in words[:n:5]] + [(w, b"k__Host;p__Other") for w in words[n:]]))
    st, es = check(tmp_path, monkeypatch, [a], DROP_THIRDS, [minus], tag="one")
    assert es.n_minus_nodes == len(minus.nodes) and es.n_nodes_dropped + es.n_nodes_subtracted + st.n_nodes == n
    st, es = check(tmp_path, monkeypatch, [a, b], DROP_THIRDS, [minus], tag="two")
    assert st.n_shared == st.n_nodes == st.n_relabelled and es.n_nodes_subtracted == 2 * sum(j % 7 not in (0, 3, 6) for j in range(0, n, 5))


# ---- where a dropped and a subtracted record stand --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pass_nodes", [None, 64, 100])
def test_positions(pass_nodes, tmp_path, monkeypatch):
    """the first and the last record of a slice, records 255 and 256 (the last of a block, the first of the next): label-dropped, then
    subtracted; then every fourth record of each kind, so that with the pass hook slices begin and end on them"""
    W, I = 8, 2
    n = 600
    words = M.random_words(M.rng(102), W, n)
    edge = (0, 255, 256, n - 1)
    gone = E.rules(drop=[b"k__Gone"])
    a = Db(W, I, [(w, b"k__Gone;p__X" if j in edge else b"k__A;p__B;c__%d" % (j % 3)) for j, w in enumerate(words)])
    other = Db(W, I, [(words[j], LA) for j in (0, 1, 255, 256, 300, n - 1)])
    st, es = check(tmp_path, monkeypatch, [a, other], gone, pass_nodes=pass_nodes, tag="d")
    assert es.n_nodes_dropped == 4 and st.n_shared == 2
    plain = Db(W, I, [(w, b"k__A;p__B;c__%d" % (j % 3)) for j, w in enumerate(words)])
    minus = Db(W, I, [(words[j], b"k__Host") for j in edge])
    st, es = check(tmp_path, monkeypatch, [plain, other], E.rules(), [minus], pass_nodes=pass_nodes, tag="s")
    assert es.n_nodes_subtracted == 8 and st.n_shared == 2
    mixed = Db(W, I, [(w, b"k__Gone;p__X" if j % 4 == 0 else b"k__A;p__B;c__%d" % (j % 3)) for j, w in enumerate(words)])
    minus = Db(W, I, [(w, b"k__Host") for w in words[2::4]] + [(words[-1] + 1, b"k__Host")])
    st, es = check(tmp_path, monkeypatch, [mixed], gone, [minus], pass_nodes=pass_nodes, tag="m")
    assert es.n_nodes_dropped == 150 == es.n_nodes_subtracted and st.n_nodes == 300
    if pass_nodes:
        assert st.n_passes > 4                                              # MINUS nodes count towards a pass; a word and the MINUS record that cancels it share their prefix, so they meet


@pytest.mark.parametrize("pass_nodes", [64, 100])
def test_minus_meets_its_word_across_the_pass_hook(pass_nodes, tmp_path, monkeypatch):
    """the MINUS input alone is larger than a pass: its slices are cut by the same prefix ranges as the regular input's"""
    W, I = 8, 2
    words = M.random_words(M.rng(103), W, 900)
    a = Db(W, I, seven(words[::3]))
    minus = Db(W, 4, [(w, b"k__Host") for j, w in enumerate(words) if j % 3 or j % 2 == 0])    # every word a lacks and half of those it has
    st, es = check(tmp_path, monkeypatch, [a], E.rules(), [minus], pass_nodes=pass_nodes)
    assert es.n_nodes_subtracted == 150 and st.n_nodes == 150 and st.n_passes > 8
    st, es = check(tmp_path, monkeypatch, [a], E.rules(), [minus], pass_nodes=pass_nodes, paths=[as_ctr(a, str(tmp_path / "a.ctr"))],
                   minus_paths=[as_ctr(minus, str(tmp_path / "m.ctr"))], tag="ctr")
    assert st.n_passes > 8


# ---- the cases of merge_edit_ref, widths and layouts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.edit_cases()))
def test_edit_cases(name, tmp_path, monkeypatch):
    """label numbering among them: the first-carrier order after drops and subtraction (first_carrier_dropped, minus), a label all of
    whose nodes vanish has no line (one_side_dropped, everything_dropped), a prefix label made by a fold of two edited texts gets its
    index at the cut's event (cut_makes_fold)"""
    inputs, r, minus, gg = E.edit_cases()[name]
    st, es = check(tmp_path, monkeypatch, inputs, r, minus, gg)
    check(tmp_path, monkeypatch, inputs, r, minus, gg, pass_nodes=64, tag="p")
    if name == "everything_dropped":
        assert st.n_nodes == 0 and st.n_labels == 0 and os.path.getsize(str(tmp_path / "in_out.ubt")) == 32


@pytest.mark.parametrize("W,I", [(4, 2), (4, 4), (8, 4), (16, 2), (16, 4)])
@pytest.mark.parametrize("name", ["cut_makes_fold", "first_carrier_dropped", "minus"])
def test_other_widths(W, I, name, tmp_path, monkeypatch):
    inputs, r, minus, gg = E.edit_cases(W, I)[name]
    check(tmp_path, monkeypatch, inputs, r, minus, gg)
    check(tmp_path, monkeypatch, inputs, r, minus, gg, pass_nodes=64, tag="p")
    cp = [as_ctr(db, str(tmp_path / ("c%d.ctr" % i))) for i, db in enumerate(inputs)]
    mp = [as_ctr(db, str(tmp_path / ("m%d.ctr" % i))) for i, db in enumerate(minus)]
    check(tmp_path, monkeypatch, inputs, r, minus, gg, paths=cp, minus_paths=mp, tag="ctr")
    check(tmp_path, monkeypatch, inputs, r, minus, gg, pass_nodes=64, paths=[cp[0]] + write_inputs(tmp_path, inputs[1:], "u"), minus_paths=mp, tag="mix")


def test_mixed_index_widths(tmp_path, monkeypatch):
    inputs, r, minus, gg = E.edit_cases(8, 2)["minus"]
    mixed = [Db(8, 4, inputs[0].nodes), inputs[1]]
    st, _ = check(tmp_path, monkeypatch, mixed, E.rules(ranks=3), minus)
    assert st.I == 4
    st, _ = check(tmp_path, monkeypatch, mixed, E.rules(ranks=3), minus, I=2, tag="narrow")
    assert st.I == 2


def fixture_ubt(name, tmp_path):
    """a fixture database as a `.ubt`, from the first prefix on that holds two nodes (xtree-compress's first-bin quirk, see test_gpu_merge.py)"""
    nodes = M.read_ctr(util.fixture_ctr(name)).nodes
    d = util.load_db_fixture(name)
    shift = {4: 8, 8: 40, 16: 104}[d.W]
    s = 0
    while nodes[s + 1][0] <= nodes[s][0] or (nodes[s + 1][0] >> shift) != (nodes[s][0] >> shift):
        s += 1
    p = str(tmp_path / (name + ".ubt"))
    open(p, "wb").write(M.db_file(Db(d.W, d.I, nodes[s:])))
    return p


@pytest.mark.parametrize("name", ["k64", "k16"])
def test_fixture_databases(name, tmp_path, monkeypatch):
    """a genuine database as `.ubt` and as the `.ctr` xtree-compress makes of it, cut to two ranks, a seventh of its nodes in a MINUS `.ctr`"""
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    ubt = fixture_ubt(name, tmp_path)
    ctr = str(tmp_path / (name + ".ctr"))
    code, _ = search.compress(ubt, ctr)
    assert code == lib.OK
    db = M.read_ubt(ubt)
    minus = Db(db.W, db.I, [(w, b"k__Host") for w, _ in db.nodes[:2] + db.nodes[3::7]])   # two nodes under its first prefix: no first-bin quirk
    mu = write_inputs(tmp_path, [minus], "minus")[0]
    mc = str(tmp_path / "minus.ctr")
    code, _ = search.compress(mu, mc)
    assert code == lib.OK
    r = E.rules(ranks=2)
    st, es = check(tmp_path, monkeypatch, [db], r, [minus], paths=[ubt], minus_paths=[mc], tag="u")
    assert es.n_nodes_subtracted == len(minus.nodes) and es.n_labels_cut > 0
    check(tmp_path, monkeypatch, [db], r, [minus], paths=[ctr], minus_paths=[mu], pass_nodes=1000, tag="c")


# ---- k = 64: the two halves are sorted one after the other ----------------------------------------------------------------------------------------
def test_k64_halves(tmp_path, monkeypatch):
    r = M.rng(104)
    H = [int.from_bytes(r.bytes(8), "little") for _ in range(9)]
    Lo = [int.from_bytes(r.bytes(8), "little") for _ in range(9)]
    words = sorted((h << 64) | l for h in H[:8] for l in Lo[:8])
    a = Db(16, 2, seven(words))
    hi_only = Db(16, 2, sorted(((h << 64) | Lo[8], b"k__Host") for h in H[:8]))               # equal to kept words in `hi` only
    lo_only = Db(16, 2, sorted(((H[8] << 64) | l, b"k__Host") for l in Lo[:8]))               # in `lo` only
    st, es = check(tmp_path, monkeypatch, [a], E.rules(), [hi_only, lo_only])
    assert es.n_nodes_subtracted == 0 and st.n_nodes == 64 and es.n_minus_nodes == 16
    both = Db(16, 2, sorted(hi_only.nodes + [(words[0], b"k__Host"), (words[37], b"k__Host"), (words[63], b"k__Host")]))
    st, es = check(tmp_path, monkeypatch, [a, a], E.rules(), [both, lo_only], paths=write_inputs(tmp_path, [a]) * 2, tag="both")
    assert es.n_nodes_subtracted == 6 and st.n_nodes == 61 == st.n_shared


# ---- runs ---------------------------------------------------------------------------------------------------------------------------------------
def test_runs(tmp_path, monkeypatch):
    W, I = 8, 2
    words = M.random_words(M.rng(105), W, 40)
    fill = lambda i: [(w, b"k__Own;p__I%d" % i) for w in words[10 + 10 * i:20 + 10 * i]]
    # words[0]: one side dropped; [1]: both sides dropped; [2]: in two MINUS inputs and in all regular inputs; [3]: in one MINUS input and
    # one regular input, under a dropped label (it counts as dropped); [4]: three records, the middle one dropped: the outer two fold
    a = Db(W, I, sorted([(words[0], LA), (words[1], LD), (words[2], LA), (words[3], LD), (words[4], LA)] + fill(0)))
    b = Db(W, I, sorted([(words[0], LD), (words[1], LD + b";c__x"), (words[2], LB), (words[4], LD)] + fill(1)))
    c = Db(W, I, sorted([(words[2], LC), (words[4], LB)] + fill(2)))
    m1 = Db(W, I, sorted([(words[2], b"k__Host"), (words[3], b"k__Host"), (words[5], b"k__Host")]))
    m2 = Db(W, 4, sorted([(words[2], b"k__Host2"), (words[6], b"k__Host2"), (words[10], b"k__Host2")]))
    r = E.rules(drop=[b"k__Z"])
    st, es = check(tmp_path, monkeypatch, [a, b, c], r, [m1, m2])
    assert (es.n_nodes_dropped, es.n_nodes_subtracted, st.n_shared, st.n_relabelled, st.n_dropped) == (5, 4, 1, 1, 0)
    out = M.read_ubt(str(tmp_path / "in_out.ubt"))
    have = dict(out.nodes)
    assert have[words[0]] == LA and have[words[4]] == b"k__A;p__B;c__C"
    assert not set(have) & {words[1], words[2], words[3], words[5], words[6], words[10]}     # words only a MINUS input holds never appear
    # the same MINUS file given twice changes nothing
    mp = write_inputs(tmp_path, [m1, m2], "mm")
    st2, es2 = check(tmp_path, monkeypatch, [a, b, c], r, [m1, m2, m1], minus_paths=mp + [mp[0]], tag="twice")
    assert es2.n_nodes_subtracted == 4 and es2.n_minus_nodes == 9
    assert open(str(tmp_path / "twice_out.ubt"), "rb").read() == open(str(tmp_path / "in_out.ubt"), "rb").read()


# ---- the 2-byte limit applies to the labels after the edit --------------------------------------------------------------------------------------
def test_a_rank_cut_brings_the_labels_under_the_two_byte_limit(tmp_path, monkeypatch):
    W = 8
    words = M.random_words(M.rng(106), W, 65535)
    a = Db(W, 4, [(w, b"k__A;p__B;c__C;o__D;f__E;g__F;s__%d;t__%d" % (j % 300, j)) for j, w in enumerate(words)])
    paths = write_inputs(tmp_path, [a])
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    out = str(tmp_path / "refused.ubt")
    with pytest.raises(lib.UtreeError) as e:
        search.merge(paths, out, I=2)
    assert e.value.code == lib.E_UNSUPPORTED and not os.path.exists(out)
    fails(tmp_path, paths, lib.E_UNSUPPORTED, says="4-byte index", I=2)                       # an edit that changes nothing: still refused
    st, es = check(tmp_path, monkeypatch, [a], E.rules(ranks=7), I=2, paths=paths)
    assert st.I == 2 and st.n_labels == 300 and es.n_labels_cut == 65535 and st.n_nodes == 65535


# ---- an edit that edits nothing is the merge ------------------------------------------------------------------------------------------------------
def test_identity(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    nothing = E.rules(drop=[b"k__Nope", b"k__A;p__"], rename=[(b"k__A;p", b"k__Q")])
    rp = rule_paths(tmp_path, nothing, "nothing")
    minus = write_inputs(tmp_path, [Db(8, 2, [])], "empty_minus")
    fields = [f for f, _ in lib.MergeStats._fields_ if f != "seconds"]
    for name, (inputs, gg) in sorted(M.fold_cases().items()):
        paths = write_inputs(tmp_path, inputs, name)
        outs = [str(tmp_path / ("%s_%d.ubt" % (name, k))) for k in range(4)]
        st0 = search.merge(paths, outs[0], gg=gg)
        st1, es1 = search.merge_edit(paths, outs[1], gg=gg)
        st2, es2 = search.merge_edit(paths, outs[2], gg=gg, **rp)
        st3, es3 = search.merge_edit(paths, outs[3], gg=gg, minus=minus)                      # labels dated by the fold, not the decode
        want = open(outs[0], "rb").read()
        assert want == M.merge(inputs, gg)[0]
        for o, st in zip(outs[1:], (st1, st2, st3)):
            assert open(o, "rb").read() == want, name
            assert [getattr(st, f) for f in fields] == [getattr(st0, f) for f in fields], name
        lines = sum(len(E.label_lines_of(db)) for db in inputs)
        assert (es1.n_label_lines, es1.n_rules_unmatched, es2.n_rules_unmatched, es3.n_minus_nodes) == (lines, 0, 3, 0)
        assert es2.n_labels_dropped == es2.n_labels_renamed == es2.n_labels_cut == es2.n_nodes_dropped == es2.n_nodes_subtracted == 0


# ---- refusals leave no file -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_no_file(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    W, I = 8, 2
    words = M.random_words(M.rng(107), W, 300)
    db = Db(W, I, seven(words) + [(words[-1] + 1, b";x")])
    good = write_inputs(tmp_path, [db])[0]
    m = Db(W, I, [(w, b"k__Host") for w in words[::3]])
    raw = M.db_file(m)
    rec = W + I
    a, b = 32 + 50 * rec, 32 + 51 * rec
    swapped = str(tmp_path / "swapped.ubt")
    open(swapped, "wb").write(raw[:a] + raw[b:b + rec] + raw[a:b] + raw[b + rec:])
    fails(tmp_path, [good], lib.E_FORMAT, says="not strictly ascending", minus=[swapped])
    other_w = write_inputs(tmp_path, [Db(16, I, [(5, b"k__Host")])], "w16")[0]
    fails(tmp_path, [good], lib.E_UNSUPPORTED, says=other_w + ": its word size differs", minus=[other_w])
    fails(tmp_path, [good], lib.E_IO, minus=[str(tmp_path / "missing.ubt")])
    cut = str(tmp_path / "cut.ubt")
    open(cut, "wb").write(raw[:-3])
    fails(tmp_path, [good], lib.E_FORMAT, minus=[cut])
    fails(tmp_path, [good], lib.E_IO, says="missing.rules", drop=str(tmp_path / "missing.rules"))
    bad = str(tmp_path / "bad.rules")
    open(bad, "wb").write(b"a\tb\nno tab\n")
    fails(tmp_path, [good], lib.E_FORMAT, says="line 2", rename=bad)
    fails(tmp_path, [good], lib.E_FORMAT, says="`;x`", ranks=1)                               # an empty edited label
    # a MINUS input's label indices are not looked at: indices that name no line are fine there, and refused in a regular input
    beyond = bytearray(raw)
    beyond[32 + 7 * rec + W] = 9
    bp = str(tmp_path / "beyond.ubt")
    open(bp, "wb").write(bytes(beyond))
    fails(tmp_path, [good, bp], lib.E_FORMAT, says="names no label line")
    check(tmp_path, monkeypatch, [Db(W, I, db.nodes[:-1])], E.rules(), [m], minus_paths=[bp], tag="ok")
    # ... and neither is a regular record's whose label line is dropped mistaken for one
    st, es = check(tmp_path, monkeypatch, [db], E.rules(drop=[b";x", b"k__A;p__B;c__L1"]), tag="dropped")
    assert es.n_nodes_dropped == 44


# ---- the command lines --------------------------------------------------------------------------------------------------------------------------
def test_command_lines(tmp_path, monkeypatch):
    for v in ("UTREE_TEST_MERGE_PASS_NODES", "UTREE_IXTYPE", "UTREE_MERGE_RANKS", "UTREE_MERGE_DROP", "UTREE_MERGE_KEEP", "UTREE_MERGE_RENAME",
              "UTREE_MERGE_MINUS", "UTREE_MERGE_PREVIEW"):
        monkeypatch.delenv(v, raising=False)
    inputs, _, minus, _ = E.edit_cases()["minus"]
    inputs = [inputs[0], Db(8, 2, inputs[1].nodes + [(max(w for w, _ in inputs[1].nodes) + 1, LD)])]
    minus = list(minus) + [Db(8, 2, [(w + 2 * (j > 0), b"k__Host2") for j, (w, _) in enumerate(inputs[0].nodes[3:15])])]   # one word of input 0
    paths = write_inputs(tmp_path, inputs)
    mp = [write_inputs(tmp_path, minus[:1], "minus")[0], as_ctr(minus[1], str(tmp_path / "minus1.ctr"))]
    each = {"UTREE_MERGE_RANKS": (E.rules(ranks=3), "3"), "UTREE_MERGE_DROP": (E.rules(drop=[b"k__Z", b"k__Typo"]), "drop"),
            "UTREE_MERGE_KEEP": (E.rules(keep=[b"k__A"]), "keep"), "UTREE_MERGE_RENAME": (E.rules(rename=[(b"k__A;p__B", b"k__A;p__Q")]), "rename"),
            "UTREE_MERGE_MINUS": (E.rules(), ":".join(mp))}
    everything = E.rules(3, [b"k__Z", b"k__Typo"], [b"k__A"], [(b"k__A;p__B", b"k__A;p__Q")])
    rp = rule_paths(tmp_path, everything, "cli")
    env_of = lambda var, val: {var: rp[val] if val in rp else val}
    runs = [(env_of(var, val), r, minus if var == "UTREE_MERGE_MINUS" else ()) for var, (r, val) in each.items()]
    all_env = {}
    for var, (_, val) in each.items():
        all_env.update(env_of(var, val))
    runs.append((all_env, everything, minus))
    for exe, gg in ((lib.MERGE_GG_CLI_PATH, True), (lib.MERGE_CLI_PATH, False)):
        for env, r, mi in runs:
            out = str(tmp_path / "cli.ubt")
            p = subprocess.run([exe, out] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env))
            assert p.returncode == 0, p.stderr
            want, ws, wes = E.merge(inputs, r, mi, gg)
            assert open(out, "rb").read() == want, env
            lines = p.stdout.decode().splitlines()
            assert len(lines) == 1 + 2 + len(mi) + 2 and lines[-2:] == ["Total nodes in tree: %d [%d labels]" % (ws["n_nodes"], ws["n_labels"]), "Tree written."]
            if mi:
                assert lines[3] == "%s: .ubt, %d nodes [1 labels]" % (mp[0], len(mi[0].nodes)) and lines[4] == "%s: .ctr, 12 nodes [1 labels]" % mp[1]
            err = p.stderr.decode()
            assert "[utree_amd] merge" in err and "%d nodes in, %d shared" % (ws["n_in_nodes"], ws["n_shared"]) in err
            assert ("[utree_amd] edit: %d label lines, %d dropped, %d renamed, %d cut, %d rules unmatched, %d nodes dropped, %d minus nodes, %d nodes subtracted"
                    % tuple(wes[k] for k in ("n_label_lines", "n_labels_dropped", "n_labels_renamed", "n_labels_cut", "n_rules_unmatched",
                                             "n_nodes_dropped", "n_minus_nodes", "n_nodes_subtracted"))) in err
            os.unlink(out)
        # the preview: no output.ubt, exit code 0, and the MINUS inputs are not even opened
        tsv = str(tmp_path / "cli.tsv")
        env = dict(os.environ, UTREE_MERGE_PREVIEW=tsv, UTREE_MERGE_MINUS=str(tmp_path / "no_such.ctr"), **{k: v for k, v in all_env.items() if k != "UTREE_MERGE_MINUS"})
        p = subprocess.run([exe, out] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert p.returncode == 0 and not os.path.exists(out) and b"Tree written" not in p.stdout, p.stderr
        files = [(pa, ".ubt", len(db.nodes), [(t, sum(l == t for _, l in db.nodes)) for t in E.label_lines_of(db)]) for pa, db in zip(paths, inputs)]
        assert open(tsv, "rb").read() == E.preview(files, everything, rp)[0]
        os.unlink(tsv)
        # without any of the variables: the plain merge, and no edit line
        p = subprocess.run([exe, out] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and open(out, "rb").read() == M.merge(inputs, gg)[0] and b"[utree_amd] edit" not in p.stderr
        os.unlink(out)
    for exe in (lib.MERGE_GG_CLI_PATH,):                                                        # the exit codes: the two binaries share the program
        for env, code in (({"UTREE_MERGE_RANKS": "three"}, 2), ({"UTREE_MERGE_RANKS": "256"}, 2), ({"UTREE_MERGE_RANKS": "3x"}, 2),
                          ({"UTREE_MERGE_DROP": str(tmp_path / "missing.rules")}, 1), ({"UTREE_MERGE_MINUS": str(tmp_path / "missing.ubt")}, 1),
                          ({"UTREE_MERGE_RENAME": rp["drop"]}, 2), ({"UTREE_MERGE_RANKS": "1", "UTREE_MERGE_RENAME": rp["rename"], "UTREE_MERGE_KEEP": rp["keep"]}, 0)):
            p = subprocess.run([exe, out] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env))
            assert p.returncode == code, (env, p.stderr)
            assert os.path.exists(out) == (code == 0) and (code == 0 or b"ERROR" in p.stderr)
            if code == 0:
                os.unlink(out)


# ---- the chain: build shards, merge with a MINUS database and a rank cut, compress, search ------------------------------------------------------
def test_shards_decontaminated_cut_compressed_and_searched(tmp_path, monkeypatch):
    monkeypatch.delenv("UTREE_TEST_MERGE_PASS_NODES", raising=False)
    r = M.rng(108)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    root = r.integers(0, 4, 3000, dtype=np.uint8)
    host = acgt[r.integers(0, 4, 500, dtype=np.uint8)].tobytes()                            # the planted "host" sequence
    refs = []
    for i in range(16):                                                                     # related references: mutated stretches of one root
        s = root[int(r.integers(0, 1000)):][:int(r.integers(600, 2000))].copy()
        m = r.random(len(s)) < 0.02
        s[m] = r.integers(0, 4, int(m.sum()), dtype=np.uint8)
        seq = acgt[s].tobytes()
        if i in (3, 11):
            seq = seq[:300] + host + seq[300:]                                              # two assemblies carry it, one in each shard
        refs.append((b"ref%d" % i, b"k__A;p__B;c__C%d;o__D%d;f__F%d;g__G%d" % (i % 2, i % 4, i % 8, i), seq))

    def build(tag, part):
        fa, mp, ubt = (str(tmp_path / ("%s.%s" % (tag, e))) for e in ("fa", "map", "ubt"))
        open(fa, "wb").write(b"".join(b">" + n + b"\n" + s + b"\n" for n, _, s in part))
        open(mp, "wb").write(b"".join(n + b"\t" + l + b"\n" for n, l, _ in part))
        p = subprocess.run([lib.BUILD_GG_CLI_PATH, fa, mp, ubt, "1", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stdout[-300:]
        return ubt
    shards = [build("s0", refs[:8]), build("s1", refs[8:])]
    hostdb = build("host", [(b"host", b"k__Host;p__Sapiens", host)])
    merged, ctr = str(tmp_path / "merged.ubt"), str(tmp_path / "merged.ctr")
    st, es = search.merge_edit(shards, merged, ranks=5, minus=[hostdb])
    lines = [M.parse_labels(ctrfile.read_ubt(p)[5]) for p in shards]                        # a built shard also has lines no node carries any more
    want, ws, wes = E.merge([M.read_ubt(p) for p in shards], E.rules(ranks=5), [M.read_ubt(hostdb)], label_lines=lines)
    assert open(merged, "rb").read() == want
    assert {k: getattr(st, k) for k in ws} == ws and {k: getattr(es, k) for k in wes} == wes
    assert es.n_nodes_subtracted >= 2 * (500 - 31) and st.n_shared > 100 and es.n_labels_cut >= 16
    p = subprocess.run([lib.COMPRESS_CLI_PATH, merged, ctr], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stdout[-300:]
    reads, n_host = [], 0
    for i in range(2000):
        if i % 10 == 0:
            a = int(r.integers(0, len(host) - 120))
            reads.append(b">h%d\n" % i + host[a:a + int(r.integers(40, 120))] + b"\n")
            n_host += 1
            continue
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
    assert not any(l.startswith(b"h") for l in got.split(b"\n")), "reads drawn from the planted host sequence print no line"
    o = orc.OracleDB.load(ctr)
    code, _, _, err = o.search_file(rd, str(tmp_path / "orc.txt"), threads=1)
    assert code == 0, err
    assert got == open(str(tmp_path / "orc.txt"), "rb").read()
    # without the MINUS database those reads are classified
    plain, pctr = str(tmp_path / "plain.ubt"), str(tmp_path / "plain.ctr")
    search.merge_edit(shards, plain, ranks=5)
    assert subprocess.run([lib.COMPRESS_CLI_PATH, plain, pctr], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 0
    p = subprocess.run([lib.CLI_PATH, pctr, rd, ours, "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0
    assert sum(l.startswith(b"h") for l in open(ours, "rb").read().split(b"\n")) > n_host // 2
