"""Where the buffers of the database tools turn over (merge_kernels.hip): decode_sort's two staging buffers, which the merge, the edit, the
compare and the inspect share, and utk_merge_emit's two output chunks.  UTREE_TEST_MERGE_STAGE_BYTES and UTREE_TEST_MERGE_OUT_NODES lower the
two sizes, so inputs of some hundred nodes go through many chunks: records cut in two by a chunk's end, a buffer used a second time, counts
that add up over the chunks.  Every result is compared byte for byte and integer for integer with the plain-Python definitions
(merge_ref, merge_edit_ref, compare_ref, inspect_ref) and with the same call without the hooks.  Last, one compare and one inspect whose
label ids pass 2^16."""
import os

import numpy as np
import pytest

import build_inputs as B
import compare_ref as CR
import inspect_ref as IR
import merge_edit_ref as E
import merge_ref as M
from utree_amd import ctrfile, search

pytestmark = pytest.mark.gpu
Db = M.Db
HOOKS = {"stage": "UTREE_TEST_MERGE_STAGE_BYTES", "out": "UTREE_TEST_MERGE_OUT_NODES", "pass_nodes": "UTREE_TEST_MERGE_PASS_NODES"}
LABS = [s for s in M.SIBLINGS] + [getattr(B, n).encode() for n in ("LA", "LB", "LX", "LC", "LD")]


def hooks(monkeypatch, stage=None, out=None, pass_nodes=None):
    for name, v in (("stage", stage), ("out", out), ("pass_nodes", pass_nodes)):
        if v:
            monkeypatch.setenv(HOOKS[name], str(v))
        else:
            monkeypatch.delenv(HOOKS[name], raising=False)


def as_ctr(db, path):
    labs = E.label_lines_of(db)
    ix = np.array([labs.index(l) for _, l in db.nodes], dtype=np.uint32)
    hi = np.array([w >> 64 for w, _ in db.nodes], dtype=np.uint64)
    lo = np.array([w & 0xFFFFFFFFFFFFFFFF for w, _ in db.nodes], dtype=np.uint64)
    ctrfile.write_ctr(path, db.W, db.I, hi, lo, ix, [l.decode("latin-1") for l in labs])
    return path


def write_inputs(tmp_path, inputs, tag="in", ctr=()):
    paths = []
    for i, db in enumerate(inputs):
        if i in ctr:
            paths.append(as_ctr(db, str(tmp_path / ("%s%d.ctr" % (tag, i)))))
        else:
            paths.append(str(tmp_path / ("%s%d.ubt" % (tag, i))))
            open(paths[-1], "wb").write(M.db_file(db))
    return paths


def pair(W, I, bad=False):
    """513 and 300 nodes.  Every fourth word of the first is in the second too.  The first carries five labels at random -- neighbouring
    lanes of a wavefront count for different labels -- but for 80 nodes in a row under one (a wavefront of one label counts once).  The
    second's labels share two ranks with the first's, so a shared word is relabelled "k__A;p__B" unless both texts are equal; with `bad`
    every third shared word meets a text of another kingdom and is dropped."""
    r = M.rng(W, I, 901)
    words = M.random_words(r, W, 513 + 171)
    r.shuffle(words)
    wa, own = sorted(words[:513]), words[513:]
    stem = b"k__A;p__B;c__L"
    a = [(w, stem + b"%d" % (2 if 200 <= j < 280 else int(r.integers(0, 5)))) for j, w in enumerate(wa)]
    b = [(w, b"k__Z;p__Y" if bad and j % 12 == 0 else stem + b"%d" % int(r.integers(0, 5))) for j, w in enumerate(wa) if j % 4 == 0]
    b += [(w, stem + b"%d;o__own" % int(r.integers(0, 5))) for w in own]
    return [Db(W, I, a), Db(W, I, sorted(b))]


def run_merge(tmp_path, paths, tag, **kw):
    out = str(tmp_path / (tag + ".ubt"))
    st = search.merge(paths, out, **kw)
    data = open(out, "rb").read()
    os.unlink(out)
    return data, st


def check_merge(tmp_path, monkeypatch, inputs, paths, gg=True, **hk):
    """the hooked merge = merge_ref = the same call without the hooks; returns the hooked run's stats"""
    want, ws = M.merge(inputs, gg)
    hooks(monkeypatch)
    plain, pst = run_merge(tmp_path, paths, "plain", gg=gg)
    hooks(monkeypatch, **hk)
    got, st = run_merge(tmp_path, paths, "hooked", gg=gg)
    assert got == want
    assert {k: getattr(st, k) for k in ws} == ws
    assert plain == want and {k: getattr(pst, k) for k in ws} == ws
    assert (st.W, st.I, st.n_inputs) == (pst.W, pst.I, pst.n_inputs) == (inputs[0].W, max(d.I for d in inputs), len(inputs))
    return st


def label_counts(data, W, I):
    """the count on every label line of a `.ubt`"""
    n = int(np.frombuffer(data[24:32], dtype="<u8")[0])
    return [int(l.split(b"\t")[1]) for l in data[32 + n * (W + I):].split(b"\n")[:-1]]


# ---- the staging buffers --------------------------------------------------------------------------------------------------------------------------
STAGE = ["7", "256", "1000", "B-1", "B", "B+1"]


@pytest.mark.parametrize("stage", STAGE)
@pytest.mark.parametrize("W,I,ctr", [(8, 2, False), (4, 2, False), (16, 4, False), (8, 2, True), (16, 2, True)])
def test_staging(W, I, ctr, stage, tmp_path, monkeypatch):
    """B: the bytes of the larger slice.  7 cuts every record in two (no record is 7 bytes) and makes hundreds of chunks; 256 and 1000 are
    multiples of no record size here but 256 = 16 x 16 (W = 16 as `.ctr`: 13 + 2 = 15 bytes, `.ubt`: 20), so the larger slice takes at
    least six chunks and both buffers are used again; B - 1 leaves a second chunk of one byte, B and B + 1 are one chunk.  With the second
    input a `.ctr`, its bin table goes up between the first slice's chunks and its own."""
    inputs = pair(W, I)
    paths = write_inputs(tmp_path, inputs, ctr=(1,) if ctr else ())
    big = 513 * (W + I)
    stage_bytes = {"B-1": big - 1, "B": big, "B+1": big + 1}.get(stage) or int(stage)
    st = check_merge(tmp_path, monkeypatch, inputs, paths, stage=stage_bytes)
    assert st.n_passes == 1 and st.n_shared == 129 and 0 < st.n_relabelled < 129 and st.n_dropped == 0


# ---- the output chunks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["1", "63", "64", "65", "256", "n-1", "n", "n+1"])
@pytest.mark.parametrize("bad", [False, True])
def test_output_chunks(bad, out, tmp_path, monkeypatch):
    """n: the nodes the reference writes.  With `bad`, n is less than the sorted count, and a chunk's first node indexes the compacted
    arrays.  The counts of the label lines add up over the chunks."""
    inputs = pair(8, 2, bad)
    want, ws = M.merge(inputs)
    n = ws["n_nodes"]
    assert n == 684 - ws["n_dropped"] and (ws["n_dropped"] >= 1) == bad
    out_nodes = {"n-1": n - 1, "n": n, "n+1": n + 1}.get(out) or int(out)
    hooks(monkeypatch, out=out_nodes)
    got, st = run_merge(tmp_path, write_inputs(tmp_path, inputs), "hooked")
    assert label_counts(got, 8, 2) == label_counts(want, 8, 2) and sum(label_counts(got, 8, 2)) == n
    assert got == want
    assert {k: getattr(st, k) for k in ws} == ws
    hooks(monkeypatch)
    plain, _ = run_merge(tmp_path, write_inputs(tmp_path, inputs), "plain")
    assert plain == want


@pytest.mark.parametrize("W,I", [(4, 2), (16, 4)])
def test_output_chunks_other_widths(W, I, tmp_path, monkeypatch):
    inputs = pair(W, I, bad=True)
    check_merge(tmp_path, monkeypatch, inputs, write_inputs(tmp_path, inputs), out=65)


# ---- both, and the passes -------------------------------------------------------------------------------------------------------------------------
def eight_inputs():
    """test_gpu_merge.py's test_eight_inputs"""
    r = M.rng(8)
    words = M.random_words(r, 8, 400)
    ins = []
    for i in range(8):
        pick = sorted(set(int(j) for j in r.integers(0, 400, 150)))
        ins.append(Db(8, 2 if i % 2 else 4, [(words[j], LABS[int(r.integers(0, len(LABS)))]) for j in pick]))
    return ins


def test_eight_inputs_in_passes_and_chunks(tmp_path, monkeypatch):
    """two sweeps over several passes, every slice in several staging chunks, every pass's output in several chunks: emit is entered once
    per pass and the label counts add up over all of it"""
    ins = eight_inputs()
    st = check_merge(tmp_path, monkeypatch, ins, write_inputs(tmp_path, ins), stage=257, out=65, pass_nodes=100)
    assert st.n_inputs == 8 and st.n_passes > 4 and st.n_dropped > 0 and st.n_relabelled > 0


# ---- the edit -------------------------------------------------------------------------------------------------------------------------------------
def rule_paths(tmp_path, r):
    out = {}
    for which in ("drop", "keep", "rename"):
        lines = getattr(r, which)
        if lines is not None:
            out[which] = str(tmp_path / (which + ".rules"))
            open(out[which], "wb").write(E.rule_file(lines))
    return out


@pytest.mark.parametrize("pass_nodes", [None, 64])
@pytest.mark.parametrize("name", ["minus", "one_side_dropped", "cut_makes_fold"])
def test_edit(name, pass_nodes, tmp_path, monkeypatch):
    """a MINUS input (its slices are staged first, in chunks like the others, and its records must still head their runs), a dropped label,
    a cut to three ranks"""
    inputs, r, minus, gg = E.edit_cases()[name]
    assert (name == "minus") == bool(minus) and (name == "one_side_dropped") == (r.drop is not None) and (name == "cut_makes_fold") == bool(r.ranks)
    paths, mp = write_inputs(tmp_path, inputs), write_inputs(tmp_path, minus, "minus")
    want, ws, wes = E.merge(inputs, r, minus, gg)
    outs = []
    for tag, hk in (("hooked", dict(stage=257, out=65, pass_nodes=pass_nodes)), ("plain", {})):
        hooks(monkeypatch, **hk)
        out = str(tmp_path / (tag + ".ubt"))
        st, es = search.merge_edit(paths, out, gg=gg, ranks=r.ranks, minus=mp, **rule_paths(tmp_path, r))
        outs.append(open(out, "rb").read())
        assert outs[-1] == want
        assert {k: getattr(st, k) for k in ws} == ws
        assert {k: getattr(es, k) for k in wes} == wes
        if tag == "hooked" and pass_nodes:
            assert st.n_passes > 1


# ---- the compare and the inspect: the same staging, no output half ---------------------------------------------------------------------------------
def prefix_sums(fig, texts, keys):
    """text or cut of a text before a ';' -> the sums of fig[x][k] over the texts x in its clade"""
    out = {}
    for t in texts:
        for p in [t] + [t[:i] for i, c in enumerate(t) if c == 0x3B]:
            row = out.setdefault(p, [0] * len(keys))
            for j, k in enumerate(keys):
                row[j] += fig[t][k]
    return out


def compare_files(fig, moves, st, a_desc, b_desc):
    """compare_ref.files with the clade columns summed per prefix, not per pair of rows (test_compare_and_inspect_staging pins the two to
    each other): 70 000 labels would take it hours"""
    out = []
    for tag, (path, layout, W, I), n, labels in ((b"a", a_desc, st["a"], st["a_labels"]), (b"b", b_desc, st["b"], st["b_labels"])):
        out.append(b"# %s\t%s\t%s\t%d\t%d\t%d\t%d\n" % (tag, path.encode(), layout.encode(), W, I, n, labels))
    out.append(b"# words\t%d\tboth\t%d\tsame\t%d\tchanged\t%d\tonly_a\t%d\tonly_b\t%d\n"
               % (st["words"], st["both"], st["same"], st["left"], st["only_a"], st["only_b"]))
    out.append(b"# taxon\ta\tb\tsame\tonly_a\tonly_b\tleft\tarrived\tclade_a\tclade_b\n")
    clade = prefix_sums(fig, [t for t, r in fig.items() if r["a"] + r["b"]], ("a", "b"))
    zero = dict.fromkeys(CR.FIGURES, 0)
    for t in sorted(clade):
        r = fig.get(t, zero)
        out.append(t + b"".join(b"\t%d" % v for v in [r[k] for k in CR.FIGURES] + clade[t]) + b"\n")
    mv = [b"# from\tto\tkmers\tkind\n"]
    for (frm, to), n in sorted(moves.items()):
        mv.append(frm + b"\t" + to + b"\t%d\t" % n + CR.kind(frm, to).encode() + b"\n")
    return b"".join(out), b"".join(mv)


def inspect_files(fig, pairs, st, desc):
    """inspect_ref.files, likewise"""
    path, layout, W, I = desc
    out = [b"# db\t%s\t%s\t%d\t%d\t%d\t%d\n" % (path.encode(), layout.encode(), W, I, st["kmers"], st["labels"])]
    out.append(b"# kmers\t%d\tisolated\t%d\tsame\t%d\tlineage\t%d\tconflict\t%d\tpair_events\t%d\tdistinct_pairs\t%d\n"
               % (st["kmers"], st["isolated"], st["same"], st["lineage"], st["conflict"], st["pair_events"], st["distinct_pairs"]))
    out.append(b"# taxon\tkmers\tisolated\tsame\tlineage\tconflict\tclade_kmers\tclade_conflict\n")
    clade = prefix_sums(fig, [t for t, r in fig.items() if r["kmers"]], ("kmers", "conflict"))
    zero = dict.fromkeys(IR.FIGURES, 0)
    for t in sorted(clade):
        r = fig.get(t, zero)
        out.append(t + b"".join(b"\t%d" % v for v in [r[k] for k in IR.FIGURES] + clade[t]) + b"\n")
    pr = [b"# from\tto\tpairs\tkind\n"]
    for (frm, to), n in sorted(pairs.items()):
        pr.append(frm + b"\t" + to + b"\t%d\t" % n + IR.kind(frm, to).encode() + b"\n")
    return b"".join(out), b"".join(pr)


def run_compare(tmp_path, pa, pb, tag):
    rep, mov = str(tmp_path / (tag + "_report.tsv")), str(tmp_path / (tag + "_moves.tsv"))
    st = search.compare(pa, pb, rep, mov)
    return st, open(rep, "rb").read(), open(mov, "rb").read()


def run_inspect(tmp_path, p, tag):
    rep, prs = str(tmp_path / (tag + "_report.tsv")), str(tmp_path / (tag + "_pairs.tsv"))
    st = search.inspect(p, rep, prs)
    return st, open(rep, "rb").read(), open(prs, "rb").read()


def many_moves():
    """test_gpu_compare.py's test_many_moves"""
    r = M.rng(6)
    words = M.random_words(r, 8, 2400)
    la = [b"k__A;p__P%d;c__a%d" % (i % 7, i) for i in range(300)]
    lb = [b"k__A;p__P%d;c__b%d" % (i % 5, i) for i in range(300)]
    return (Db(8, 2, [(w, la[int(r.integers(0, 300))]) for w in words[:2000]]),
            Db(8, 4, [(w, lb[int(r.integers(0, 300))]) for w in words[400:]]))


def every_class():
    """test_gpu_inspect.py's test_every_class_and_every_kind"""
    SP_A, SP_B = M.G + b";s__a", M.G + b";s__b"
    x, y, z, q, e = 0x1111 << 20, 0x2222 << 36, 0x3333 << 44, 0x77 << 50, 0x99 << 54
    return Db(8, 2, sorted([(x, SP_A), (x ^ 1, SP_A), (x ^ (2 << 10), SP_A), (y, SP_B), (y ^ (1 << 2), M.G), (z, b"k__A;p__B"),
                            (z ^ 3, b"k__A;p__Bx"), (q, b";p__E"), (q ^ (1 << 40), b";p__E;c__F"), (e, b"k__Z")]))


@pytest.mark.parametrize("stage", [7, 1000])
def test_compare_and_inspect_staging(stage, tmp_path, monkeypatch):
    """both tools under small staging chunks, and with the output hook set as well: they write no nodes, so it must change nothing"""
    a, b = many_moves()
    pa, pb = write_inputs(tmp_path, [a, b], "cmp")
    fig, moves, ws = CR.compare(a, b)
    want = CR.files(fig, moves, ws, (pa, ".ubt", 8, 2), (pb, ".ubt", 8, 4))
    assert compare_files(fig, moves, ws, (pa, ".ubt", 8, 2), (pb, ".ubt", 8, 4)) == want
    db = every_class()
    pd = write_inputs(tmp_path, [db], "ins")[0]
    ifig, pairs, iws = IR.inspect(db)
    iwant = IR.files(ifig, pairs, iws, (pd, ".ubt", 8, 2))
    assert inspect_files(ifig, pairs, iws, (pd, ".ubt", 8, 2)) == iwant
    for tag, hk in (("plain", {}), ("staged", dict(stage=stage)), ("both", dict(stage=stage, out=1)), ("out", dict(out=1))):
        hooks(monkeypatch, **hk)
        st, rep, mov = run_compare(tmp_path, pa, pb, tag)
        assert (rep, mov) == want, tag
        assert {k: getattr(st, k) for k in ws} == ws, tag
        assert st.n_passes == 1 and st.n_moves > 1000
        st, rep, prs = run_inspect(tmp_path, pd, tag)
        assert (rep, prs) == iwant, tag
        assert {k: getattr(st, k) for k in iws} == iws, tag


# ---- label ids above 2^16 -------------------------------------------------------------------------------------------------------------------------
N_FILL = 66000


def filler(i):
    return b"k__F;p__F;c__F;o__F;f__F%d;g__G%d;s__%d" % (i % 40, i % 1600, i)


def high(tag, i):
    return b"k__H;p__H;c__H;o__H;f__%s%d;g__G%d;s__%d" % (tag, i % 20, i % 400, i)


def first_line_of(db):
    """label text -> its line in merge_ref.db_file's label tail (the first input's lines are interned in this order, so a text's id in the
    universe is its line at the least)"""
    return {t: i for i, t in enumerate(E.label_lines_of(db))}


def test_compare_ids_above_65535(tmp_path, monkeypatch):
    """70 000 seven-rank texts over 75 000 words of A.  The 66 000 lowest words of A carry 66 000 filler texts, one each, so every text met
    later -- the 2 000 that A's 9 000 highest words carry, and the 2 000 other ones B gives those words -- has an id above 65 535: in the
    value word, in the counters' slots, in the move key and in what is read back.  An id cut to 16 bits would name a filler text."""
    hooks(monkeypatch)
    r = M.rng(70000, 1)
    words = M.random_words(r, 8, 75000)
    a = Db(8, 4, [(w, filler(j)) for j, w in enumerate(words[:N_FILL])]
           + [(w, high(b"A", j % 2000 if j < 2000 else int(r.integers(0, 2000)))) for j, w in enumerate(words[N_FILL:])])
    b = Db(8, 4, [(w, filler(j)) for j, w in list(enumerate(words[:N_FILL]))[::100]]
           + [(w, high(b"B", j % 2000 if j < 2000 else int(r.integers(0, 2000)))) for j, w in enumerate(words[N_FILL:])])
    line = first_line_of(a)
    assert len(line) == 68000 and len(set(line) | set(t for _, t in b.nodes)) == 70000
    pa, pb = write_inputs(tmp_path, [a, b], "ids")
    fig, moves, ws = CR.compare(a, b)
    assert len(moves) >= 1000 and all(line[f] >= N_FILL and t not in line for f, t in moves)
    want = compare_files(fig, moves, ws, (pa, ".ubt", 8, 4), (pb, ".ubt", 8, 4))
    st, rep, mov = run_compare(tmp_path, pa, pb, "ids")
    assert mov == want[1]
    assert rep == want[0]
    assert {k: getattr(st, k) for k in ws} == ws
    assert st.n_moves >= 1000 and st.left == 9000 and st.same == 660 and st.only_a == N_FILL - 660


def test_inspect_ids_above_65535(tmp_path, monkeypatch):
    """70 000 seven-rank texts over 75 000 words.  The 66 000 words below 2^63 carry 66 000 filler texts, one each; the 9 000 words above
    are 4 500 pairs one substitution apart (below the top base, so both stay above), under 4 000 texts whose ids are therefore above 65 535."""
    hooks(monkeypatch)
    monkeypatch.delenv("UTREE_INSPECT_PAIRS", raising=False)
    r = M.rng(70000, 2)
    top = 1 << 63
    low = sorted(set(w & (top - 1) for w in M.random_words(r, 8, N_FILL + 50)))[:N_FILL]
    up = {}
    for w in M.random_words(r, 8, 6000):
        if len(up) >= 9000:
            break
        v = IR.mutate(8, w | top, int(r.integers(0, 31)), int(r.integers(1, 4)))
        if (w | top) not in up and v not in up:
            up[w | top] = up[v] = None
    assert len(low) == N_FILL and len(up) == 9000
    db = Db(8, 4, [(w, filler(j)) for j, w in enumerate(low)] + [(w, high(b"I", j % 4000)) for j, w in enumerate(sorted(up))])
    line = first_line_of(db)
    assert len(line) == 70000
    fig, pairs, ws = IR.inspect(db)
    IR.check_invariants(fig, pairs, ws)
    n_high = sum(line[f] >= N_FILL and line[t] >= N_FILL for f, t in pairs)
    assert n_high >= 100 and n_high >= len(pairs) - 200               # (two random words one substitution apart: a handful at the most)
    p = write_inputs(tmp_path, [db], "ids")[0]
    want = inspect_files(fig, pairs, ws, (p, ".ubt", 8, 4))
    st, rep, prs = run_inspect(tmp_path, p, "ids")
    assert prs == want[1]
    assert rep == want[0]
    assert {k: getattr(st, k) for k in ws} == ws
    assert st.distinct_pairs >= 100 and st.labels == 70000
