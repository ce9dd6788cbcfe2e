"""Editing while merging, without a GPU: the surface of the ABI, the argument checks (before any file is touched), the label edit and the
rule files through the host-only preview (utree_merge_edit_preview), the yardstick -- tests/merge_edit_ref.py pinned to the GENUINE builder
on the imagined FASTA of the edited inputs -- and label_edit.c under AddressSanitizer as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import pytest

import merge_edit_ref as E
import merge_ref as M
import util
from oracle import orc
from utree_amd import lib, search

REF = os.path.join(util.ROOT, "oracle", "_ref")
CSRC = os.path.join(util.ROOT, "utree_amd", "csrc")


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------------------
def test_names_are_declared_bound_and_exported():
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in ("utree_merge_files_edit", "utree_merge_edit_preview"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in lib.SYMBOLS and hasattr(L, name)
    for t in ("utree_merge_edit", "utree_merge_edit_stats"):
        assert "} %s;" % t in hdr
    assert C.sizeof(lib.MergeEdit) == 48 and C.sizeof(lib.MergeEditStats) == 64          # the header's layouts on LP64
    flat = " ".join(hdr.split()).replace(" * ", " ")
    for limit in ("k-mers that an earlier fold lifted to an ancestor and k-mers an earlier build dropped as BAD do not change back",
                  "A rename does not re-fold earlier folds", "MINUS is by identical word, as stored",
                  "A MINUS database built above compression level 0 holds only a sample of its k-mers"):
        assert limit in flat, limit
    steps = [flat.index(s) for s in ("1. clade match", "2. selection, on the original text", "3. rename", "4. ranks", "5. empty result")]
    assert steps == sorted(steps)


def test_sizes_the_library_checks_are_the_bindings(tmp_path):
    """utree_merge_edit.size is checked against the C struct: the binding's size passes, any other is UTREE_E_ARG"""
    p = str(tmp_path / "a.ubt")
    open(p, "wb").write(M.db_file(M.Db(8, 2, [(5, b"k__A;p__B")])))
    arr = (C.c_char_p * 1)(p.encode())
    L = lib.load()
    es = lib.MergeEditStats()
    ed = lib.MergeEdit()
    assert ed.size == C.sizeof(lib.MergeEdit)
    assert L.utree_merge_edit_preview(arr, 1, C.byref(ed), str(tmp_path / "p.tsv").encode(), C.byref(es)) == lib.OK and es.n_label_lines == 1
    for size in (0, 40, 47, 49, 56):
        ed.size = size
        assert L.utree_merge_edit_preview(arr, 1, C.byref(ed), str(tmp_path / "q.tsv").encode(), C.byref(es)) == lib.E_ARG
    assert not os.path.exists(str(tmp_path / "q.tsv"))


def test_nothing_pinned_moved():
    L = lib.load()
    assert L.utree_abi_version() == 4
    assert C.sizeof(lib.MergeStats) == 72 and C.sizeof(lib.MergeInput) == 32 and C.sizeof(lib.SearchRequest) == 128


def test_argument_checks_come_before_any_file(tmp_path):
    L = lib.load()
    out, tsv = str(tmp_path / "never.ubt"), str(tmp_path / "never.tsv")
    missing = str(tmp_path / "missing.ubt").encode()
    arr = (C.c_char_p * 1)(missing)
    st, es = lib.MergeStats(), lib.MergeEditStats()

    def both(ed):
        return (L.utree_merge_files_edit(arr, 1, out.encode(), 0, 1, 0, C.byref(ed), C.byref(st), C.byref(es)),
                L.utree_merge_edit_preview(arr, 1, C.byref(ed), tsv.encode(), C.byref(es)))
    ed = lib.MergeEdit()
    ed.size = 8
    assert both(ed) == (lib.E_ARG, lib.E_ARG)
    assert both(lib.MergeEdit(ranks=256)) == (lib.E_ARG, lib.E_ARG)
    assert both(lib.MergeEdit(n_minus=-1)) == (lib.E_ARG, lib.E_ARG)
    assert both(lib.MergeEdit(n_minus=1)) == (lib.E_ARG, lib.E_ARG)                         # a NULL array
    one = (C.c_char_p * 1)(None)
    assert both(lib.MergeEdit(n_minus=1, minus_paths=C.cast(one, C.POINTER(C.c_char_p)))) == (lib.E_ARG, lib.E_ARG)   # a NULL entry
    # a bad rule file path would be UTREE_E_IO, a missing input too: the argument comes first
    assert both(lib.MergeEdit(ranks=300, drop_path=str(tmp_path / "no_rules").encode())) == (lib.E_ARG, lib.E_ARG)
    assert both(lib.MergeEdit(ranks=255)) == (lib.E_IO, lib.E_IO)                           # in range: now the input is missed
    # utree_merge_files' own checks hold with an edit
    ok = lib.MergeEdit()
    assert L.utree_merge_files_edit(arr, 0, out.encode(), 0, 1, 0, C.byref(ok), C.byref(st), C.byref(es)) == lib.E_ARG
    assert L.utree_merge_files_edit(arr, 1, out.encode(), 3, 1, 0, C.byref(ok), C.byref(st), C.byref(es)) == lib.E_ARG
    assert L.utree_merge_files_edit(arr, 1, None, 0, 1, 0, C.byref(ok), C.byref(st), C.byref(es)) == lib.E_ARG
    assert L.utree_merge_edit_preview(arr, 1, None, tsv.encode(), C.byref(es)) == lib.E_ARG
    assert L.utree_merge_edit_preview(arr, 1, C.byref(ok), None, C.byref(es)) == lib.E_ARG
    assert L.utree_merge_edit_preview(None, 1, C.byref(ok), tsv.encode(), C.byref(es)) == lib.E_ARG
    assert not os.path.exists(out) and not os.path.exists(tsv)


# ---- 2. the label edit and the rule files, through the preview ---------------------------------------------------------------------------
LABELS = [b"k__A;p__B;c__C;o__D", b"k__A;p__B;c__C;o__E", b"k__A;p__Bx;c__C", b"k__A;p__B", b"k__A", b"k__Z;p__Y;c__W;o__V;f__U",
          b"k__Z;p__Y", b"k__With space;p__\x80\xfe\xff;c__x", b"B;x", b"C;y", b";x"]


def write_db(tmp_path, labels=LABELS, name="db.ubt", W=8):
    """one node per label, word j under labels[j]; the file's lines state 1 node each"""
    p = str(tmp_path / name)
    open(p, "wb").write(M.db_file(M.Db(W, 2, [(10 + j, l) for j, l in enumerate(labels)])))
    return p


def run_preview(tmp_path, db, raw=None, **kw):
    """the preview with the rule files given as bytes (raw: {which: bytes}) or as merge_edit_ref rule lines (kw): (tsv bytes, stats, paths)"""
    paths = {}
    for which in ("drop", "keep", "rename"):
        data = (raw or {}).get(which)
        if data is None and kw.get(which) is not None:
            data = E.rule_file(kw[which])
        if data is not None:
            paths[which] = str(tmp_path / (which + ".rules"))
            open(paths[which], "wb").write(data)
    tsv = str(tmp_path / "preview.tsv")
    es = search.merge_preview([db], tsv, ranks=kw.get("ranks", 0), **paths)
    return open(tsv, "rb").read(), es, paths


def rows(tsv: bytes):
    """label text -> (stated count, action, edited text)"""
    out = {}
    for line in tsv.split(b"\n")[:-1]:
        if not line.startswith(b"# "):
            t, c, a, e = line.split(b"\t")
            out[t] = (int(c), a.decode(), e)
    return out


def check_preview(tmp_path, labels=LABELS, **kw):
    db = write_db(tmp_path, labels)
    got, es, paths = run_preview(tmp_path, db, **kw)
    r = E.rules(kw.get("ranks", 0), kw.get("drop"), kw.get("keep"), kw.get("rename"))
    want, figures = E.preview([(db, ".ubt", len(labels), [(l, 1) for l in labels])], r, paths)
    assert got == want
    assert {k: getattr(es, k) for k in figures} == figures
    return rows(got), es


def test_clade_match_is_not_a_prefix_match(tmp_path):
    r, es = check_preview(tmp_path, drop=[b"k__A;p__B"])
    assert [t for t, v in r.items() if v[1] == "drop"] == [b"k__A;p__B;c__C;o__D", b"k__A;p__B;c__C;o__E", b"k__A;p__B"]
    assert r[b"k__A;p__Bx;c__C"] == (1, "keep", b"k__A;p__Bx;c__C") and es.n_nodes_dropped == 3


def test_longest_old_wins_and_nothing_chains(tmp_path):
    r, _ = check_preview(tmp_path, rename=[(b"k__A", b"k__N"), (b"k__A;p__B", b"k__A;p__Q"), (b"k__A;p__Q", b"k__A;p__R"), (b"B", b"C"), (b"C", b"D")])
    assert r[b"k__A;p__B;c__C;o__D"][2] == b"k__A;p__Q;c__C;o__D"                            # not k__N..., and not ...p__R
    assert r[b"k__A;p__Bx;c__C"][2] == b"k__N;p__Bx;c__C" and r[b"k__A"][2] == b"k__N"
    assert r[b"B;x"] == (1, "rename", b"C;x") and r[b"C;y"] == (1, "rename", b"D;y")          # A -> B and B -> C leave an A label at B
    assert r[b"k__Z;p__Y"][1] == "keep"


def test_drop_beats_keep_and_selection_sees_the_original_text(tmp_path):
    r, es = check_preview(tmp_path, keep=[b"k__A", b"k__Q"], drop=[b"k__A;p__B;c__C", b"k__N"], rename=[(b"k__A", b"k__N"), (b"k__Z", b"k__Q")])
    assert r[b"k__A;p__B;c__C;o__D"][1] == "drop" and r[b"k__A;p__B"] == (1, "rename", b"k__N;p__B")   # k__N is dropped by name, its new bearer is not
    assert r[b"k__Z;p__Y"][1] == "drop"                                                     # it becomes k__Q only after the selection
    assert es.n_rules_unmatched == 2 and es.n_labels_dropped == 8


def test_ranks_apply_after_the_rename(tmp_path):
    r, es = check_preview(tmp_path, ranks=2, rename=[(b"k__Z;p__Y;c__W", b"k__Z")])
    assert r[b"k__Z;p__Y;c__W;o__V;f__U"] == (1, "rename+cut", b"k__Z;o__V")                  # cut of the renamed text, not rename of the cut one
    assert r[b"k__A;p__B;c__C;o__D"] == (1, "cut", b"k__A;p__B") and r[b"k__A;p__B"][1] == "keep" and r[b"k__A"][1] == "keep"
    assert es.n_labels_cut == 5 and es.n_labels_renamed == 1
    r, es = check_preview(tmp_path, ranks=9)
    assert all(v[1] == "keep" and v[2] == t for t, v in r.items()) and es.n_labels_cut == 0 # more ranks than any label has tokens


def test_an_empty_result_is_refused(tmp_path):
    db = write_db(tmp_path)
    with pytest.raises(lib.UtreeError) as e:
        run_preview(tmp_path, db, ranks=1)
    assert e.value.code == lib.E_FORMAT and "`;x`" in e.value.detail
    assert not os.path.exists(str(tmp_path / "preview.tsv"))
    with pytest.raises(E.EmptyLabel):
        E.edited([M.Db(8, 2, [(1, b";x")])], E.rules(ranks=1))
    got, _, _ = run_preview(tmp_path, db, ranks=1, keep=[b"k__A", b"k__Z", b"B", b"C", b"k__With space"])
    assert rows(got)[b";x"][1] == "drop"                                                    # a dropped label is never empty


def test_crlf_last_line_without_newline_spaces_and_high_bytes(tmp_path):
    db = write_db(tmp_path)
    raw = {"drop": b"\r\nk__Z;p__Y\r\n\r\nk__Never\r\n\n", "keep": b"k__With space\nk__Z\r\nk__A",
           "rename": b"k__With space;p__\x80\xfe\xff\tk__ \xff\r\n\nB\tC"}
    got, es, paths = run_preview(tmp_path, db, raw=raw)
    r = rows(got)
    assert r[b"k__With space;p__\x80\xfe\xff;c__x"] == (1, "rename", b"k__ \xff;c__x")
    assert r[b"k__Z;p__Y"][1] == "drop" and r[b"k__A"][1] == "keep" and r[b"B;x"][1] == "drop"
    assert es.n_rules_unmatched == 1
    assert got.split(b"\n")[-2] == b"# unmatched\t%s\t4\tk__Never" % paths["drop"].encode()
    assert b"# unmatched\t%s\t3\tB" % paths["rename"].encode() not in got                   # B;x was looked at, and matched, before it was dropped


def test_a_repeated_label_line_counts_once_and_states_its_first_count(tmp_path):
    W, I = 8, 2
    recs = b"".join(M.word_bytes(W, w) + ix.to_bytes(I, "little") for w, ix in ((1, 0), (2, 1), (3, 1)))
    import numpy as np
    raw = np.array([W, 0, I, 3], dtype="<u8").tobytes() + recs + b"k__A;p__B\t1\nk__Z;p__Y\t1\nk__A;p__B\t0\nk__Z;p__Y\t1\nk__Never;p__Seen\t0\n"
    p = str(tmp_path / "rep.ubt")
    open(p, "wb").write(raw)
    got, es, paths = run_preview(tmp_path, p, drop=[b"k__Z"])
    want, figures = E.preview([(p, ".ubt", 3, [(b"k__A;p__B", 1), (b"k__Z;p__Y", 1), (b"k__A;p__B", 0), (b"k__Z;p__Y", 1), (b"k__Never;p__Seen", 0)])],
                              E.rules(drop=[b"k__Z"]), paths)
    assert got == want and es.n_label_lines == 3 == figures["n_label_lines"] and es.n_nodes_dropped == 1 and es.n_labels_dropped == 1
    assert got.startswith(b"# input\t%s\t.ubt\t3\t3\n" % p.encode())


def test_unmatched_rules_are_listed_with_file_and_line(tmp_path):
    db = write_db(tmp_path)
    got, es, paths = run_preview(tmp_path, db, raw={"drop": b"k__Typo\n\nk__Z\nk__Typo\n", "keep": b"k__A\nk__Z\nB\nC\n;x\nk__With space\nk__A;p__C\n",
                                                    "rename": b"k__A;p__By\tq\nk__A\tk__A\n"})
    tail = [l for l in got.split(b"\n") if l.startswith(b"# unmatched")]
    assert tail == [b"# unmatched\t%s\t1\tk__Typo" % paths["drop"].encode(), b"# unmatched\t%s\t4\tk__Typo" % paths["drop"].encode(),
                    b"# unmatched\t%s\t7\tk__A;p__C" % paths["keep"].encode(), b"# unmatched\t%s\t1\tk__A;p__By" % paths["rename"].encode()]
    assert es.n_rules_unmatched == 4


@pytest.mark.parametrize("which,data,line", [
    ("drop", b"k__A\n\nk__B\tx\n", 3), ("keep", b"\tk__A", 1), ("rename", b"a\tb\r\nno tab\r\n", 2), ("rename", b"a\tb\tc\n", 1),
    ("rename", b"a\tb\n\tc\n", 2), ("rename", b"a\tb\n\n\nc\t\n", 4), ("rename", b"a\tb\nc\td\n\na\te", 4), ("rename", b"x\ty\na\t\r\n", 2)])
def test_malformed_rule_lines_name_file_and_line(which, data, line, tmp_path):
    db = write_db(tmp_path)
    with pytest.raises(lib.UtreeError) as e:
        run_preview(tmp_path, db, raw={which: data})
    assert e.value.code == lib.E_FORMAT
    assert str(tmp_path / (which + ".rules")) in e.value.detail and "line %d:" % line in e.value.detail
    assert not os.path.exists(str(tmp_path / "preview.tsv"))


def test_a_missing_rule_file_is_an_io_error(tmp_path):
    db = write_db(tmp_path)
    for which in ("drop", "keep", "rename"):
        with pytest.raises(lib.UtreeError) as e:
            search.merge_preview([db], str(tmp_path / "p.tsv"), **{which: str(tmp_path / "missing.rules")})
        assert e.value.code == lib.E_IO and "missing.rules" in e.value.detail
    assert not os.path.exists(str(tmp_path / "p.tsv"))


def test_preview_reads_ctr_inputs_and_ignores_minus(tmp_path):
    import numpy as np
    from utree_amd import ctrfile
    db = M.Db(8, 2, [(w, b"k__S;p__L%d" % (j % 3)) for j, w in enumerate(M.random_words(M.rng(8, 2, 50, 9), 8, 50))])
    u, c = str(tmp_path / "a.ubt"), str(tmp_path / "b.ctr")
    open(u, "wb").write(M.db_file(db))
    labs = E.label_lines_of(db)
    ctrfile.write_ctr(c, 8, 2, np.zeros(50, dtype=np.uint64), np.array([w for w, _ in db.nodes], dtype=np.uint64),
                      np.array([labs.index(l) for _, l in db.nodes], dtype=np.uint32), [l.decode() for l in labs])
    tsv = str(tmp_path / "two.tsv")
    L = lib.load()
    arr = (C.c_char_p * 2)(u.encode(), c.encode())
    nowhere = (C.c_char_p * 1)(str(tmp_path / "no_such.ctr").encode())
    ed = lib.MergeEdit(ranks=1, n_minus=1, minus_paths=C.cast(nowhere, C.POINTER(C.c_char_p)))
    es = lib.MergeEditStats()
    assert L.utree_merge_edit_preview(arr, 2, C.byref(ed), tsv.encode(), C.byref(es)) == lib.OK
    lines = open(tsv, "rb").read().split(b"\n")
    assert lines[0] == b"# input\t%s\t.ubt\t50\t3" % u.encode() and lines[4] == b"# input\t%s\t.ctr\t50\t3" % c.encode()
    assert es.n_label_lines == 6 and es.n_labels_cut == 6 and es.n_minus_nodes == 0 and es.n_nodes_subtracted == 0
    counts = sorted(int(l.split(b"\t")[1]) for l in lines[1:4])
    assert sum(counts) == 50 and lines[1].endswith(b"\tcut\tk__S")


# ---- 3. merge_edit_ref against the genuine builder -----------------------------------------------------------------------------------------
def genuine(tmp_path, inputs, gg, I):
    """the `.ubt` bytes of the builder(s) on the imagined FASTA at compression level 0: {who: bytes}"""
    W = inputs[0].W
    fa, mp = M.imagined(inputs)
    fa_p, mp_p = str(tmp_path / "im.fa"), str(tmp_path / "im.map")
    open(fa_p, "wb").write(fa)
    open(mp_p, "wb").write(mp)
    out = {}
    code, _, _, _, err = orc.build_file(fa_p, mp_p, str(tmp_path / "orc.ubt"), W=W, I=I, complevel=0, gg=gg)
    assert code == 0, err
    out["oracle"] = open(str(tmp_path / "orc.ubt"), "rb").read()
    name = M.reference_binary(W, I, gg)
    exe = os.path.join(REF, name) if name else None
    if exe and os.path.exists(exe):
        p = subprocess.run([exe, fa_p, mp_p, str(tmp_path / "ref.ubt"), "1", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stdout[-300:]
        out[name] = open(str(tmp_path / "ref.ubt"), "rb").read()
    return out


CASES = [(8, 2, n) for n in E.edit_cases()] + [(4, 2, "cut_makes_fold"), (16, 2, "minus"), (8, 4, "first_carrier_dropped")]


@pytest.mark.parametrize("W,I,name", CASES)
def test_the_definition_is_the_builders(W, I, name, tmp_path):
    inputs, r, minus, gg = E.edit_cases(W, I)[name]
    want, stats, es = E.merge(inputs, r, minus, gg, I)
    fed = E.edited(inputs, r, minus)
    if not any(db.nodes for db in fed):
        import numpy as np
        assert want == np.array([W, 0, I, 0], dtype="<u8").tobytes()                       # nothing is fed: the 32-byte header alone
        return
    for who, got in genuine(tmp_path, fed, gg, I).items():
        assert got == want, "merge_edit_ref differs from %s on the imagined FASTA" % who


def test_the_cases_show_what_they_are_named_for():
    c = E.edit_cases()
    L = M._labels()
    figures = lambda name: E.merge(*c[name][:3], gg=c[name][3])
    _, st, es = figures("cut_makes_equal")
    assert st["n_shared"] == 1 and st["n_relabelled"] == 0 and es["n_labels_cut"] == 2
    data, st, _ = figures("cut_makes_fold")
    assert st["n_relabelled"] == 2 and b"\nk__A;p__B\t2\n" in data
    data, st, es = figures("one_side_dropped")
    assert st["n_shared"] == 1 and st["n_dropped"] == 0 and es["n_nodes_dropped"] == 4      # without the drop two of the four words are BAD
    assert M.merge(c["one_side_dropped"][0])[1]["n_dropped"] == 2
    data, st, es = figures("rename_makes_equal")
    assert st["n_shared"] == 2 and st["n_relabelled"] == 0 and st["n_labels"] == 3 and L["LB"] not in data
    data, st, es = figures("first_carrier_dropped")
    tail = M.parse_labels(data[32 + st["n_nodes"] * 10:])
    assert tail.index(b"k__A;p__B") > 0 and es["n_nodes_dropped"] == 3                      # not label 0, though the first record would have made it so
    data, st, es = figures("minus")
    assert es["n_nodes_subtracted"] == 5 and es["n_minus_nodes"] == 14 and st["n_shared"] == 1


# ---- 4. label_edit.c under AddressSanitizer, stand-alone ------------------------------------------------------------------------------------
def test_label_edit_under_the_sanitizers(tmp_path):
    probe = str(tmp_path / "probe.c")
    open(probe, "w").write("int main(void) { return 0; }\n")
    cc = os.environ.get("CC", "cc")
    try:
        p = subprocess.run([cc, "-fsanitize=address,undefined", probe, "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except OSError:
        pytest.skip("no C compiler")
    if p.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtime")
    exe = str(tmp_path / "label_edit_asan")
    p = subprocess.run(["make", "-s", "-C", CSRC, "label-edit-asan", "LABEL_EDIT_ASAN=" + exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and b"label_edit_asan: ok" in p.stdout, p.stdout[-2000:].decode(errors="replace")
    assert b"ERROR: AddressSanitizer" not in p.stdout and b"runtime error" not in p.stdout
