"""The database compare without a GPU: the surface of the ABI, the argument checks (which come before any file or device is touched), the
host-only writer utree_compare_write pinned byte for byte to tests/compare_ref.py, and compare_ref's own invariants."""
import ctypes as C
import os
import re

import pytest

import compare_ref as R
import merge_ref as M
import util
from utree_amd import lib, search

A_DESC, B_DESC = ("old dir/a.ubt", ".ubt", 8, 2), ("new/b.ctr", ".ctr", 8, 4)


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------------------
def test_names_are_declared_bound_and_exported():
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in ("utree_compare_files", "utree_compare_write"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in lib.SYMBOLS and hasattr(L, name)
    for t in ("utree_compare_stats", "utree_compare_input", "utree_compare_entry", "utree_compare_move"):
        assert "} %s;" % t in hdr
    assert lib.COMPARE_CLI_PATH.endswith("utree-compare") and callable(search.compare)
    for text in ("a = same + only_a + left", "b = same + only_b + arrived", "sum(left) = sum(arrived) = changed", "compared as stored",
                 "different compression levels", "indistinguishable from one that was"):
        assert text in hdr, "the header states the definition, the invariants and the limits"


def test_the_stats_layout_is_the_headers():
    """twelve 64-bit figures, four 32-bit ones, a double: 120 bytes, fields in the header's order"""
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    body = hdr[:hdr.index("} utree_compare_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {"):], flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        parts = decl.replace(",", " ").split()
        names += parts[1:]
    assert names == [f[0] for f in lib.CompareStats._fields_]
    assert C.sizeof(lib.CompareStats) == 12 * 8 + 4 * 4 + 8 == 120
    assert C.sizeof(lib.CompareInput) == 24 and C.sizeof(lib.CompareEntry) == 56 and C.sizeof(lib.CompareMove) == 16


def test_nothing_else_moved():
    L = lib.load()
    assert L.utree_abi_version() == 4
    assert C.sizeof(lib.SearchRequest) == 128 and lib.SearchRequest._fields_[-1][0] == "redistribute_reads_path"
    assert C.sizeof(lib.MergeStats) == 72 and C.sizeof(lib.MergeInput) == 32


def test_argument_checks_come_before_any_file(tmp_path):
    L = lib.load()
    rep, mov = str(tmp_path / "never.tsv").encode(), str(tmp_path / "never_moves.tsv").encode()
    missing = str(tmp_path / "missing.ubt").encode()
    good = str(tmp_path / "good.ubt")
    open(good, "wb").write(M.db_file(M.Db(8, 2, [(5, b"k__A;p__B")])))
    st = lib.CompareStats()
    assert L.utree_compare_files(None, missing, rep, mov, 0, C.byref(st)) == lib.E_ARG
    assert L.utree_compare_files(missing, None, rep, mov, 0, C.byref(st)) == lib.E_ARG
    assert L.utree_compare_files(missing, missing, None, mov, 0, C.byref(st)) == lib.E_ARG
    assert L.utree_compare_files(missing, missing, rep, mov, 0, None) == lib.E_ARG
    assert L.utree_compare_files(missing, missing, rep, mov, 0, C.byref(st)) == lib.E_IO          # only now is a file looked for
    assert L.utree_compare_files(good.encode(), missing, rep, None, 0, C.byref(st)) == lib.E_IO   # ... and B before any device
    assert b"missing.ubt" in L.utree_last_hip_error()
    assert not os.path.exists(rep) and not os.path.exists(mov)
    with pytest.raises(lib.UtreeError) as e:
        search.compare(good, missing.decode(), rep.decode())
    assert e.value.code == lib.E_IO and "cannot open" in e.value.detail


# ---- 2. the writer against the definition --------------------------------------------------------------------------------------------------
def write(tmp_path, fig, moves, a_desc=A_DESC, b_desc=B_DESC, with_moves=True, repeat=False):
    """utree_compare_write on compare_ref's figures: (code, report bytes, moves bytes or None, stats).  repeat: every entry is given
    twice, split in two, to be added up by text."""
    texts = list(fig)
    pos = {t: i for i, t in enumerate(texts)}
    ent = []
    for t in texts:
        r = fig[t]
        five = [r[k] for k in ("same", "only_a", "only_b", "left", "arrived")]
        ent.append((t, five))
    if repeat:
        ent = [(t, [v // 2 for v in f]) for t, f in ent] + [(t, [v - v // 2 for v in f]) for t, f in ent]
    keep = [C.create_string_buffer(t, len(t) + 1) for t, _ in ent]
    E = (lib.CompareEntry * max(len(ent), 1))()
    for i, (t, f) in enumerate(ent):
        E[i].text, E[i].len = C.cast(keep[i], C.c_char_p), len(t)
        E[i].same, E[i].only_a, E[i].only_b, E[i].left, E[i].arrived = f
    mv = list(moves.items())
    Mv = (lib.CompareMove * max(len(mv), 1))()
    for i, ((f, t), n) in enumerate(mv):
        Mv[i].from_, Mv[i].to, Mv[i].kmers = pos[f], pos[t] + (len(texts) if repeat else 0), n
    ins = [lib.CompareInput(path=d[0].encode(), is_ctr=int(d[1] == ".ctr"), W=d[2], I=d[3]) for d in (a_desc, b_desc)]
    rep, mov = str(tmp_path / "report.tsv"), str(tmp_path / "moves.tsv")
    st = lib.CompareStats()
    code = lib.load().utree_compare_write(C.byref(ins[0]), C.byref(ins[1]), E, len(ent), Mv, len(mv), rep.encode(),
                                          mov.encode() if with_moves else None, C.byref(st))
    read = lambda p: open(p, "rb").read() if os.path.exists(p) else None
    return code, read(rep), read(mov), st


def agree(tmp_path, a, b, **kw):
    fig, moves, st = R.compare(a, b)
    R.check_invariants(fig, moves, st)
    want_rep, want_mov = R.files(fig, moves, st, A_DESC, B_DESC)
    code, rep, mov, got = write(tmp_path, fig, moves, **kw)
    assert code == lib.OK and rep == want_rep and mov == want_mov
    assert {k: getattr(got, k) for k in st} == st and got.n_passes == 0
    return fig, moves, st, rep, mov


G = M.G
SP_A, SP_B = G + b";s__a", G + b";s__b"
ODD = b"k__\xc3\x84 \xff;p__two words;c__x"                         # bytes above 0x7F and spaces


def test_writer_matches_the_definition_on_hand_made_databases(tmp_path):
    a = M.Db(8, 2, [(1, SP_A), (2, SP_A), (3, SP_B), (4, G), (5, G), (6, ODD), (7, ODD), (8, b"k__Z"), (9, SP_A), (10, b"k__A;p__Bx")])
    b = M.Db(8, 4, [(1, G), (2, SP_A), (3, SP_A), (4, SP_B), (5, G), (6, ODD + b";o__deep"), (8, b"k__Y"), (9, G), (11, ODD), (12, b"k__A")])
    fig, moves, st, rep, mov = agree(tmp_path, a, b)
    kinds = {(f, t): R.kind(f, t) for f, t in moves}
    assert set(kinds.values()) == {"lifted", "lowered", "moved"} and moves[(SP_A, G)] == 2
    assert kinds[(SP_A, G)] == "lifted" and kinds[(G, SP_B)] == "lowered" and kinds[(SP_B, SP_A)] == "moved" and kinds[(b"k__Z", b"k__Y")] == "moved"
    lines = rep.split(b"\n")
    assert lines[0] == b"# a\told dir/a.ubt\t.ubt\t8\t2\t10\t6" and lines[1] == b"# b\tnew/b.ctr\t.ctr\t8\t4\t10\t7"
    assert lines[2] == b"# words\t12\tboth\t8\tsame\t2\tchanged\t6\tonly_a\t2\tonly_b\t2"
    rows = {l.split(b"\t")[0]: [int(v) for v in l.split(b"\t")[1:]] for l in lines[4:-1]}
    assert [l.split(b"\t")[0] for l in lines[4:-1]] == sorted(rows), "rows in bytewise order"
    assert rows[b"k__A;p__B"] == [0, 0, 0, 0, 0, 0, 0, 6, 6], "a pure prefix: zero own figures; k__A;p__Bx is not in its clade"
    assert rows[G][:2] == [2, 3] and rows[G][7:] == [6, 6], "a text that is a label and a prefix of others"
    assert rows[b"k__A"] == [0, 1, 0, 0, 1, 0, 0, 7, 7]
    assert rows[ODD][:2] == [2, 1] and rows[b"k__\xc3\x84 \xff;p__two words"][7:] == [2, 2]
    assert mov.split(b"\n")[0] == b"# from\tto\tkmers\tkind"
    # entries of equal text are added up, and so are their moves; no moves file when none is asked for
    code, rep2, mov2, _ = write(tmp_path, fig, moves, repeat=True)
    assert code == lib.OK and (rep2, mov2) == (rep, mov)
    os.unlink(str(tmp_path / "moves.tsv"))
    code, rep3, mov3, _ = write(tmp_path, fig, moves, with_moves=False)
    assert code == lib.OK and rep3 == rep and mov3 is None


def test_writer_identical_databases_and_no_moves(tmp_path):
    a = M.Db(8, 2, [(1, SP_A), (2, SP_B), (3, ODD)])
    fig, moves, st, rep, mov = agree(tmp_path, a, M.Db(8, 4, list(a.nodes)))
    assert st["identical"] == 1 and moves == {} and mov == b"# from\tto\tkmers\tkind\n"
    fig, moves, st, rep, mov = agree(tmp_path, a, M.Db(8, 2, a.nodes[:2] + [(9, ODD)]))       # words differ, no label changed: still no move
    assert st["identical"] == 0 and mov == b"# from\tto\tkmers\tkind\n" and (st["only_a"], st["only_b"]) == (1, 1)
    empty = M.Db(8, 2, [])
    fig, moves, st, rep, mov = agree(tmp_path, empty, empty)
    assert st["identical"] == 1 and rep.count(b"\n") == 4
    agree(tmp_path, a, empty)


def test_writer_refuses_figures_that_do_not_add_up(tmp_path):
    a = M.Db(8, 2, [(1, SP_A), (2, SP_A), (3, SP_B)])
    b = M.Db(8, 2, [(1, G), (2, SP_B), (3, SP_B)])
    fig, moves, st = R.compare(a, b)
    for broken in ({(SP_A, G): 2}, {(SP_A, G): 1}, {**moves, (SP_B, G): 1}, {(SP_A, G): 1, (SP_A, SP_A): 1}):
        code, rep, mov, _ = write(tmp_path, fig, broken)
        assert code == lib.E_ARG and rep is None and mov is None
    L = lib.load()
    ins = lib.CompareInput(path=b"x", W=8, I=2)
    assert L.utree_compare_write(None, C.byref(ins), None, 0, None, 0, b"r", None, None) == lib.E_ARG
    assert L.utree_compare_write(C.byref(ins), C.byref(ins), None, 0, None, 0, None, None, None) == lib.E_ARG
    assert L.utree_compare_write(C.byref(ins), C.byref(ins), None, 1, None, 0, str(tmp_path / "r").encode(), None, None) == lib.E_ARG
    assert not os.path.exists(str(tmp_path / "r"))
    code, rep, mov, _ = write(tmp_path / "no_such_dir", fig, moves)
    assert code == lib.E_IO and rep is None and mov is None


# ---- 3. the definition's own invariants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.fold_cases()))
def test_invariants_on_the_fold_cases(name, tmp_path):
    inputs, gg = M.fold_cases()[name]
    tree, _, _ = M.fold(inputs, gg)
    merged = M.Db(8, 2, [(w, tree[w]) for w in sorted(tree) if tree[w] is not M.BAD])
    for a, b in [(inputs[0], inputs[1]), (inputs[1], inputs[0])] + [(db, merged) for db in inputs]:
        fig, moves, st = agree(tmp_path, a, b)[:3]
        assert st["a"] == len(a.nodes) and st["b"] == len(b.nodes)
    # against the merge: what an input loses is what the fold dropped as BAD, and the fold only ever lifts
    for db in inputs:
        fig, moves, st = R.compare(db, merged)
        assert st["only_a"] == sum(tree[w] is M.BAD for w, _ in db.nodes)
        assert all(R.kind(f, t) == "lifted" for f, t in moves)
