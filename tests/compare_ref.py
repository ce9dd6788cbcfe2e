"""The database compare (include/utree_amd.h: utree_compare_files) restated in plain Python: dicts over the nodes of two merge_ref.Db.
compare(a, b) gives the seven figures per label text, the moves with their kinds and the totals; files(...) the exact bytes of the report
and of the moves file."""
import merge_ref as M

FIGURES = ("a", "b", "same", "only_a", "only_b", "left", "arrived")


def compare(a: M.Db, b: M.Db):
    """(fig: text -> {figure: words}, moves: (from, to) -> words, stats)"""
    da, db = dict(a.nodes), dict(b.nodes)
    fig, moves = {}, {}
    row = lambda t: fig.setdefault(t, dict.fromkeys(FIGURES, 0))
    for w, t in da.items():
        row(t)["a"] += 1
        if w not in db:
            row(t)["only_a"] += 1
        elif db[w] == t:
            row(t)["same"] += 1
        else:
            row(t)["left"] += 1
            row(db[w])["arrived"] += 1
            moves[(t, db[w])] = moves.get((t, db[w]), 0) + 1
    for w, t in db.items():
        row(t)["b"] += 1
        if w not in da:
            row(t)["only_b"] += 1
    st = {k: sum(r[k] for r in fig.values()) for k in FIGURES}
    st["both"] = st["same"] + st["left"]
    st["words"] = len(set(da) | set(db))
    st["a_labels"], st["b_labels"] = len(set(da.values())), len(set(db.values()))
    st["n_moves"] = len(moves)
    st["W"] = a.W
    st["identical"] = int(st["left"] == st["only_a"] == st["only_b"] == 0)
    return fig, moves, st


def kind(frm: bytes, to: bytes) -> str:
    return "lifted" if frm.startswith(to + b";") else "lowered" if to.startswith(frm + b";") else "moved"


def in_clade(p: bytes, t: bytes) -> bool:
    return t == p or t.startswith(p + b";")


def files(fig, moves, st, a_desc, b_desc):
    """(report bytes, moves bytes).  a_desc, b_desc: (path, '.ubt' | '.ctr', W, I) as the `# a` / `# b` lines name the inputs."""
    out = []
    for tag, (path, layout, W, I), n, labels in ((b"a", a_desc, st["a"], st["a_labels"]), (b"b", b_desc, st["b"], st["b_labels"])):
        out.append(b"# %s\t%s\t%s\t%d\t%d\t%d\t%d\n" % (tag, path.encode(), layout.encode(), W, I, n, labels))
    out.append(b"# words\t%d\tboth\t%d\tsame\t%d\tchanged\t%d\tonly_a\t%d\tonly_b\t%d\n"
               % (st["words"], st["both"], st["same"], st["left"], st["only_a"], st["only_b"]))
    out.append(b"# taxon\ta\tb\tsame\tonly_a\tonly_b\tleft\tarrived\tclade_a\tclade_b\n")
    texts = [t for t, r in fig.items() if r["a"] + r["b"]]
    rows = set(texts)
    for t in texts:
        rows.update(t[:i] for i, c in enumerate(t) if c == 0x3B)
    zero = dict.fromkeys(FIGURES, 0)
    for t in sorted(rows):                                       # bytes sort bytewise, the shorter first on a tie
        r = fig.get(t, zero)
        clade = [sum(fig[x][k] for x in texts if in_clade(t, x)) for k in ("a", "b")]
        out.append(t + b"".join(b"\t%d" % v for v in [r[k] for k in FIGURES] + clade) + b"\n")
    mv = [b"# from\tto\tkmers\tkind\n"]
    for (frm, to), n in sorted(moves.items()):
        mv.append(frm + b"\t" + to + b"\t%d\t" % n + kind(frm, to).encode() + b"\n")
    return b"".join(out), b"".join(mv)


def check_invariants(fig, moves, st):
    """the three row invariants and the move sums"""
    for t, r in fig.items():
        assert r["a"] == r["same"] + r["only_a"] + r["left"], t
        assert r["b"] == r["same"] + r["only_b"] + r["arrived"], t
        assert r["left"] == sum(n for (f, _), n in moves.items() if f == t), t
        assert r["arrived"] == sum(n for (_, to), n in moves.items() if to == t), t
    assert st["left"] == st["arrived"] == sum(moves.values())
    assert st["words"] == st["both"] + st["only_a"] + st["only_b"]
    assert all(f != t for f, t in moves)
