"""The database inspection (include/utree_amd.h: utree_inspect_file) restated in plain Python: dicts over the nodes of one merge_ref.Db.
inspect(db) gives the four classes per label text, the pair events per ordered pair of texts and the totals; files(...) the exact bytes of
the report and of the pairs file."""
import merge_ref as M

CLASSES = ("isolated", "same", "lineage", "conflict")
FIGURES = ("kmers",) + CLASSES


def bases(W: int) -> int:
    """k: for W = 4 only the low 32 bits carry the 16-mer"""
    return 16 if W == 4 else 4 * W


def neighbours(W: int, w: int):
    """the 3k words one substitution away from w"""
    return [w ^ (d << (2 * p)) for p in range(bases(W)) for d in (1, 2, 3)]


def ancestor(x: bytes, y: bytes) -> bool:
    """x is an ancestor of y: y begins with x followed by ';' (literally, for the empty text too)"""
    return y.startswith(x + b";")


def one_lineage(x: bytes, y: bytes) -> bool:
    return x == y or ancestor(x, y) or ancestor(y, x)


def inspect(db: M.Db):
    """(fig: text -> {figure: nodes}, pairs: (from, to) -> pair events, stats)"""
    d = dict(db.nodes)
    assert len(d) == len(db.nodes)
    fig, pairs = {}, {}
    for w, t in d.items():
        held = [d[v] for v in neighbours(db.W, w) if v in d]
        for t2 in held:
            if t2 != t:
                pairs[(t, t2)] = pairs.get((t, t2), 0) + 1
        if any(not one_lineage(t, t2) for t2 in held):
            cls = "conflict"
        elif any(t2 != t for t2 in held):
            cls = "lineage"
        else:
            cls = "same" if held else "isolated"
        r = fig.setdefault(t, dict.fromkeys(FIGURES, 0))
        r["kmers"] += 1
        r[cls] += 1
    st = {k: sum(r[k] for r in fig.values()) for k in FIGURES}
    st["pair_events"], st["distinct_pairs"] = sum(pairs.values()), len(pairs)
    st["labels"] = len(fig)
    st["W"], st["I"] = db.W, db.I
    st["clean"] = int(st["conflict"] == 0)
    return fig, pairs, st


def kind(frm: bytes, to: bytes) -> str:
    return "ancestor" if ancestor(to, frm) else "descendant" if ancestor(frm, to) else "conflict"


def in_clade(p: bytes, t: bytes) -> bool:
    return t == p or t.startswith(p + b";")


def files(fig, pairs, st, desc):
    """(report bytes, pairs bytes).  desc: (path, '.ubt' | '.ctr', W, I) as the `# db` line names the input."""
    path, layout, W, I = desc
    out = [b"# db\t%s\t%s\t%d\t%d\t%d\t%d\n" % (path.encode(), layout.encode(), W, I, st["kmers"], st["labels"])]
    out.append(b"# kmers\t%d\tisolated\t%d\tsame\t%d\tlineage\t%d\tconflict\t%d\tpair_events\t%d\tdistinct_pairs\t%d\n"
               % (st["kmers"], st["isolated"], st["same"], st["lineage"], st["conflict"], st["pair_events"], st["distinct_pairs"]))
    out.append(b"# taxon\tkmers\tisolated\tsame\tlineage\tconflict\tclade_kmers\tclade_conflict\n")
    texts = [t for t, r in fig.items() if r["kmers"]]
    rows = set(texts)
    for t in texts:
        rows.update(t[:i] for i, c in enumerate(t) if c == 0x3B)
    zero = dict.fromkeys(FIGURES, 0)
    for t in sorted(rows):                                       # bytes sort bytewise, the shorter first on a tie
        r = fig.get(t, zero)
        clade = [sum(fig[x][k] for x in texts if in_clade(t, x)) for k in ("kmers", "conflict")]
        out.append(t + b"".join(b"\t%d" % v for v in [r[k] for k in FIGURES] + clade) + b"\n")
    pr = [b"# from\tto\tpairs\tkind\n"]
    for (frm, to), n in sorted(pairs.items()):
        pr.append(frm + b"\t" + to + b"\t%d\t" % n + kind(frm, to).encode() + b"\n")
    return b"".join(out), b"".join(pr)


def check_invariants(fig, pairs, st):
    """the row invariant, the column sums, the pair sums and the symmetry of the pairs"""
    for t, r in fig.items():
        assert r["kmers"] == sum(r[c] for c in CLASSES), t
    for k in FIGURES:
        assert st[k] == sum(r[k] for r in fig.values()), k
    assert st["kmers"] == sum(st[c] for c in CLASSES)
    assert st["pair_events"] == sum(pairs.values()) and st["distinct_pairs"] == len(pairs)
    mirror = {"ancestor": "descendant", "descendant": "ancestor", "conflict": "conflict"}
    for (f, t), n in pairs.items():
        assert f != t and n > 0 and pairs.get((t, f)) == n, (f, t)
        assert kind(t, f) == mirror[kind(f, t)], (f, t)
    # a node is a conflict node exactly when it has a pair event of kind conflict, a lineage node when it has only others
    assert (st["conflict"] > 0) == any(kind(f, t) == "conflict" for f, t in pairs)
    assert (st["lineage"] + st["conflict"] > 0) == bool(pairs)


# ---------------------------------------------------------------- planted inputs ----------------------------------------------------------------
def mutate(W: int, w: int, p: int, d: int) -> int:
    return w ^ (d << (2 * p))


def planted(W: int, I: int, n: int, key, labels, share: int = 3):
    """n nodes: random words under random labels, every `share`-th of them followed by a copy mutated at a random base under a random label
    (a random word has no neighbour with near certainty, so every neighbour here is planted)."""
    r = M.rng(W, I, n, key)
    words = {}
    for w in M.random_words(r, W, n):
        if len(words) >= n:
            break
        words[w] = labels[int(r.integers(0, len(labels)))]
        if len(words) % share == 0 and len(words) < n:
            v = mutate(W, w, int(r.integers(0, bases(W))), int(r.integers(1, 4)))
            if v not in words:
                words[v] = labels[int(r.integers(0, len(labels)))]
    return M.Db(W, I, sorted(words.items()))
