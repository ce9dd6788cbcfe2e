"""merge_ref.merge restated on numpy arrays, for inputs too large for a dict of Python ints (test_merge_scale_cpu.py pins the two to each
other byte for byte).  A database here is an ADb: W, I, its words as two u64 arrays (hi: None unless W = 16), per node the number of its
label text, and the texts; nodes in file order (ascending words).

The restatement: the inputs end to end, a stable sort by word -- equal words stay in input order -- and the runs of equal words.  A run of
one record keeps its label.  A run of two or more goes record by record through merge_ref.step, the very step merge_ref.fold takes.  Labels
are numbered by the clock of the event that creates them: the label of record g (g counts the records in input order) at 2g, the text a
step cuts to at 2g + 1; a text made twice keeps its earlier time, and no two events share a time.

Below: the generators of the two production-sized inputs of test_gpu_merge_scale.py, every size a parameter."""
from collections import namedtuple

import numpy as np

import merge_ref as M

ADb = namedtuple("ADb", "W I hi lo lab texts")
NEVER = np.iinfo(np.int64).max


def from_db(db: M.Db) -> ADb:
    """labels numbered by first appearance, as merge_ref.db_file numbers them"""
    texts = {}
    lab = np.array([texts.setdefault(t, len(texts)) for _, t in db.nodes], dtype=np.int64)
    lo = np.array([w & 0xFFFFFFFFFFFFFFFF for w, _ in db.nodes], dtype=np.uint64)
    hi = np.array([w >> 64 for w, _ in db.nodes], dtype=np.uint64) if db.W == 16 else None
    return ADb(db.W, db.I, hi, lo, lab, list(texts))


def records(W: int, I: int, hi, lo, ix):
    """the nodes as the `.ubt` holds them: the W-byte little-endian word, then the I-byte index"""
    word = [("lo", "<u4" if W == 4 else "<u8")] + ([("hi", "<u8")] if W == 16 else [])
    rec = np.empty(len(lo), dtype=np.dtype(word + [("ix", "<u2" if I == 2 else "<u4")]))
    assert rec.dtype.itemsize == W + I
    rec["lo"] = lo
    if W == 16:
        rec["hi"] = hi
    rec["ix"] = ix
    return rec


def ubt_parts(W: int, I: int, hi, lo, ix, texts):
    """(header bytes, record array, label tail bytes): every text gets a line, in index order, with the nodes that carry it"""
    counts = np.bincount(ix, minlength=len(texts))
    tail = b"".join(t + b"\t%d\n" % c for t, c in zip(texts, counts.tolist()))
    return np.array([W, 0, I, len(lo)], dtype="<u8").tobytes(), records(W, I, hi, lo, ix), tail


def write_ubt(path: str, db: ADb):
    head, rec, tail = ubt_parts(db.W, db.I, db.hi, db.lo, db.lab, db.texts)
    with open(path, "wb") as f:
        f.write(head)
        rec.tofile(f)
        f.write(tail)


def merge_parts(inputs, gg=True, I=0):
    """(header bytes, record array, label tail bytes, stats) of the merged `.ubt`"""
    W = inputs[0].W
    assert all(db.W == W for db in inputs)
    I_out = I or max(db.I for db in inputs)
    # one table of texts; tid[g]: the text of record g
    table, tids = {}, []
    for db in inputs:
        own = np.array([table.setdefault(t, len(table)) for t in db.texts], dtype=np.int64)
        tids.append(own[db.lab] if len(db.lab) else np.zeros(0, dtype=np.int64))
    tid = np.concatenate(tids)
    lo = np.concatenate([db.lo for db in inputs])
    hi = np.concatenate([db.hi for db in inputs]) if W == 16 else None
    n = len(lo)
    # a stable sort by word: equal words stay in input order.  Every input ascends, so the sort finds a few long runs to merge; for W = 16
    # it sorts by the high half alone where that already leaves the low halves of every group of equal high halves in order
    order = np.argsort(hi if W == 16 else lo, kind="stable")
    s_lo, s_hi = lo[order], hi[order] if W == 16 else None
    if W == 16 and ((s_hi[1:] == s_hi[:-1]) & (s_lo[1:] < s_lo[:-1])).any():
        order = np.lexsort((lo, hi))
        s_lo, s_hi = lo[order], hi[order]
    head = np.ones(n, dtype=bool)
    if n:
        head[1:] = s_lo[1:] != s_lo[:-1]
        if W == 16:
            head[1:] |= s_hi[1:] != s_hi[:-1]
    start = np.flatnonzero(head)
    length = np.diff(np.append(start, n))
    state = tid[order[start]]                                                         # a run of one record keeps its label
    # the label of record g is created at 2g: the first record that carries a text dates it
    texts = list(table)
    born = np.full(len(texts), NEVER, dtype=np.int64)
    first_tid, first_g = np.unique(tid, return_index=True)
    born[first_tid] = 2 * first_g
    born = born.tolist()
    n_dropped = n_relabelled = 0
    shared = np.flatnonzero(length > 1)
    for r, s, e in zip(shared.tolist(), start[shared].tolist(), (start[shared] + length[shared]).tolist()):
        gs = order[s:e].tolist()
        run = [texts[t] for t in tid[gs].tolist()]
        st = run[0]
        for g, lab in zip(gs[1:], run[1:]):
            st, cut = M.step(st, lab, gg)
            if cut is not None:
                t = table.setdefault(cut, len(table))
                if t == len(texts):
                    texts.append(cut)
                    born.append(NEVER)
                born[t] = min(born[t], 2 * g + 1)                                     # a text already present keeps its index
        if st is M.BAD:
            state[r] = -1
            n_dropped += 1
        else:
            state[r] = table[st]
            n_relabelled += st not in run
    born = np.array(born, dtype=np.int64)
    by_time = np.argsort(born, kind="stable")
    by_time = by_time[born[by_time] != NEVER]
    assert len(set(born[by_time].tolist())) == len(by_time)                           # no two events share a time
    ix_of = np.full(len(texts), -1, dtype=np.int64)
    ix_of[by_time] = np.arange(len(by_time))
    keep = state >= 0
    out_ix = ix_of[state[keep]]
    assert (out_ix >= 0).all()
    stats = {"n_in_nodes": n, "n_shared": len(shared), "n_dropped": n_dropped, "n_relabelled": n_relabelled,
             "n_nodes": int(keep.sum()), "n_labels": len(by_time)}
    return ubt_parts(W, I_out, s_hi[start][keep] if W == 16 else None, s_lo[start][keep], out_ix, [texts[t] for t in by_time.tolist()]) + (stats,)


def merge(inputs, gg=True, I=0):
    """(the output file's bytes, stats), as merge_ref.merge"""
    head, rec, tail, stats = merge_parts(inputs, gg, I)
    return head + rec.tobytes() + tail, stats


# ---------------------------------------------------------------- production-sized inputs ----------------------------------------------------------------
STEM = b"k__A;p__B;c__C;o__D;f__F"


def species(tag: bytes, n: int):
    """n species in n // 4 genera.  Two of different tags never are equal: of one genus they fold to the genus, else to the family STEM"""
    return [STEM + b";g__G%d;s__%s%d" % (i % max(n // 4, 1), tag, i) for i in range(n)]


def own_words(r, a_lo, n, allowed):
    """n ascending words that a_lo lacks: a_lo[i] + 1 at n places i (of the index array `allowed`) where a_lo[i + 1] is further than that"""
    free = allowed[a_lo[allowed + 1] - a_lo[allowed] >= 2]
    return a_lo[np.sort(r.choice(free, n, replace=False))] + np.uint64(1)


def staging_inputs(n_a=13_600_000, n_b=200_000, n_shared=65_536, straddle=13_421_772, n_labels=20, seed=1):
    """(A, B, B's shared words as indices into A, sorted; per shared word whether B gives it A's own label) for W = 16, I = 4.
    A: n_a words whose high halves ascend by random gaps.  B: n_shared of A's words -- A's first and last, and straddle - 2 ... straddle + 2
    among them -- every eighth of them under A's own label, the others under a species of the tag "b"; and n_b - n_shared words of its own."""
    r = np.random.default_rng([20261021, seed])
    hi = np.cumsum(r.integers(2, 1 << 40, n_a, dtype=np.uint64), dtype=np.uint64)
    lo = r.integers(0, (1 << 64) - 1, n_a, dtype=np.uint64, endpoint=True)
    ta, tb = species(b"a", n_labels), species(b"b", n_labels)
    a = ADb(16, 4, hi, lo, r.integers(0, n_labels, n_a), ta)
    must = np.array([0, n_a - 1] + list(range(straddle - 2, straddle + 3)))
    rest = np.setdiff1d(r.choice(n_a, n_shared + len(must), replace=False), must)[:n_shared - len(must)]
    sh = np.sort(np.concatenate([must, rest]))
    assert len(np.unique(sh)) == n_shared
    keeps = np.arange(n_shared) % 8 == 3
    sh_lab = np.where(keeps, a.lab[sh] + n_labels, r.integers(0, n_labels, n_shared))     # B's texts: tb, then ta
    own_hi = own_words(r, hi, n_b - n_shared, np.arange(n_a - 1))
    b_hi = np.concatenate([hi[sh], own_hi])
    b_lo = np.concatenate([lo[sh], r.integers(0, (1 << 64) - 1, len(own_hi), dtype=np.uint64, endpoint=True)])
    b_lab = np.concatenate([sh_lab, r.integers(0, n_labels, len(own_hi))])
    o = np.argsort(b_hi, kind="stable")
    return a, ADb(16, 4, b_hi[o], b_lo[o], b_lab[o], tb + ta), sh, keeps


def output_inputs(n_a=17_000_000, n_b=100_000, n_sib=50_000, n_bad=5_000, around=1 << 24, n_labels=20, seed=2):
    """(A, B, the four of A's words that the merged file holds at nodes around - 2 ... around + 1) for W = 4, I = 2.
    A: n_a words ascending by gaps of 1 ... 250.  B: n_sib of A's words under species of the tag "b" (relabelled), n_bad under a text of
    another kingdom (BAD: dropped), the rest its own.  Where the output holds a word of A follows from counting B's own and BAD words below
    it; the four named words are among the n_sib."""
    r = np.random.default_rng([20261021, seed])
    lo = np.cumsum(r.integers(1, 251, n_a, dtype=np.uint64), dtype=np.uint64)
    assert int(lo[-1]) < 1 << 32
    ta, tb = species(b"a", n_labels), species(b"b", n_labels) + [b"k__Z;p__Y"]
    a = ADb(4, 2, None, lo, r.integers(0, n_labels, n_a), ta)
    own = own_words(r, lo, n_b - n_sib - n_bad, np.arange(n_a - 1))
    pick = r.choice(n_a, n_sib + n_bad, replace=False)
    bad = np.sort(pick[:n_bad])
    # A's node i, unless BAD, stands at output node i + (B's own words below it) - (BAD words below it)
    i = np.setdiff1d(np.arange(max(around - n_b, 0), min(around + n_b, n_a)), bad)
    at = i + np.searchsorted(own, lo[i]) - np.searchsorted(bad, i)
    four = i[(at >= around - 2) & (at <= around + 1)]
    assert len(four) == 4, "one of B's own words stands there: take another seed"
    sib = np.sort(np.concatenate([np.setdiff1d(pick[n_bad:], four)[:n_sib - 4], four]))
    b_lo = np.concatenate([lo[sib], lo[bad], own])
    b_lab = np.concatenate([r.integers(0, n_labels, n_sib), np.full(n_bad, n_labels), r.integers(0, n_labels, len(own))])
    o = np.argsort(b_lo, kind="stable")
    return a, ADb(4, 2, None, b_lo[o], b_lab[o], tb), lo[four]
