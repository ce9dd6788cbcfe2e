"""The database merge (include/utree_amd.h: utree_merge_files) restated in plain Python: a dict keyed by word, the builder's insert loop
(xeTreeU / xeTreeU_RF, itree.c:242-307), its label numbering (addSampleU, 593 and 299) and the `.ubt` bytes (UT_writeTreeBinary, 1317-1343).
Also the generator of the IMAGINED build's FASTA and map -- one record of k bases per input node, named i<input>_<node> -- on which the
genuine builder is the yardstick for this file (test_merge_cpu.py pins the two to each other), and small writers for input files.

A database here is a Db: W, I and its nodes [(word, label text as bytes)] in file order (ascending words)."""
from collections import namedtuple

import numpy as np

from utree_amd import ctrfile

Db = namedtuple("Db", "W I nodes")
BAD = None


def shared_semicolons(a: bytes, b: bytes) -> int:
    """';' the two texts have in common before their first difference (itree.c:286-295)"""
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += x == 0x3B
    return n


def cut_before(a: bytes, m: int) -> bytes:
    """a cut before its m-th ';' (m >= 1)"""
    pos = -1
    for _ in range(m):
        pos = a.index(b";", pos + 1)
    return a[:pos]


def step(st, lab: bytes, gg=True):
    """The insert loop's step on a word the tree holds already under st (a label text or BAD), met again under lab.
    Returns (the word's new state, the text the step cut st to -- a label from now on -- or None)."""
    if st is BAD or st == lab:
        return st, None
    if not gg:
        return BAD, None
    m = shared_semicolons(st, lab)
    if m < 2:
        return BAD, None
    st = cut_before(st, m)
    return st, st


def fold(inputs, gg=True):
    """The insert loop over the nodes of the inputs, input by input, each in file order.
    Returns (tree: word -> label text or BAD, labels: text -> index in order of creation, stats)."""
    tree, labels, seen_in = {}, {}, {}
    for db in inputs:
        for w, lab in db.nodes:
            labels.setdefault(lab, len(labels))                  # the record's label exists once the record is parsed
            seen_in.setdefault(w, []).append(lab)
            if w not in tree:
                tree[w] = lab
                continue
            tree[w], cut = step(tree[w], lab, gg)
            if cut is not None:
                labels.setdefault(cut, len(labels))              # a text already present keeps its index
    shared = [w for w, ls in seen_in.items() if len(ls) > 1]
    stats = {"n_in_nodes": sum(len(db.nodes) for db in inputs), "n_shared": len(shared),
             "n_dropped": sum(tree[w] is BAD for w in shared),
             "n_relabelled": sum(tree[w] is not BAD and tree[w] not in seen_in[w] for w in shared),
             "n_nodes": sum(v is not BAD for v in tree.values()), "n_labels": len(labels)}
    return tree, labels, stats


def word_bytes(W: int, w: int) -> bytes:
    return int(w).to_bytes(W, "little")


def ubt_file(W: int, I: int, nodes, labels) -> bytes:
    """header, (W-byte little-endian word, I-byte index) per node, `text \\t nodes carrying it \\n` per label in index order"""
    counts = [0] * len(labels)
    body = bytearray()
    for w, lab in nodes:
        ix = labels[lab]
        counts[ix] += 1
        body += word_bytes(W, w) + ix.to_bytes(I, "little")
    tail = b"".join(t + b"\t%d\n" % counts[i] for t, i in sorted(labels.items(), key=lambda kv: kv[1]))
    return np.array([W, 0, I, len(nodes)], dtype="<u8").tobytes() + bytes(body) + tail


def merge(inputs, gg=True, I=0):
    """(the output file's bytes, stats)"""
    W = inputs[0].W
    assert all(db.W == W for db in inputs)
    I_out = I or max(db.I for db in inputs)
    tree, labels, stats = fold(inputs, gg)
    nodes = [(w, tree[w]) for w in sorted(tree) if tree[w] is not BAD]
    return ubt_file(W, I_out, nodes, labels), stats


def db_file(db: Db, extra_labels=()) -> bytes:
    """A Db as a `.ubt`: labels numbered by first appearance among its nodes, then `extra_labels` (lines no node carries)."""
    labels = {}
    for _, lab in db.nodes:
        labels.setdefault(lab, len(labels))
    for lab in extra_labels:
        labels.setdefault(lab, len(labels))
    return ubt_file(db.W, db.I, db.nodes, labels)


def parse_labels(text: bytes):
    """distinct label texts in order of first appearance (the loader's numbering, itree.c:191-220)"""
    out, seen = [], set()
    for line in text.split(b"\n")[:-1]:
        t = line.split(b"\t", 1)[0]
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def read_ubt(path: str) -> Db:
    W, I, hi, lo, ix, text = ctrfile.read_ubt(path)
    labs = parse_labels(text)
    return Db(W, I, [((int(h) << 64) | int(l), labs[int(i)]) for h, l, i in zip(hi, lo, ix)])


def read_ctr(path: str) -> Db:
    d = ctrfile.read_ctr(path)
    hi, lo = d.words()
    labs = parse_labels(d.label_text)
    return Db(d.W, d.I, [((int(h) << 64) | int(l), labs[int(i)]) for h, l, i in zip(hi, lo, d.ix())])


def imagined(inputs):
    """(FASTA bytes, map bytes) of the imagined build: per input node one record `>i<input>_<node>` of exactly k bases."""
    k = 4 * inputs[0].W
    fa, mp = [], []
    for i, db in enumerate(inputs):
        for j, (w, lab) in enumerate(db.nodes):
            name = b"i%d_%d" % (i, j)
            fa.append(b">" + name + b"\n" + ctrfile.decode_kmer(w >> 64, w & 0xFFFFFFFFFFFFFFFF, k).encode() + b"\n")
            mp.append(name + b"\t" + lab + b"\n")
    return b"".join(fa), b"".join(mp)


def reference_binary(W: int, I: int, gg: bool):
    """name of the genuine builder of oracle/Makefile for (W, I, mode), or None where the reference ships none"""
    name = {(8, 2, True): "utree-buildGG", (8, 2, False): "utree-build", (16, 2, True): "utree-buildGG-k64", (16, 2, False): "utree-build-k64",
            (4, 2, True): "utree-buildGG-k16", (4, 2, False): "utree-build-k16", (8, 4, True): "utree-buildGG-ix32",
            (16, 4, True): "utree-buildGG-k64-ix32"}
    return name.get((W, I, bool(gg)))


# ---------------------------------------------------------------- seeded inputs ----------------------------------------------------------------
def rng(*key):
    return np.random.default_rng([20261019, 77] + [int(k) for k in key])


def random_words(r, W: int, n: int, spread: bool = True):
    """n distinct words of W bytes, ascending.  spread: uniform over the whole range (their top 24 bits differ, so passes can cut between any two)."""
    out = set()
    while len(out) < n:
        v = int.from_bytes(r.bytes(W), "little")
        if not spread:
            v &= (1 << 30) - 1
        out.add(v)
    return sorted(out)


# ---------------------------------------------------------------- the fold, case by case ----------------------------------------------------------------
G = b"k__A;p__B;c__C;o__D;f__F;g__G"
SIBLINGS = (G + b";s__a", G + b";s__b", G + b";s__c")         # a then b: genus G; then c: G against G;s__c shares one ';' less -> family
PFX, PFX_LONG = b"k__A;p__B;c__C", b"k__A;p__B;c__C;o__D"     # the shorter is a prefix of the longer: "k__A;p__B"


def _labels():
    import build_inputs as B
    return {n: getattr(B, n).encode() for n in ("LA", "LB", "LX", "LC", "LD", "LE", "LF")}


def planted(W: int, I: int, label_rows, key, n_fill: int = 40):
    """One input per column of label_rows: row r is a word every input with a label in that row carries (None: the input lacks the word).
    Each input also gets n_fill words of its own under two more labels, so the shared runs sit among unshared nodes."""
    r = rng(W, I, key)
    n_in = len(label_rows[0])
    words = random_words(r, W, len(label_rows) + n_fill * n_in)
    r.shuffle(words)
    sh, own = words[:len(label_rows)], words[len(label_rows):]
    dbs = []
    for i in range(n_in):
        nodes = [(w, row[i]) for w, row in zip(sh, label_rows) if row[i] is not None]
        nodes += [(w, b"k__Own;p__I%d;c__%d" % (i, j % 2)) for j, w in enumerate(own[i * n_fill:(i + 1) * n_fill])]
        dbs.append(Db(W, I, sorted(nodes)))
    return dbs


def fold_cases(W: int = 8, I: int = 2):
    """name -> (inputs, gg)"""
    import itertools
    L = _labels()
    LA, LB, LX, LC, LD, LE, LF = (L[n] for n in ("LA", "LB", "LX", "LC", "LD", "LE", "LF"))
    out = {
        "two_way_cut": (planted(W, I, [(LA, LB), (LE, LF), (LA, LA), (LA, LC)], 1), True),
        "genus_to_family": (planted(W, I, [SIBLINGS, SIBLINGS[:2] + (None,), (SIBLINGS[0], None, SIBLINGS[2])], 2), True),
        "prefix_of_the_other": (planted(W, I, [(PFX, PFX_LONG), (PFX_LONG, PFX)], 3), True),
        "bad_stays_bad": (planted(W, I, [(LA, LD, LB), (LA, LD, LA), (LD, LD, LD)], 4), True),
        "plain_build": (planted(W, I, [(LA, LB), (LA, LA), (LA, None), (LB, LB)], 5), False),
        "all_dropped": ([Db(W, I, [(5, LA), (9, LB)]), Db(W, I, [(5, LD), (9, LD)])], True),
    }
    for perm in itertools.permutations(range(3)):
        trio = (LA, LB, LX)
        out["order_%d%d%d" % perm] = (planted(W, I, [tuple(trio[p] for p in perm), (LA, LB, LC)], 6), True)
    return out
