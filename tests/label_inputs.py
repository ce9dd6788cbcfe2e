"""Databases by label count, and reads by label rank.

32-bit label indices exist for databases with more than 65 534 labels, and several pieces of the search change at a label count: the lane
pass takes a k = 32 / u32 image only below 2^19 - 1 labels (a tally slot keeps 19 bits of rank), classify_long_k keeps its touched-label
bitmap in LDS up to 65 536 labels and in HBM above, the rank-specific vote's histogram rows are clamped to 512 MiB, the vote table's ids
and the u16 record's rank field end at 0xFFFD for the 65 534 labels u16 indices allow.  build() writes a database of exactly n labels in
which every rank can be hit; reads() plants chosen ranks -- the lowest, the highest, neighbours across a bitmap word, a spread over every
thread's stretch of the bitmap sweep -- into reads of the lengths at which the kernels change.

Rank = position of a label's text in bytewise order (what the image's rank2ix holds).  Everything is seeded numpy; nothing is stored.
"""
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from utree_amd import ctrfile

N_FORMS = 64 * 5 + 37               # five full grabs of the lane pass and a ragged one
N_MANY = 2500                       # more long reads than classify_long_k has workgroups (n_cu * 8 = 2048)
LONG_MIN, LONG_MAX = 2120, 2300     # above UTREE_MID_DEFAULT (2112 staged bases): classify_long_k without the lane pass
EDGE = 64                           # this many of the lowest and of the highest ranks get two extra k-mers

# name: (k, I, labels, seed)
DATABASES = {
    "top19": (32, 4, (1 << 19) - 2, 1901),       # the last count the lane pass takes
    "over19": (32, 4, (1 << 19) - 1, 1902),      # the first it must not take
    "lds": (32, 4, 65536, 1903),                 # nbw = 2048: the long-read bitmap still in LDS
    "hbm": (32, 4, 65537, 1904),                 # nbw = 2049: in HBM
    "hbm64": (64, 4, 65537, 1905),               # the wave-per-read kernels alone, u32 labels
    "max16": (32, 2, 65534, 1906),               # the I = 2 maximum, vote table on
    "max16k64": (64, 2, 65534, 1907),            # lane pass, k = 64
    "max16k16": (16, 2, 65534, 1908),            # direct table, u16 sentinel
}
# the vote table's shape limits: 300 labels of exactly 8 tokens and 200 .. 255 bytes, and the same set with one label of 256 bytes
SHAPE_DATABASES = {"vt255": (32, 2, 300, 1909), "vt256": (32, 2, 300, 1909)}

_SPECIES = ("", ";s__", ";s__S0", ";s__S1", ";s__S1_", ";s__S2", ";s__S10", ";s__x_")


def label_texts(n):
    """n distinct labels of up to seven ranks, eight under each genus: the genus itself (the ancestor of the others), the genus with an empty
    last rank, and six species, two of them with tokens ending in '_' and two that are prefixes of another."""
    out = []
    g = 0
    while len(out) < n:
        head = "k__B;p__P%d;c__C%d;o__O%d;f__F%d;g__G%d" % (g >> 12, (g >> 9) & 7, (g >> 6) & 7, (g >> 3) & 7, g & 7)
        out += [head + s for s in _SPECIES]
        g += 1
    return out[:n]


def shape_label_texts(n, rng, longest):
    """n labels of exactly 8 tokens and 200 .. 255 bytes (so tok_end and len pass 127 and reach 255) in families of four that share their
    first six tokens; `longest` = 256 pads the first label to 256 bytes."""
    out = []
    for i in range(n):
        fam, member = i // 4, i % 4
        toks = ["k__B", "p__P%d" % (fam % 3), "c__" + "c" * 60 + "%d" % (fam % 5), "o__" + "o" * 50 + "%d" % fam, "f__F%d_" % (fam % 2),
                "g__G%d" % fam, "s__S%d" % (member // 2), "t__T%d" % member if member != 3 else "t__"]
        s = ";".join(toks)
        want = 255 if i % 7 == 0 else int(rng.integers(200, 256))
        pad = want - len(s)
        assert pad >= 0
        toks[3] = toks[3] + "x" * pad                         # (the padding sits in the fourth token: the later tokens end beyond byte 127)
        out.append(";".join(toks))
    if longest == 256:
        toks = out[0].split(";")
        toks[3] += "x"
        out[0] = ";".join(toks)
    assert len(set(out)) == n and all(s.count(";") == 7 for s in out)
    assert max(len(s) for s in out) == longest and min(len(s) for s in out) >= 200
    return out


@dataclass
class Built:
    name: str
    k: int
    I: int
    n: int                          # labels
    ctr: str                        # path of the .ctr
    labels: List[str]               # file order
    by_rank: List[str]              # the same texts in rank order
    rank_of: np.ndarray             # uint32[n]: rank of the label with file index i
    ix_of_rank: np.ndarray          # uint32[n]: file index of the label at rank r
    hi: np.ndarray                  # uint64[N] words, ascending
    lo: np.ndarray
    ix: np.ndarray                  # uint32[N] label (file index) of every node
    first: np.ndarray               # int64[n]: a node of every label
    by_label: np.ndarray = field(default=None)      # nodes sorted by label, start[l] .. start[l + 1]
    start: np.ndarray = field(default=None)
    edge: Dict[int, int] = field(default_factory=dict)     # rank 0, 1, n-2, n-1 -> the label's file index

    def nodes_of_rank(self, r):
        l = int(self.ix_of_rank[r])
        return self.by_label[self.start[l]:self.start[l + 1]]

    def kmer_of_rank(self, r, which=0):
        nd = self.nodes_of_rank(r)
        j = int(nd[which % len(nd)])
        return ctrfile.decode_kmer(int(self.hi[j]), int(self.lo[j]), self.k)

    @property
    def nbw(self):
        return (self.n + 31) >> 5

    @property
    def sweep_per(self):
        """Bitmap words each of classify_long_k's 256 threads sweeps."""
        return (self.nbw + 255) // 256


def _distinct_words(rng, n, k):
    """n distinct random k-mers as (hi, lo), unsorted."""
    def draw(m):
        lo = rng.integers(0, 1 << 63, m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, m, dtype=np.uint64)
        hi = rng.integers(0, 1 << 63, m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, m, dtype=np.uint64)
        if k == 16:
            lo &= np.uint64(0xFFFFFFFF)
        if k != 64:
            hi[:] = 0
        return hi, lo
    hi, lo = draw(n)
    for _ in range(100):
        o = np.lexsort((lo, hi))
        dup = np.zeros(n, bool)
        dup[o[1:]] = (hi[o][1:] == hi[o][:-1]) & (lo[o][1:] == lo[o][:-1])
        if not dup.any():
            return hi, lo
        hi[dup], lo[dup] = draw(int(dup.sum()))
    raise AssertionError("k-mers could not be drawn")


def build(k, I, n_labels, seed, tmp, name=None, texts=None):
    """A .ctr (ctrfile.write_ctr) of n_labels labels: one random k-mer per label, 20 000 more on random labels, two more for each of the 64
    lowest and the 64 highest ranks; no word twice, every bin regular.  File order of the labels is a seeded permutation of rank order."""
    rng = np.random.default_rng(seed)
    n = n_labels
    texts = label_texts(n) if texts is None else texts
    assert len(set(texts)) == n
    by_rank = sorted(texts, key=lambda s: s.encode("latin-1"))
    ix_of_rank = rng.permutation(n).astype(np.uint32)         # rank r sits at file index ix_of_rank[r]
    rank_of = np.empty(n, np.uint32)
    rank_of[ix_of_rank] = np.arange(n, dtype=np.uint32)
    labels = [by_rank[int(r)] for r in rank_of]
    e = min(EDGE, n // 2)
    ix = np.concatenate([np.arange(n, dtype=np.uint32), rng.integers(0, n, 20000).astype(np.uint32),
                         np.repeat(ix_of_rank[:e], 2), np.repeat(ix_of_rank[n - e:], 2)])
    hi, lo = _distinct_words(rng, len(ix), k)
    o = np.lexsort((lo, hi))
    hi, lo, ix = hi[o], lo[o], ix[o]
    ctr = str(tmp / ("%s.ctr" % (name or "labels_%d_%d_%d" % (k, I, n))))
    ctrfile.write_ctr(ctr, k // 4, I, hi, lo, ix, labels)
    by_label = np.argsort(ix, kind="stable")
    start = np.searchsorted(ix[by_label], np.arange(n + 1))
    b = Built(name or "", k, I, n, ctr, labels, by_rank, rank_of, ix_of_rank, hi, lo, ix, by_label[start[:-1]], by_label, start)
    b.edge = {r: int(ix_of_rank[r]) for r in (0, 1, n - 2, n - 1)}
    return b


def build_named(name, tmp):
    if name in SHAPE_DATABASES:
        k, I, n, seed = SHAPE_DATABASES[name]
        texts = shape_label_texts(n, np.random.default_rng(seed), 255 if name == "vt255" else 256)
        return build(k, I, n, seed, tmp, name, texts)
    k, I, n, seed = DATABASES[name]
    return build(k, I, n, seed, tmp, name)


# ---- reads ----------------------------------------------------------------------------------------------------------------------------
def _rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def _joined(built, picks, sep="N"):
    """picks: [(rank, count)]: every label's k-mers (its `count` first ones, round again where it has fewer) in the order given."""
    return sep.join(built.kmer_of_rank(r, j) for r, c in picks for j in range(c))


def _padded(rng, s, L):
    """s somewhere inside L bases (as it is where it is longer), random bases around it, an N on each side that has some."""
    room = L - len(s) - 2
    if room < 0:
        return s
    front = int(rng.integers(0, room + 1))
    return _rnd(rng, front) + "N" + s + "N" + _rnd(rng, room - front)


def form_sets(built, seed):
    """N_FORMS label sets [(rank, count)], in file order of the reads: 0 .. 5 distinct labels each, counts 1 .. 3.  Of the reads of 2, 3 and 4
    labels every third has one of the four highest ranks as its highest label, every third one of the four lowest ranks among its labels
    (every sixth: nothing but the lowest four, so one of them is its highest too); the other reads of two labels are a leaf with its own
    ancestor, or two siblings."""
    rng = np.random.default_rng(seed)
    n, k = built.n, built.k
    budget = {16: 150, 32: 150}.get(k)                      # k = 16 and 32: a read fits one lane; k = 64: as long as it gets
    rank_text = built.by_rank
    pos = {s: r for r, s in enumerate(rank_text)}

    def related(j):
        """a leaf with its own ancestor (even j) or with a sibling (odd j): the texts decide; a label set without ancestors: siblings alone"""
        for tries in range(1000):
            a = int(rng.integers(0, n))
            head = rank_text[a].rsplit(";", 1)[0]
            sib = [r for r in range(max(0, a - 8), min(n, a + 9)) if r != a and rank_text[r].startswith(head + ";")]
            if not rank_text[a].endswith("__") and sib and (head in pos or j % 2 or tries >= 200):
                break
        other = pos[head] if j % 2 == 0 and head in pos else sib[j % len(sib)]
        return [(a, 1 + (j // 2) % 2), (other, 1 + (j // 4) % 2)]

    sets = []
    for i in range(N_FORMS):
        nl = i % 6
        kind = (i // 6) % 6
        if nl == 0:
            sets.append([])
            continue
        if nl == 2 and kind in (2, 5):                      # the two-label reads that are neither at the top nor at the bottom
            sets.append(related(i // 18))
            continue
        if nl in (2, 3, 4) and kind in (0, 3):              # highest label among the top four
            top = n - 1 - int(rng.integers(0, 4))
            rest = rng.choice(top, nl - 1, replace=False) if kind == 0 else top - 1 - rng.choice(min(6, top), nl - 1, replace=False)
            ranks = [top] + [int(x) for x in rest]
        elif nl in (2, 3, 4) and kind == 1:                 # one of the lowest four among random ones
            ranks = [int(rng.integers(0, 4))] + [int(x) for x in 4 + rng.choice(n - 4, nl - 1, replace=False)]
        elif nl in (2, 3, 4) and kind == 4:                 # nothing but the lowest four
            ranks = [int(x) for x in rng.choice(4, nl, replace=False)]
        else:
            ranks = [int(x) for x in rng.choice(n, nl, replace=False)]
        ranks = [ranks[j] for j in rng.permutation(nl)]
        counts = [int(rng.integers(1, 4)) for _ in ranks]
        if budget:
            while sum(counts) * (k + 1) - 1 > budget and max(counts) > 1:
                counts[int(np.argmax(counts))] -= 1
        sets.append(list(zip(ranks, counts)))
    order = rng.permutation(len(sets))
    return [sets[j] for j in order]


def spread_ranks(n, j, parts=5):
    """60 ranks spread over all of them; j = 0: round(i * (n - 1) / 59); j = 1 .. parts - 1: the same moved on by j / parts of a step."""
    return sorted({min(n - 1, int(round((i + j / parts) * (n - 1) / 59))) for i in range(60)})


def long_sets(built):
    """(tag, [(rank, count)], separator) of the `long` reads."""
    n = built.n
    w = built.sweep_per - 1                                  # the word that ends thread 0's stretch of the sweep
    mid = (n // 2) & ~31
    out = [("r0", [(0, 3)], "N"), ("rtop", [(n - 1, 2)], "N"), ("r0top", [(0, 2), (n - 1, 1)], "N"), ("top_r0", [(n - 1, 3), (0, 1)], "N"),
           ("oneword", [(mid + 3, 1), (mid + 17, 2)], "N"), ("oneword_ends", [(mid, 1), (mid + 31, 1)], "N"),
           ("stretch", [(32 * w + 31, 2), (32 * w + 32, 1)], "N"), ("stretch_up", [(32 * w + 32, 1)], "N"), ("stretch_lo", [(32 * w + 31, 1)], "N")]
    for j in range(5):
        out.append(("spread%d" % j, [(r, 1) for r in spread_ranks(n, j)], "N"))
    return out


def touched_words_cover(built, rank_lists):
    """The condition on the set of `long` reads: the union of their labels' bitmap words reaches every thread's stretch of the sweep (`per` words
    each, the last one shorter), the first and the last word included."""
    words = {r >> 5 for ranks in rank_lists for r in ranks}
    per, nbw = built.sweep_per, built.nbw
    threads = (nbw + per - 1) // per
    return 0 in words and nbw - 1 in words and all(any(x in words for x in range(t * per, min(nbw, (t + 1) * per))) for t in range(threads))


def reads(built, kind, seed):
    """[(name, sequence)].  forms: N_FORMS reads of none to five labels, k-mers joined by N (five labels at k = 32: 160 bases, no N);
    lanes: the same label sets inside 161 .. 289, 1000 .. 1063 and 2000 .. 2095 bases; long: chosen ranks in reads of 2120 .. 2300 bases and
    one of 70 concatenated k-mers; many_long: N_MANY such reads of one to three random labels; singles: 3000 reads of one k-mer of a
    random label, named <sample>_<n> over three samples."""
    rng = np.random.default_rng(seed)
    k, n = built.k, built.n
    if kind in ("forms", "lanes"):
        sets = form_sets(built, seed=built.n % 1000 + built.k)             # the same label sets for both kinds
        out = []
        for i, picks in enumerate(sets):
            if not picks:
                s = _rnd(rng, 100)
            else:
                s = _joined(built, picks)
                if k == 32 and len(picks) == 5:
                    s = _joined(built, [(r, 1) for r, _ in picks], sep="")      # five labels in one lane: 160 bases
            if kind == "lanes":
                lo, hi = ((161, 289), (1000, 1063), (2000, 2095))[i % 3]
                if len(s) + 2 > hi:
                    lo, hi = max(2000, len(s) + 2), max(2095, len(s) + 2)
                s = _padded(rng, s, int(rng.integers(max(lo, len(s) + 2), hi + 1)))
            out.append(("%s%d_%d" % (kind[0], len(picks), i), s))
        return out
    if kind == "long":
        out = [(tag, _padded(rng, _joined(built, picks, sep), int(rng.integers(LONG_MIN, LONG_MAX + 1)))) for tag, picks, sep in long_sets(built)]
        chain = [int(x) for x in rng.choice(n, 70, replace=False)]
        out.append(("chain70", _padded(rng, _joined(built, [(r, 1) for r in chain], ""), LONG_MIN)))
        return out
    if kind == "many_long":
        out = []
        for i in range(N_MANY):
            picks = [(int(r), int(rng.integers(1, 4))) for r in rng.choice(n, 1 + i % 3, replace=False)]
            out.append(("m%d" % i, _padded(rng, _joined(built, picks), int(rng.integers(LONG_MIN, LONG_MAX + 1)))))
        return out
    if kind == "singles":
        return [("smp%d_%d" % (i % 3, i), built.kmer_of_rank(int(r))) for i, r in enumerate(rng.integers(0, n, 3000))]
    raise ValueError(kind)


def fasta(rs):
    return b"".join(b">" + n.encode() + b"\n" + s.encode() + b"\n" for n, s in rs)


READ_SEED = {"forms": 21, "lanes": 22, "long": 23, "many_long": 24, "singles": 25}


def reads_data(built, kind):
    """FASTA bytes of one kind, or of several joined by '+' in that order."""
    return b"".join(fasta(reads(built, part, READ_SEED[part])) for part in kind.split("+"))


# ---- what is searched on which database -------------------------------------------------------------------------------------------------
# database: the kinds the classifying search (xtree-searchGG) runs on it, both strand modes each
SEARCH_RUNS = {
    "top19": ("forms", "lanes", "long", "many_long"),
    "over19": ("forms", "lanes"),
    "lds": ("long",),
    "hbm": ("long", "many_long", "forms+long+singles"),
    "hbm64": ("forms", "long"),
    "max16": ("forms", "long"),
    "max16k64": ("forms", "long"),
    "max16k16": ("forms", "long"),
    "vt255": ("forms",),
    "vt256": ("forms",),
}
# database: the kinds the rank-specific search (xtree-search) runs on it, both strand modes each
RANK_RUNS = {"top19": ("forms+long",), "hbm": ("forms+long",), "max16": ("forms+long",)}


def run_key(name, kind, rc, rank=False):
    return "labels_%s%s_%s%s" % ("rank_" if rank else "", name, kind.replace("+", ""), "_rc" if rc else "")


def reference_binary(k, I, rank=False):
    """The build of the genuine reference (oracle/Makefile: ref) for this record format."""
    return ("xtree-search" if rank else "xtree-searchGG") + {16: "-k16", 32: "", 64: "-k64"}[k] + ("-ix32" if I == 4 else "")
