"""Seeded inputs (numpy only) for the rank-specific search's depth and edge tests, over the committed fixture databases.

What a read's vote picks up from "the latest earlier read with more hits" depends on every read's HIT COUNT, so the
builders here choose database k-mers, and then take each read's hit count from the CPU oracle (RankResult.found) and
assert the layout they need from those -- they do not assume how many hits a sequence keeps.

  depth_case      > 2 * 262 144 reads whose donors lie at every level of the kernels' 64-ary max tree
  vote_split_case reads keeping 62 .. 65 hits (one entry per lane / label histogram) with planted ties
  edge_case       hits at the window-block and LDS-segment edges of rank_hits_k, k = 32 and k = 64
  joint_case      reads around the 'N' that joins a read to its reverse complement
  workspace_case  reads that fill the hit-list entries they reserve
"""
import functools
from collections import namedtuple

import numpy as np

import util
from oracle import orc

BLOCK, GROUP, SUPER = 64, 4096, 262144            # reads per entry of nh's 64-block, lvl[0] and lvl[1] of the max tree
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


Kmers = namedtuple("Kmers", "k asc lab by_label ints")


@functools.lru_cache(maxsize=None)
def oracle_db(name: str) -> orc.OracleDB:
    return orc.OracleDB.load(util.fixture_ctr(name))


@functools.lru_cache(maxsize=None)
def db_kmers(name: str) -> Kmers:
    """The fixture database's k-mers as ASCII rows [n, k], their label indices, the rows of each label, and the set of
    words as Python ints (bin prefix + stored suffix, as test_rank_random_reads_vs_oracle decodes them)."""
    d = util.load_db_fixture(name)
    hi, lo = d.suffixes()
    prefix = (np.searchsorted(d.binix, np.arange(d.n_nodes), side="right") - 1).astype(np.uint64)
    if d.W == 8:
        hi, lo = np.zeros_like(lo), lo | (prefix << np.uint64(40))
    else:
        assert d.W == 16
        hi = hi | (prefix << np.uint64(40))
    sh = (2 * (31 - np.arange(32))).astype(np.uint64)
    asc = ACGT[((lo[:, None] >> sh) & np.uint64(3)).astype(np.intp)]
    if d.W == 16:
        asc = np.concatenate([ACGT[((hi[:, None] >> sh) & np.uint64(3)).astype(np.intp)], asc], axis=1)
    lab = d.ix().astype(np.int64)
    order = np.argsort(lab, kind="stable")
    cuts = np.searchsorted(lab[order], np.arange(int(lab.max()) + 2))
    by_label = [order[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]
    ints = set((int(h) << 64) | int(l) for h, l in zip(hi.tolist(), lo.tolist()))
    # the labels are the oracle's: a sample of the rows looked up in it
    o = oracle_db(name)
    for j in np.random.default_rng(5).integers(0, len(lab), 500).tolist():
        assert o.lookup(int(hi[j]), int(lo[j])) == lab[j], (name, j)
    return Kmers(d.k, asc, lab, by_label, ints)


def pick_rows(km: Kmers, labs, rng) -> np.ndarray:
    """One random k-mer row of each label in `labs`."""
    labs = np.asarray(labs, dtype=np.int64)
    cnt = np.array([len(x) for x in km.by_label], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return np.concatenate(km.by_label)[start[labs] + (rng.random(len(labs)) * cnt[labs]).astype(np.int64)]


def joined(km: Kmers, rows) -> bytes:
    """The k-mers of `rows` joined by 'N': one hit per k-mer and no other (back to back, the word the reference looks up
    at a joint -- built from the hit before it -- can be a database word, and the k-mer after it is then not looked up)."""
    m = np.full((len(rows), km.k + 1), ord("N"), dtype=np.uint8)
    m[:, :km.k] = km.asc[rows]
    return m.tobytes()[:-1]


def fasta(reads) -> bytes:
    return b"".join(b">" + n + b"\n" + s + b"\n" for n, s in reads)


def oracle_records(name: str, data: bytes, rc: bool = False, **prm) -> np.ndarray:
    """orc.RankSearch.read over the file's reads in order, from a fresh state: one RANK_RESULT_DTYPE record per read."""
    off, ln = frame(data)
    rs = orc.RankSearch(oracle_db(name), **prm)
    return rs.read_batch(np.frombuffer(data, dtype=np.uint8), off, ln, rc=rc)


def frame(data: bytes):
    """Offsets and lengths of the sequence lines of a strict two-line FASTA, vectorised."""
    nl = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)
    assert len(nl) % 2 == 0 and data[-1:] == b"\n"
    off = (nl[0::2] + 1).astype(np.uint64)
    return off, (nl[1::2] - nl[0::2] - 1).astype(np.uint32)


def vote(labels, extra):
    """(label, most, second) of a read's own hit labels plus the one entry past them (itree.c:984-997): first-come maximum."""
    seq = list(labels) + [extra]
    cnt = {}
    for v in seq:
        cnt[v] = cnt.get(v, 0) + 1
    most = second = 0
    ix = 0
    for v in seq:
        c = cnt[v]
        cnt[v] = 0
        if c > most:
            second, most, ix = most, c, v
        elif c > second:
            second = c
    return ix, most, second


def prev_greater(nh: np.ndarray) -> np.ndarray:
    """donor[r] = the latest q < r with nh[q] > nh[r] (-1: none), for every read with a hit; monotonic stack."""
    donor = np.full(len(nh), -1, dtype=np.int64)
    v = nh.tolist()
    stack = []                                            # reads whose counts strictly decrease towards the top
    for r in np.flatnonzero(nh > 0).tolist():
        c = v[r]
        while stack and v[stack[-1]] <= c:
            stack.pop()
        if stack:
            donor[r] = stack[-1]
        stack.append(r)
    return donor


def tier_of(r: np.ndarray, donor: np.ndarray) -> np.ndarray:
    """1 same 64-read block, 2 same 4 096-read group, 3 same 262 144-read supergroup, 4 an earlier supergroup, 5 no donor."""
    t = np.full(len(r), 4, dtype=np.int64)
    t[(donor >> 18) == (r >> 18)] = 3
    t[(donor >> 12) == (r >> 12)] = 2
    t[(donor >> 6) == (r >> 6)] = 1
    t[donor < 0] = 5
    return t


def prev_greater_before(nh: np.ndarray, reads: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """The latest q < bound[i] with nh[q] > nh[reads[i]] (-1: none): the candidate a search that skips [bound, r) finds."""
    rich = np.flatnonzero(nh >= 2)                        # only these can exceed a count >= 1
    rc = nh[rich].tolist()
    pos = np.searchsorted(rich, bound, side="left") - 1
    out = np.where(pos >= 0, rich[np.maximum(pos, 0)], -1).astype(np.int64)
    for i in np.flatnonzero(nh[reads] >= 2).tolist():     # a one-hit read takes any of them; the others walk back
        p, n = int(pos[i]), int(nh[reads[i]])
        while p >= 0 and rc[p] <= n:
            p -= 1
        out[i] = rich[p] if p >= 0 else -1
    return out


# ----------------------------------------------------------------------------------------------------------------
DepthCase = namedtuple("DepthCase", "data n seq_off seq_len nk own1 rich records")


def _depth_plan():
    """{read index: k-mers} of the reads with two or more k-mers.  Everything else keeps one hit or none."""
    plan = {}

    def put(p, h):
        assert p not in plan
        plan[p] = h
    stairs = lambda top: list(range(top, 1, -2)) + list(range(3, top, 2))     # descending, then rising between the steps
    p = 320                                               # [0, 320): nothing to pick up -- the carried array
    for h in stairs(42):                                  # 9 reads apart: donors in the same block or the one before
        put(p, h); p += 9
    for i, p in enumerate(range(1000, 5000, 20)):         # dense two-hit reads, a three now and then
        put(p, 3 if i % 10 == 9 else 2)
    cyc = [2, 3, 2, 5, 2, 2, 4, 2, 8, 2, 12]
    for i, p in enumerate(range(5000, 60000, 1500)):      # gaps of several blocks, some across a group's end
        q = p + (i * 37) % 200
        if not 40800 <= q < 41000:
            put(q, cyc[i % len(cyc)])
    for i in range(40):                                   # one block's lanes 24 .. 63 strictly descending 42 .. 3, the last
        put(10 * GROUP - BLOCK + 24 + i, 42 - i)          # block of its group: rank_state_k hands each its own index range
    # [60 000, 262 144): nothing with two hits -- donors in another group of the supergroup
    put(SUPER, 41)                                        # first read of supergroup 1: its donor (42) is in supergroup 0
    p = SUPER + 5000
    for h in stairs(40):                                  # 70 apart: donors in other blocks and groups
        put(p, h); p += 70
    for i, p in enumerate(range(270000, 400000, 5000)):
        put(p + (i * 211) % 900, cyc[(i + 3) % len(cyc)])
    # [~400 000, 2 * 262 144 + 1 500): nothing with two hits -- the last stretch picks up from supergroup 1
    b = 2 * SUPER
    for p, h in ((1500, 3), (1520, 4), (1540, 6), (1560, 9), (1600, 2), (1700, 5), (2000, 41), (2500, 45), (2560, 43),
                 (4096 + 10, 6), (4096 + 64 + 5, 2)):
        put(b + p, h)                                     # 4 > 3, 6, 9: from supergroup 1; 41: from supergroup 0, past 1; 45: no donor
    for p in range(2100, 4000, 150):
        if b + p not in plan:
            put(b + p, 2)
    return plan


@functools.lru_cache(maxsize=2)
def depth_case(seed: int = 1) -> DepthCase:
    """2 * 262 144 + 4 096 + 64 + 37 reads over `rk`: ~70 % single database k-mers from many labels, ~30 % 8 bp reads
    (no hit), and the sparse reads of _depth_plan (2 .. 45 k-mers joined by 'N').  The entry a read picks up is entry n of its donor,
    so: the reads with several k-mers carry different labels at the same list position, one-hit reads often carry the
    label at position 1 of the nearest or second-nearest such read before them, and a read with n > 1 k-mers often
    repeats its donor's label at position n.  A wrong donor then changes the vote.
    Fields: data (FASTA), n, seq_off / seq_len, nk (k-mers per read == the oracle's hit count, asserted), own1 (label of a
    one-k-mer read, else -1), rich {read: labels of its k-mers}, records (the oracle's, default parameters)."""
    km = db_kmers("rk")
    rng = np.random.default_rng(7000 + seed)
    n = 2 * SUPER + GROUP + BLOCK + 37
    plan = _depth_plan()
    assert max(plan) < n
    n_lab = len(km.by_label)
    o = oracle_db("rk")
    nk = (rng.random(n) >= 0.30).astype(np.int64)
    nk[:5] = 0                                            # a first batch can be zero-hit reads only
    P = np.array(sorted(plan), dtype=np.int64)
    nk[P] = [plan[int(p)] for p in P]
    # ---- the reads with several k-mers, in file order (a donor's labels are drawn before its takers')
    donor = prev_greater(nk)                              # by the plan; the conditions are asserted from the oracle's counts
    rich, rich_seq = {}, {}
    scratch = orc.RankSearch(o)
    last1 = -1
    for p in P.tolist():
        h = plan[p]
        for attempt in range(50):
            labs = rng.integers(0, n_lab, h).tolist()
            if rng.random() < 0.5:                        # repeat the entry this read will pick up
                q = int(donor[p])
                labs[int(rng.integers(0, h))] = rich[q][h] if q >= 0 else 0
            if labs[1] == last1:
                continue
            s = joined(km, pick_rows(km, labs, rng))
            if scratch.read(s).found == h:
                break
        else:
            raise AssertionError("no %d-k-mer read with %d hits" % (h, h))
        rich[p], rich_seq[p], last1 = labs, s, labs[1]
    # ---- one-k-mer reads: label 1 of the nearest / second-nearest read with several k-mers before them, label 0, or any
    ones = np.flatnonzero(nk == 1)
    at1 = np.array([rich[int(p)][1] for p in P], dtype=np.int64)
    j = np.searchsorted(P, ones) - 1
    e1 = np.where(j >= 0, at1[np.maximum(j, 0)], 0)
    e2 = np.where(j >= 1, at1[np.maximum(j - 1, 0)], 0)
    u = rng.random(len(ones))
    lab1 = rng.integers(0, n_lab, len(ones))
    lab1 = np.where(u < 0.25, e1, np.where(u < 0.35, e2, np.where(u < 0.40, 0, lab1)))
    rows1 = pick_rows(km, lab1, rng)
    own1 = np.full(n, -1, dtype=np.int64)
    own1[ones] = lab1
    # ---- the file: ">dNNNNNN\n" + sequence + "\n"
    seq_len = np.where(nk == 0, 8, nk * 33 - 1).astype(np.int64)
    rec_off = np.concatenate([[0], np.cumsum(seq_len + 10)])
    out = np.empty(int(rec_off[-1]), dtype=np.uint8)
    rec_off = rec_off[:-1]
    seq_off = rec_off + 9
    idx = np.arange(n)
    out[rec_off], out[rec_off + 1], out[rec_off + 8], out[seq_off + seq_len] = ord(">"), ord("d"), 10, 10
    for i in range(6):
        out[rec_off + 2 + i] = 48 + (idx // 10 ** (5 - i)) % 10
    zeros = np.flatnonzero(nk == 0)
    out[seq_off[zeros][:, None] + np.arange(8)] = ACGT[rng.integers(0, 4, (len(zeros), 8))]
    for a in range(0, len(ones), 65536):
        sl = slice(a, a + 65536)
        out[seq_off[ones[sl]][:, None] + np.arange(32)] = km.asc[rows1[sl]]
    for p, s in rich_seq.items():
        out[seq_off[p]:seq_off[p] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    seq_off, seq_len = seq_off.astype(np.uint64), seq_len.astype(np.uint32)
    records = orc.RankSearch(o).read_batch(out, seq_off, seq_len)
    assert np.array_equal(records["found"], nk), "a read does not keep one hit per k-mer"
    return DepthCase(out.tobytes(), n, seq_off, seq_len, nk, own1, rich, records)


def depth_labels_at(case: DepthCase, q: np.ndarray, n: np.ndarray) -> np.ndarray:
    """Entry n[i] of read q[i]'s hit list (q < 0: the untouched carried array, label 0)."""
    return np.array([case.rich[int(a)][int(b)] if a >= 0 else 0 for a, b in zip(q.tolist(), n.tolist())], dtype=np.int64)


def depth_outcome(case: DepthCase, reads: np.ndarray, entry: np.ndarray) -> np.ndarray:
    """[len(reads), 4] (label, most, second, printed) under the default parameters if read i picked up entry[i]."""
    out = np.zeros((len(reads), 4), dtype=np.int64)
    a = case.own1[reads]
    same = a == entry
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = a, np.where(same, 2, 1), np.where(same, 0, 1), same
    for i in np.flatnonzero(a < 0).tolist():
        ix, most, second = vote(case.rich[int(reads[i])], int(entry[i]))
        out[i] = (ix, most, second, int(most >= 2 and most >= 2 * second))
    return out


# ----------------------------------------------------------------------------------------------------------------
SplitCase = namedtuple("SplitCase", "data n targets")


@functools.lru_cache(maxsize=2)
def vote_split_case(seed: int = 1, repeats: int = 23) -> SplitCase:
    """Pairs (donor, target) of reads of k-mers joined by 'N' over `rk`: the target keeps n = 62, 63, 64 or 65 hits -- 63 is the last count voted with one
    entry per lane -- in one of five label mixes, and the donor before it keeps n + 1 hits or about twice as many, with
    entry n = A, B, C or a label the target does not carry:
      A = B on top (the entry breaks the tie either way, or leaves it), A one ahead of B (the entry makes the tie),
      B = C as runners-up, B one ahead of C, and A exactly twice B (the SLACK = 2 limit).
    160 reads per repeat, 100 of them voted through the label histogram.  targets: read indices of the targets."""
    km = db_kmers("rk")
    rng = np.random.default_rng(8000 + seed)
    n_lab = len(km.by_label)
    mixes = [(20, 20, 10), (20, 19, 10), (30, 10, 10), (30, 10, 9), (24, 12, 6)]

    read_of = lambda labs: joined(km, pick_rows(km, labs, rng))
    reads, targets = [], []
    for rep in range(repeats):
        for n in (62, 63, 64, 65):
            for mi, (ca, cb, cc) in enumerate(mixes):
                for which in range(4):
                    ls = rng.permutation(n_lab)[:12].tolist()
                    A, B, Cc, X = ls[:4]
                    fill = [ls[4 + i % 8] for i in range(n - ca - cb - cc)]        # at most 3 of each
                    if (rep + mi + which) % 2:
                        body = [A] * (ca - 1) + [B] * (cb - 1) + [Cc] * (cc - 1) + fill
                        tl = [A, B, Cc] + [body[i] for i in rng.permutation(len(body))]
                    else:                                                           # B and C first appear past entry 32
                        tl = [A] * ca + fill + [B] * cb + [Cc] * cc
                    assert len(tl) == n
                    dn = n + 1 if (rep + which) % 3 else 2 * n + int(rng.integers(0, 9))
                    dl = rng.integers(0, n_lab, dn).tolist()
                    dl[n] = (A, B, Cc, X)[which]
                    reads.append((b"s%d_%d_%d_%dd" % (rep, n, mi, which), read_of(dl)))
                    targets.append(len(reads))
                    reads.append((b"s%d_%d_%d_%dt" % (rep, n, mi, which), read_of(tl)))
    return SplitCase(fasta(reads), len(reads), np.array(targets, dtype=np.int64))


# ----------------------------------------------------------------------------------------------------------------
EdgeCase = namedtuple("EdgeCase", "data n fwd rc planted")


def _chain(km: Kmers, rng, length: int) -> bytes:
    """`length` bases every window of which is a database k-mer (the databases hold overlapping windows of references)."""
    k = km.k
    mask = (1 << (2 * k)) - 1
    for attempt in range(2000):
        row = int(rng.integers(0, len(km.asc)))
        s = bytearray(km.asc[row].tobytes())
        w = 0
        for c in s:
            w = (w << 2) | b"ACGT".index(c)
        while len(s) < length:
            nxt = [x for x in range(4) if (((w << 2) | x) & mask) in km.ints]
            if not nxt:
                break
            x = nxt[int(rng.integers(0, len(nxt)))]
            w = ((w << 2) | x) & mask
            s.append(b"ACGT"[x])
        if len(s) == length and len(set(s)) > 2:
            return bytes(s)
    raise AssertionError("no run of %d database windows" % (length - k + 1))


def _register_pairs(km: Kmers, S: int):
    """(w0 row, d, g row): database word g is what the reference's register holds d bases after a hit on w0 -- w0's
    last k-d-S+1 bases, S-1 'A's, then d new bases (oracle/utree_oracle.c rank_hits); k = 32."""
    assert km.k == 32
    code = np.zeros(256, dtype=np.uint64)
    code[list(b"ACGT")] = np.arange(4, dtype=np.uint64)
    words = np.zeros(len(km.asc), dtype=np.uint64)
    for i in range(32):
        words = (words << np.uint64(2)) | code[km.asc[:, i]]
    out = []
    for d in range(S, 32 - S + 1):                        # keep >= 1 base of w0
        keep = 32 - d - (S - 1)
        key_g = words >> np.uint64(2 * d)                 # g's first k-d bases
        key_w = (words & np.uint64((1 << (2 * keep)) - 1)) << np.uint64(2 * (S - 1))
        srt = np.argsort(key_g, kind="stable")
        pos = np.searchsorted(key_g[srt], key_w)
        ok = (pos < len(srt)) & (key_g[srt[np.minimum(pos, len(srt) - 1)]] == key_w)
        for w0 in np.flatnonzero(ok).tolist():
            g = int(srt[pos[w0]])
            if g != w0 and len(set(km.asc[w0].tolist())) > 2:
                out.append((w0, d, g))
    return out


def _overlap_pairs(km: Kmers, S: int, per: int = 4):
    """(row 1, d, row 2): database k-mer 2 starts d bases after database k-mer 1 and agrees with it where they overlap,
    S <= d < k."""
    k = km.k
    out = []
    for d in range(S, k):
        void = np.dtype((np.void, k - d))
        suf = np.ascontiguousarray(km.asc[:, d:]).view(void).ravel()
        pre = np.ascontiguousarray(km.asc[:, :k - d]).view(void).ravel()
        _, i, j = np.intersect1d(suf, pre, return_indices=True)
        keep = np.flatnonzero(i != j)[:per]
        out += [(int(i[t]), d, int(j[t])) for t in keep]
    return out


def found_of_prefixes(name: str, seq: bytes, lens) -> list:
    """The oracle's hit count (forward run) of seq[:n] for every n in lens.  Hits are kept left to right, so the hits of a
    prefix are the read's hits that end inside it: the difference between two prefixes counts the hits between them."""
    lens = np.asarray(lens, dtype=np.uint32)
    rs = orc.RankSearch(oracle_db(name))
    return rs.read_batch(np.frombuffer(seq, dtype=np.uint8), np.zeros(len(lens), dtype=np.uint64), lens)["found"].astype(int).tolist()


def planted_ok(name: str, seq: bytes, k: int, w: int, second: int, base: int) -> bool:
    """From the oracle: seq (a read, or read + 'N' + reverse complement written out) keeps `base` hits before window w, one
    AT window w, none in the windows up to `second` and one at `second`; second < 0: none from w to the end."""
    if second >= 0:
        return found_of_prefixes(name, seq, [w + k - 1, w + k, second + k - 1, second + k]) == [base, base + 1, base + 1, base + 2]
    return found_of_prefixes(name, seq, [w + k - 1, w + k, len(seq)]) == [base, base + 1, base + 1]


EDGE_STARTS = (63, 64, 959, 960, 961, 1919, 1920)
EDGE_WINDOWS = (959, 960, 961, 1920, 1921)
Planted = namedtuple("Planted", "read rc w kind second base")


@functools.lru_cache(maxsize=4)
def edge_case(name: str, seed: int = 1) -> EdgeCase:
    """Reads over `rk` (k = 32) or `k64` with a hit AT window w = 63, 64, 959, 960, 961, 1 919 or 1 920 and database k-mers
    S .. k-1 windows after it, which the reference does NOT look up as such: what it looks up there is its register word,
    built from the hit.  Three kinds of core, placed at base w:
      0 (rk)  a run of 2k+20 database windows (the database holds every window of its references): the next hit is
              k windows on, none of the database k-mers between is one;
      1 (rk)  the register word d bases after the hit IS a database word: a second hit exactly d windows on, S <= d <= k-S;
      2 (k64) two database k-mers that overlap by k-d bases, S <= d < k, then a third clear of them: the second is no hit.
    Every (w, kind) comes in a read with room for the whole core, and in reads with exactly 959, 960, 961, 1 920 and
    1 921 windows (which cut the core where they end), after a database k-mer at window 0 (of the reverse strand, for the RC run) where there is room.  For the RC
    run the same cores are placed by the windows of read + 'N' + reverse complement -- w >= 959 with room for the core; 63 and
    64 only with kind 1, the reverse strand then being shorter than the other cores -- and in reads with exactly 960 and
    1 920 such windows, where the hit falls in the last one.
    Each read is redrawn until the ORACLE puts its hits there (planted_ok): filler before a core can complete a database
    window by chance.  fwd / rc: indices of the reads laid out for the forward / the RC run; planted: what the oracle was
    asked per read (read, rc, w, kind, second hit's window or -1, hits before w)."""
    km = db_kmers(name)
    k = km.k
    S = k // 4
    rng = np.random.default_rng(9000 + seed + k)
    filler = lambda m: ACGT[rng.integers(0, 4, max(0, m))].tobytes()
    kmer = lambda: km.asc[int(rng.integers(0, len(km.asc)))].tobytes()
    if k == 32:
        kinds, pairs = (0, 1), _register_pairs(km, S)
    else:
        kinds, pairs = (2,), _overlap_pairs(km, S)
    assert len(pairs) >= 20

    def body(w, L, kind, head):
        """(L bases, window of the second hit or -1): [database k-mer at 0] filler, the core at base w, filler."""
        if kind == 0:
            core, second = _chain(km, rng, 3 * k + 19), w + k
        elif kind == 1:
            w0, d, g = pairs[int(rng.integers(0, len(pairs)))]
            core, second = km.asc[w0].tobytes() + km.asc[g].tobytes()[k - d:] + filler(3), w + d
        else:
            a, d, b = pairs[int(rng.integers(0, len(pairs)))]
            core, second = km.asc[a].tobytes() + km.asc[b].tobytes()[k - d:] + filler(8) + kmer(), w + k + d + 8
        pre = (kmer() + filler(w - k)) if head else filler(w)
        return (pre + core + filler(L - w - len(core)))[:L], (second if second + k <= L else -1)
    reads, fwd, rc, planted = [], [], [], []

    def add(tag, w, L, kind, reverse, need_second):
        """A read of L bases with the core at window w of the read (forward) or of read + N + revcomp; False if none fits."""
        p = w - (L + 1) if reverse else w
        head = p >= k + 8                                     # at window 0 of the read / of the reverse strand
        for attempt in range(300):
            s, second = body(p, L, kind, head)
            if need_second and second < 0:
                continue
            if reverse:
                s, second = revcomp(s), (second + L + 1 if second >= 0 else -1)
            whole = s + b"N" + revcomp(s) if reverse else s
            if planted_ok(name, whole, k, w, second, int(head)):
                (rc if reverse else fwd).append(len(reads))
                planted.append(Planted(len(reads), reverse, w, kind, second, int(head)))
                reads.append((tag, s))
                return True
        return False
    for w in EDGE_STARTS:
        for kind in kinds:
            assert add(b"f%d_room_%d" % (w, kind), w, w + 4 * k + 60, kind, False, True)
            for nwin in EDGE_WINDOWS:
                if nwin > w:
                    assert add(b"f%d_%d_%d" % (w, nwin, kind), w, nwin + k - 1, kind, False, False)
            L = w - 1 - (0 if w < 959 else 80)               # the reverse strand starts at window L + 1
            if L >= k:
                add(b"r%d_room_%d" % (w, kind), w, L, kind, True, True)
            for nwin in (960, 1920):                         # windows of read + N + revcomp: 2L + 2 - k
                L = (nwin + k - 2) // 2
                if 0 <= w - (L + 1) <= L - k:
                    assert add(b"r%d_%d_%d" % (w, nwin, kind), w, L, kind, True, False)
    return EdgeCase(fasta(reads), len(reads), np.array(fwd), np.array(rc), planted)


JointCase = namedtuple("JointCase", "data n short last_fwd first_rev")


@functools.lru_cache(maxsize=4)
def joint_case(name: str, seed: int = 1) -> JointCase:
    """Reads around the 'N' between a read and its reverse complement: runs of database windows of k-1, k and k+1 bases,
    every length L < k with 2L+1 >= k (each window of read + N + revcomp holds the N: no hit), and reads of k .. 150 bases
    that end in a database k-mer (a hit in the last forward window) or in the reverse complement of one (a hit in the
    first reverse window), or begin with one.  short / last_fwd / first_rev: indices of those reads."""
    km = db_kmers(name)
    k = km.k
    rng = np.random.default_rng(9500 + seed + k)
    filler = lambda m: ACGT[rng.integers(0, 4, m)].tobytes()
    kmer = lambda: km.asc[int(rng.integers(0, len(km.asc)))].tobytes()
    reads, short, last_fwd, first_rev = [], [], [], []
    for L in (k - 1, k, k + 1):
        for rep in range(3):
            s = (_chain(km, rng, k + 1) if k == 32 else kmer() + filler(1))[:L]     # k64 holds no two adjacent windows
            if L < k:
                short.append(len(reads))
            reads.append((b"c%d_%d" % (L, rep), s))
            reads.append((b"cr%d_%d" % (L, rep), revcomp(s)))
            if L < k:
                short.append(len(reads) - 1)
    for L in range(k // 2, k):                            # 2L + 1 >= k > L
        short.append(len(reads))
        reads.append((b"h%d" % L, kmer()[:L]))
    for L in (k, k + 1, k + 7, 100, 150):
        if L < k:
            continue
        last_fwd.append(len(reads)); reads.append((b"lf%d" % L, filler(L - k) + kmer()))
        first_rev.append(len(reads)); reads.append((b"fr%d" % L, filler(L - k) + revcomp(kmer())))
        reads.append((b"ff%d" % L, kmer() + filler(L - k)))
        reads.append((b"lr%d" % L, revcomp(kmer()) + filler(L - k)))
    return JointCase(fasta(reads), len(reads), np.array(short), np.array(last_fwd), np.array(first_rev))


# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def workspace_case(mixed: bool, seed: int = 1, n: int = 1200) -> bytes:
    """Reads over `rk` that reserve 511 hit-list entries at the default step of 8 windows (4 088 windows; mixed: also 512
    and 513 entries, 4 096 and 4 097 windows), alternately all 'A' -- "A" * 32 is a database word and so is the register
    word after a hit on it, so the read hits every 8th window and fills its reservation to the last entry -- and database
    k-mers back to back (one hit per k-mer)."""
    km = db_kmers("rk")
    assert 0 in km.ints                                   # "A" * 32
    rng = np.random.default_rng(9900 + seed + int(mixed))
    reads = []
    for i in range(n):
        nwin = (4088, 4096, 4097)[i % 3] if mixed else 4088
        L = nwin + 31
        if i % 2 == 0:
            s = b"A" * L
        else:
            s = (km.asc[rng.integers(0, len(km.asc), L // 32 + 1)].tobytes())[:L]
        reads.append((b"w%d" % i, s))
    return fasta(reads)
