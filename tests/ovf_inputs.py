"""Databases whose buckets hold an exact, chosen number of k-mers, and a plain-Python model of the overflow area their image must have.

The minimizer hash (csrc/device_common.hpp: mix32 of the canonical 16-mer) is a bijection on 32 bits, so a 16-mer -- the CORE -- can be
chosen for any wanted hash value.  A core with a tiny hash is the minimizer of every k-mer that holds it, wherever it lies, and in a small
database every region of the table has 2^16 slots: slot (pair of buckets) = h >> 8, bucket = 2 * slot + orientation, and the hash's low
eight bits are the top of the record key.  A Spec says how many k-mers hold one (core, orientation) at which position; build() draws the
flanks (seeded), checks every k-mer's two minimizer views with a numpy restatement of minimizer_views, and draws again where a flank
happened to beat the core.  model() restates image_build.hip's bucket_k / ovf_count_k: what stays inline, which runs are heavy, and how
many record slots the packed overflow area has -- utree_dev_info.overflow_bytes is exactly that times the record size."""
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from utree_amd import ctrfile

M32 = 0xFFFFFFFF
C1, C2 = 0x9E3779B1, 0x85EBCA6B
C1_INV, C2_INV = pow(C1, -1, 1 << 32), pow(C2, -1, 1 << 32)
MIN_LOW_BITS = 9                    # 16-mers are ranked by hash >> 9, leftmost on ties (device_common.hpp)
OVF_DIR_MIN = 32                    # a run of more records, all of one hash value, is heavy
OVF_DIR_MAX = 0xFFFF                # ... up to the directory's 16-bit offsets


def mix32(x):
    x = (x * C1) & M32
    x ^= x >> 15
    return (x * C2) & M32


def unmix32(h):
    x = (h * C2_INV) & M32
    x ^= x >> 15
    x ^= x >> 30
    return (x * C1_INV) & M32


def rc16(x):
    r = 0
    for j in range(16):
        r = (r << 2) | (3 - ((x >> (2 * j)) & 3))
    return r


def mer_codes(x):
    return np.array([(x >> (30 - 2 * j)) & 3 for j in range(16)], dtype=np.uint8)


def margin(k):
    """UTREE_MIN_MARGIN: the minimizer of a k = 64 window keeps two bases' distance from the window's ends."""
    return 2 if k == 64 else 0


def positions(k):
    """Positions a k-mer's minimizer may take."""
    return list(range(margin(k), k - 16 - margin(k) + 1))


def rec_words(W, I):
    return (2 if W == 16 else 1) * (2 if I == 4 else 1)


def cap(W, I, bucket_bytes):
    return bucket_bytes // 8 // rec_words(W, I)


def dir_slots(W, I):
    """OvfDir<W, I>::SLOTS: K-16+2 offsets of 16 bits, in record slots."""
    ew = rec_words(W, I)
    return (2 * (4 * W - 16 + 2) + 8 * ew - 1) // (8 * ew)


def cores_in_slot(slot):
    """(hash, canonical 16-mer) of every hash value of slot `slot` (hashes slot * 256 ..) that has a canonical, non-palindromic preimage."""
    out = []
    for h in range(slot << 8, (slot + 1) << 8):
        x = unmix32(h)
        if h and x < rc16(x):
            out.append((h, x))
    return out


# ---- numpy restatement of minimizer_views -------------------------------------------------------------------------------------------
def _mix32_np(x):
    x = (x * np.uint64(C1)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    return (x * np.uint64(C2)) & np.uint64(M32)


def views(bases):
    """bases: uint8[N, k] codes.  Both views of every k-mer: dict of hf, of, pf (leftmost 16-mer of the smallest rank) and hg, og, pg
    (rightmost; orientation 1 for a palindrome)."""
    n, k = bases.shape
    nm = k - 15
    b = bases.astype(np.uint64)
    m = np.zeros((n, nm), np.uint64)
    r = np.zeros((n, nm), np.uint64)
    for i in range(16):
        m = (m << np.uint64(2)) | b[:, i:i + nm]
        r = (r << np.uint64(2)) | (np.uint64(3) - b[:, 15 - i:15 - i + nm])
    h = _mix32_np(np.minimum(m, r))
    j0 = margin(k)
    key = (h >> np.uint64(MIN_LOW_BITS))[:, j0:nm - j0]
    rows = np.arange(n)
    pf = np.argmin(key, axis=1) + j0
    pg = (nm - j0 - 1) - np.argmin(key[:, ::-1], axis=1)
    return {"hf": h[rows, pf], "of": (m[rows, pf] > r[rows, pf]).astype(np.uint8), "pf": pf,
            "hg": h[rows, pg], "og": (m[rows, pg] >= r[rows, pg]).astype(np.uint8), "pg": pg}


def pack(bases):
    """(hi, lo) words of uint8[N, k] codes, first base most significant."""
    n, k = bases.shape
    b = bases.astype(np.uint64)
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)
    for j in range(k - 32, k):
        lo = (lo << np.uint64(2)) | b[:, j]
    for j in range(0, k - 32):
        hi = (hi << np.uint64(2)) | b[:, j]
    return hi, lo


ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def text(row):
    return ACGT[row].tobytes().decode()


def revcomp(s):
    return s.encode().translate(_COMP)[::-1].decode()


@dataclass
class Spec:
    """`counts[pos]` k-mers whose minimizer is `core` (a canonical 16-mer; orient 1: they hold its reverse complement) at position pos."""
    core: int
    orient: int
    counts: Dict[int, int]
    name: str = ""
    fixed: np.ndarray = None        # uint8[n, k]: the k-mers themselves, ascending by position (else: random flanks, drawn by build())

    @property
    def n(self):
        return sum(self.counts.values())

    @property
    def hash(self):
        return mix32(self.core)


def spread(k, n):
    """n k-mers spread evenly over the allowed positions."""
    ps = positions(k)
    c = {}
    for i in range(n):
        p = ps[(i * len(ps)) // n]
        c[p] = c.get(p, 0) + 1
    return c


@dataclass
class Built:
    k: int
    specs: List[Spec]
    bases: np.ndarray               # uint8[N, k]: the designed k-mers first (spec after spec, position after position), then the filler
    spec_of: np.ndarray             # int32[N]: index into specs, -1 for filler
    pos_of: np.ndarray              # int32[N]: designed minimizer position (-1 for filler)
    ix: np.ndarray                  # uint32[N]: label index
    labels: List[str]
    hi: np.ndarray = field(default=None)
    lo: np.ndarray = field(default=None)

    @property
    def n_designed(self):
        return int((self.spec_of >= 0).sum())

    def write(self, path, I):
        order = np.lexsort((self.lo, self.hi))
        ctrfile.write_ctr(path, self.k // 4, I, self.hi[order], self.lo[order], self.ix[order], self.labels)
        return path


LABELS = ["k__B;p__P%d;c__C%d;o__O%d" % (a, b, c) for a in range(2) for b in range(3) for c in range(5)] + \
         ["k__B;p__P%d;c__C%d" % (a, b) for a in range(2) for b in range(3)] + ["k__B;p__P%d" % a for a in range(2)]


def build(k, specs, seed, filler=0):
    """The k-mers of `specs` plus `filler` random ones whose minimizer hash is no designed bucket's (>= 2^20) and whose two views agree.
    Every designed k-mer is checked: both views are (the core's hash, the spec's orientation, the spec's position)."""
    rng = np.random.default_rng(seed)
    sid, pid = [], []
    for si, s in enumerate(specs):
        assert s.core < rc16(s.core), "core not canonical"
        for p in sorted(s.counts):
            assert p in positions(k), "position %d is none the minimizer may take" % p
            sid += [si] * s.counts[p]
            pid += [p] * s.counts[p]
    sid = np.array(sid + [-1] * filler, dtype=np.int32)
    pid = np.array(pid + [-1] * filler, dtype=np.int32)
    n = len(sid)
    cores = np.zeros((len(specs), 16), np.uint8)
    hashes = np.zeros(len(specs), np.uint64)
    for si, s in enumerate(specs):
        cores[si] = mer_codes(rc16(s.core) if s.orient else s.core)
        hashes[si] = s.hash
    orient = np.array([s.orient for s in specs], dtype=np.uint8)
    bases = np.zeros((n, k), np.uint8)
    des = sid >= 0
    given = np.zeros(n, bool)
    for si, s in enumerate(specs):
        if s.fixed is not None:
            given[sid == si] = True
    todo = np.flatnonzero(~given)
    for si, s in enumerate(specs):
        if s.fixed is not None:
            bases[sid == si] = s.fixed
    v = views(bases[given]) if given.any() else None
    if v is not None:
        g = np.flatnonzero(given)
        assert np.array_equal(v["pf"], pid[g]) and np.array_equal(v["pg"], pid[g]) and np.array_equal(v["hf"], hashes[sid[g]]) and \
            np.array_equal(v["of"], orient[sid[g]]) and np.array_equal(v["og"], orient[sid[g]]), "a given k-mer's minimizer is not its spec's"
    for _ in range(100):
        if not len(todo):
            break
        bases[todo] = rng.integers(0, 4, (len(todo), k), dtype=np.uint8)
        d = todo[des[todo]]
        if len(d):
            cols = pid[d][:, None] + np.arange(16)[None, :]
            bases[d[:, None], cols] = cores[sid[d]]
        v = views(bases[todo])
        same = (v["pf"] == v["pg"]) & (v["of"] == v["og"])
        t_des = des[todo]
        s_ = np.where(t_des, sid[todo], 0)
        ok_des = same & (v["pf"] == pid[todo]) & (v["hf"] == hashes[s_]) & (v["of"] == orient[s_]) if len(specs) else same
        ok_fill = same & (v["hf"] >= np.uint64(1 << 20))
        ok = np.where(t_des, ok_des, ok_fill)
        bad = set(todo[~ok].tolist())
        hi, lo = pack(bases)
        o = np.lexsort((lo, hi))
        dup = np.zeros(n, bool)
        eq = (hi[o][1:] == hi[o][:-1]) & (lo[o][1:] == lo[o][:-1])
        dup[o[1:]] = eq
        dup[o[:-1]] |= eq                                    # both of an equal pair: a given k-mer is never drawn again, its double is
        bad |= set(np.flatnonzero(dup & ~given).tolist())
        todo = np.array(sorted(bad), dtype=np.int64)
    assert not len(todo), "flanks could not be drawn"
    ix = np.where(des, (sid * 7 + pid) % len(LABELS), rng.integers(0, len(LABELS), n)).astype(np.uint32)
    hi, lo = pack(bases)
    o = np.lexsort((lo, hi))
    assert not ((hi[o][1:] == hi[o][:-1]) & (lo[o][1:] == lo[o][:-1])).any(), "k-mers are not distinct"
    return Built(k, list(specs), bases, sid, pid, ix, LABELS, hi, lo)


# ---- the model of the image ---------------------------------------------------------------------------------------------------------
def rest32(bases, pos):
    """k = 32: the 16 bases outside the 16-mer at `pos` (min_rest), first base on top."""
    j = np.arange(16)[None, :]
    cols = np.where(j < pos[:, None], j, j + 16)
    b = bases[np.arange(len(bases))[:, None], cols].astype(np.int64)
    r = np.zeros(len(bases), np.int64)
    for x in range(16):
        r = (r << 2) | b[:, x]
    return r


def chain_heads(pos, rest):
    """ChainRun's linking rule (image_build.hip), k = 32: the record at position p with outer bases `rest` follows a record at p - 1 whose
    rest >> 2 equals its rest's low 30 bits -- the t-th of the up to four such records at p (by leading base) follows the t-th of the up to
    four at p - 1.  Heads = records that follow none."""
    at, before = {}, {}
    for p, r in zip(pos.tolist(), rest.tolist()):
        at[(p, r & 0x3FFFFFFF)] = at.get((p, r & 0x3FFFFFFF), 0) + 1
        before[(p + 1, r >> 2)] = before.get((p + 1, r >> 2), 0) + 1
    return len(pos) - sum(min(n, before.get(key, 0)) for key, n in at.items())


def model(built, I, bucket_bytes, dir_on=True, chains=False):
    """The packed overflow area the image of `built` must have: {"slots", "runs": [(bucket, n, c, heavy, slots)], "ovf_scan"}.
    bucket_k leaves all n records of a bucket inline if n <= CAP, else CAP-1 and a descriptor; the run's c = n - (CAP-1) records are the
    bucket's LAST ones in key order (hash's low eight bits, position, outer bases); ovf_count_k calls the run heavy when OVF_DIR_MIN < c <=
    0xFFFF and its first and last record have the same hash bits.  A heavy run gets OvfDir::SLOTS more slots when directories are on; with
    chains on (k = 32) it takes two words per chain and one rank per record instead."""
    W = built.k // 4
    CAP = cap(W, I, bucket_bytes)
    EW = rec_words(W, I)
    chains = chains and W == 8 and dir_on
    v = views(built.bases)
    assert np.array_equal(v["pf"], v["pg"]) and np.array_equal(v["of"], v["og"]), "a k-mer with two views would be stored twice"
    h = v["hf"].astype(np.int64)
    bucket = 2 * (h >> 8) + v["of"]                   # 2^16 slots per region: slot = hash >> 8 over the whole range
    hlow = h & 0xFF
    pos = v["pf"].astype(np.int64)
    rest = rest32(built.bases, pos) if W == 8 else np.zeros(len(h), np.int64)       # (k = 64: the order inside one position changes no count)
    order = np.lexsort((rest, pos, hlow, bucket))
    bs, hl, ps, rs = bucket[order], hlow[order], pos[order], rest[order]
    starts = np.flatnonzero(np.r_[True, bs[1:] != bs[:-1]])
    ends = np.r_[starts[1:], len(bs)]
    runs, slots = [], 0
    for s, e in zip(starts, ends):
        n = int(e - s)
        if n <= CAP:
            continue
        c = n - (CAP - 1)
        heavy = OVF_DIR_MIN < c <= OVF_DIR_MAX and hl[s + CAP - 1] == hl[e - 1]
        if heavy and chains:
            heads = chain_heads(ps[s + CAP - 1:e], rs[s + CAP - 1:e])
            sl = (2 * heads + (c * I + 7) // 8 + EW - 1) // EW
        else:
            sl = c + (dir_slots(W, I) if heavy and dir_on else 0)
        runs.append((int(bs[s]), n, c, bool(heavy), sl))
        slots += sl
    return {"slots": slots, "bytes": slots * EW * 8, "runs": runs, "ovf_scan": 16 if slots * 4 > len(h) else 32}


def bucket_of(spec):
    return 2 * (spec.hash >> 8) + spec.orient


# ---- reads ----------------------------------------------------------------------------------------------------------------------------
def near_misses(built, rows, members):
    """For every k-mer of `rows` (designed ones) two words that are not in the database but have the same minimizer at the same position:
    the first and the last base outside the core changed.  Returns uint8[M, k]."""
    out = []
    for which in (0, 1):
        cand = built.bases[rows].copy()
        p = built.pos_of[rows]
        k = built.k
        col = np.where(p > 0, 0, 16) if which == 0 else np.where(p < k - 16, k - 1, p - 1)
        left = np.ones(len(rows), bool)
        orig = cand[np.arange(len(rows)), col].copy()
        for alt in (1, 2, 3):
            idx = np.flatnonzero(left)
            if not len(idx):
                break
            cand[idx, col[idx]] = (orig[idx] + alt) & 3
            v = views(cand[idx])
            b = built.bases[rows[idx]]
            vo = views(b)
            hi, lo = pack(cand[idx])
            fresh = np.array([(int(a), int(c)) not in members for a, c in zip(hi, lo)], dtype=bool)
            ok = fresh & (v["pf"] == vo["pf"]) & (v["hf"] == vo["hf"]) & (v["of"] == vo["of"])
            left[idx[ok]] = False
        out.append(cand[~left])
    return np.concatenate(out)


def boundary_rows(built):
    """Of every (spec, position) the k-mers with the smallest and the largest outer bases: the first and the last record of each range a
    position directory names, the last record of the run among them."""
    rows = np.flatnonzero(built.spec_of >= 0)
    k = built.k
    j = np.arange(k - 16)[None, :]
    pos = built.pos_of[rows]
    rest = built.bases[rows[:, None], np.where(j < pos[:, None], j, j + 16)]
    order = np.lexsort(tuple(rest[:, ::-1].T) + (pos, built.spec_of[rows]))
    s, p = built.spec_of[rows][order], pos[order]
    first = np.r_[True, (s[1:] != s[:-1]) | (p[1:] != p[:-1])]
    last = np.r_[first[1:], True]
    return np.sort(rows[order[first | last]])


def reads_for(built, seed, sample=None, random_reads=300):
    """(a) every placed k-mer (or `sample` of them and boundary_rows), (b) two near misses of every third and of boundary_rows, (c) per spec and populated position a read of
    k + (k-16) bases around one placed k-mer with the core in the middle -- its windows ask for every position of the run, one of them
    a hit -- and one with random flanks, (d) the reverse complements of all of these, (e) random reads.  Returns [(name, sequence)] and
    the rows of (a), the rows whose near misses were made, and the near misses (for the CPU checks)."""
    rng = np.random.default_rng(seed)
    k = built.k
    rows = np.flatnonzero(built.spec_of >= 0)
    if sample is not None and sample < len(rows):
        rows = np.union1d(rng.choice(rows, sample, replace=False), boundary_rows(built))
    members = set(zip((int(x) for x in built.hi), (int(x) for x in built.lo)))
    third = np.union1d(rows[::3], boundary_rows(built))
    miss = near_misses(built, third, members)
    reads = [("a%d" % r, text(built.bases[r])) for r in rows]
    reads += [("b%d" % i, text(m)) for i, m in enumerate(miss)]
    ext = k - 16
    for si, s in enumerate(built.specs):
        core = mer_codes(rc16(s.core) if s.orient else s.core)
        for p in sorted(s.counts):
            r = int(np.flatnonzero((built.spec_of == si) & (built.pos_of == p))[0])
            seq = np.concatenate([rng.integers(0, 4, ext - p, dtype=np.uint8), built.bases[r], rng.integers(0, 4, p, dtype=np.uint8)])
            reads.append(("c%d_%d" % (si, p), text(seq)))
        seq = np.concatenate([rng.integers(0, 4, ext, dtype=np.uint8), core, rng.integers(0, 4, ext, dtype=np.uint8)])
        reads.append(("c%d_x" % si, text(seq)))
    reads += [("d_" + n, revcomp(s)) for n, s in reads]
    reads += [("e%d" % i, text(rng.integers(0, 4, int(rng.integers(k, 161)), dtype=np.uint8))) for i in range(random_reads)]
    return reads, rows, third, miss


def fasta(reads):
    return b"".join(b">" + n.encode() + b"\n" + s.encode() + b"\n" for n, s in reads)


# ---- the designed databases -----------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (15, 16, 17, 31, 32, 33, 34, 100)


def _pick(slot, nth=0):
    return cores_in_slot(slot)[nth][1]


def thresholds_specs(W, I, bucket_bytes):
    """One bucket each, distinct slots: n = CAP-1 .. CAP+2 records, and runs of c = 15 .. 100 (n = c + CAP-1); the first core also in the
    other orientation (run of 33), the 100-run's too (run of 17): both buckets of a pair overflow."""
    k, CAP = 4 * W, cap(W, I, bucket_bytes)
    specs = []
    slot = 1
    for n in (CAP - 1, CAP, CAP + 1, CAP + 2):
        specs.append(Spec(_pick(slot), n & 1, spread(k, n), "n%d" % n))
        slot += 1
    for c in RUN_LENGTHS:
        specs.append(Spec(_pick(slot), c & 1, spread(k, c + CAP - 1), "c%d" % c))
        slot += 1
    specs.append(Spec(specs[4].core, 1 - specs[4].orient, spread(k, 33 + CAP - 1), "c33_other"))
    specs.append(Spec(specs[-2].core, 1 - specs[-2].orient, spread(k, 17 + CAP - 1), "c17_other"))
    return specs


def not_heavy_specs(W, I, bucket_bytes):
    """Two pairs of cores that share a slot and an orientation.  Pair one: CAP-1 + 20 records of the smaller hash and 20 of the larger: the run
    of 20 + 20 > 32 records begins in the first core's records and ends in the second's: not heavy.  Pair two: CAP-1 records of the smaller
    hash -- exactly the inline ones -- and 40 of the larger: the run is one hash value's alone, heavy."""
    k, CAP = 4 * W, cap(W, I, bucket_bytes)
    a = cores_in_slot(20)
    b = cores_in_slot(21)
    assert a[0][0] < a[1][0] and b[0][0] < b[1][0]
    return [Spec(a[0][1], 0, spread(k, CAP - 1 + 20), "mix_lo"), Spec(a[1][1], 0, spread(k, 20), "mix_hi"),
            Spec(b[0][1], 1, spread(k, CAP - 1), "inline_lo"), Spec(b[1][1], 1, spread(k, 40), "heavy_hi")]


def positions_specs(W, I, bucket_bytes):
    """Heavy runs of about 60 records: all at the lowest position, all at the highest, at every other position only, and one record at each
    position but one that holds 40."""
    k, CAP = 4 * W, cap(W, I, bucket_bytes)
    ps = positions(k)
    n = 60 + CAP - 1
    every_other = {p: 0 for p in ps[::2]}
    for i in range(n):
        every_other[ps[::2][i % len(ps[::2])]] += 1
    lump = {p: 1 for p in ps}
    lump[ps[len(ps) // 3]] = 40                          # (k = 32: 16 + 40 records, a run of 41 at the largest CAP: heavy everywhere)
    return [Spec(_pick(30), 0, {ps[0]: n}, "lowest"), Spec(_pick(31), 1, {ps[-1]: n}, "highest"),
            Spec(_pick(32), 0, every_other, "every_other"), Spec(_pick(33), 1, lump, "lump")]


def stretch_spec(k, core, orient, n_stretches, seed, name):
    """The k-mers that slide over `n_stretches` random stretches with the core in the middle, and over a sibling of each that differs in the
    base in front of the core: consecutive k-mers overlap in k - 1 bases -- the records ChainRun links (k = 32) -- and the sibling's branch
    off where the changed base enters."""
    rng = np.random.default_rng(seed)
    mg = margin(k)
    L = k - 16 - mg
    word = mer_codes(rc16(core) if orient else core)
    rows, pos = [], []
    for _ in range(n_stretches):
        while True:
            S = np.concatenate([rng.integers(0, 4, L, dtype=np.uint8), word, rng.integers(0, 4, L, dtype=np.uint8)])
            T = S.copy()
            T[L - 1] = (T[L - 1] + 1 + int(rng.integers(0, 3))) & 3
            offs = list(range(0, L - mg + 1))
            km = [S[o:o + k] for o in offs] + [T[o:o + k] for o in offs if o <= L - 1]
            pp = [L - o for o in offs] + [L - o for o in offs if o <= L - 1]
            v = views(np.array(km))
            if np.array_equal(v["pf"], pp) and np.array_equal(v["pg"], pp) and (v["hf"] == mix32(core)).all() and \
                    (v["of"] == orient).all() and (v["og"] == orient).all():
                break
        rows += km
        pos += pp
    rows, pos = np.array(rows), np.array(pos)
    o = np.argsort(pos, kind="stable")
    counts = {}
    for p in pos.tolist():
        counts[p] = counts.get(p, 0) + 1
    return Spec(core, orient, counts, name, rows[o])


def stretch_specs(W, I, bucket_bytes):
    """A heavy run of sliding k-mers: three stretches and their siblings."""
    return [stretch_spec(4 * W, _pick(34), 0, 3, 34 + W, "stretch")]


def sixteen_bits_specs(W, I, bucket_bytes):
    """A run of exactly 65535 records (heavy: the directory's last entry is 65535) and, in another slot, one of 65536 (not heavy)."""
    k, CAP = 4 * W, cap(W, I, bucket_bytes)
    return [Spec(_pick(40), 0, spread(k, 65535 + CAP - 1), "c65535"), Spec(_pick(41), 1, spread(k, 65536 + CAP - 1), "c65536")]


def many_runs_specs(W, I, bucket_bytes, n_buckets=200):
    """200 overflowing buckets in 100 slots (both orientations of a core): even ones with runs of 5 or 9 .. 16 records (SHORT: every fifth even
    one has 5), odd ones of 17 .. 60 (LONG)."""
    k, CAP = 4 * W, cap(W, I, bucket_bytes)
    specs = []
    for b in range(n_buckets):
        c = (5 if b % 10 == 0 else 9 + (b // 2) % 8) if b % 2 == 0 else 17 + ((b // 2) * 5) % 44
        specs.append(Spec(_pick(50 + b // 2), b % 2, spread(k, c + CAP - 1), "m%d_c%d" % (b, c)))
    return specs


def stitched_reads(built, n_reads, seed, n_forward=None):
    """150-base reads over a many_runs_specs database, each with several different cores 29-30 bases apart, so that every core is the only
    whole one in some windows and so the minimizer of a run of its own -- a run whose bucket overflows.
    k = 32: [a placed k-mer of a LONG bucket][SHORT][LONG][SHORT][LONG], cores at p0, 39, 69, 99, 128.  A window s = [s, s + 32) holds the core at c
            whole iff c - 16 <= s <= c: the ranges [<= p0], [23, 39], [53, 69], [83, 99], [112, 118] are disjoint, so the read has five
            overflowing runs, the two SHORT ones of 17 windows, the LONG ones of >= 1, 17 and 7.
    k = 64: [a placed k-mer of a LONG bucket, core at p0 >= 25][SHORT][LONG][SHORT], cores at p0, 70, 99, 128.  The core at c is a candidate of
            window s iff c - 46 <= s <= c - 2 (UTREE_MIN_MARGIN): alone for s in [0, 23] (p0), [47, 52] (70), [69, 81] (99) -- three overflowing
            runs for certain, the LONG ones of >= 24 and >= 13 windows, at most four in all.
    SHORT buckets here have runs of 9 .. 16 records, LONG ones of 17 .. 60.
    The first n_forward reads (default: the largest multiple of 64 up to three quarters of them) are as described: whole wavefronts' worth
    of 64 consecutive reads.  The reads behind them are reverse-complemented: there every core names the OTHER bucket of its pair (a SHORT
    piece a LONG bucket and the reverse, the 5-record buckets included) and the window ranges are mirrored; nothing is claimed for them but
    the oracle's lines."""
    rng = np.random.default_rng(seed)
    if n_forward is None:
        n_forward = (n_reads * 3 // 4) // 64 * 64
    k = built.k
    nb = len(built.specs)
    short = [b for b in range(0, nb, 2) if b % 10]
    long_ = list(range(1, nb, 2))
    lead, plan = (7, ("S", "L", "S", "L")) if k == 32 else (6, ("S", "L", "S"))
    lens = (30, 30, 29, 29) if k == 32 else (29, 29, 28)
    rows_of = {}
    for b in long_:
        r = np.flatnonzero((built.spec_of == b) & (built.pos_of >= (0 if k == 32 else 25)))
        if len(r):
            rows_of[b] = r
    out = []
    for i in range(n_reads):
        while True:
            b0 = long_[int(rng.integers(0, len(long_)))]
            picks = [b0] + [(short if t == "S" else long_)[int(rng.integers(0, len(short if t == "S" else long_)))] for t in plan]
            if b0 in rows_of and len({p // 2 for p in picks}) == len(picks):       # different cores, not the two orientations of one
                break
        parts = [built.bases[int(rng.choice(rows_of[b0]))]]
        for b, ln in zip(picks[1:], lens):
            s = built.specs[b]
            piece = rng.integers(0, 4, ln, dtype=np.uint8)
            piece[lead:lead + 16] = mer_codes(rc16(s.core) if s.orient else s.core)
            parts.append(piece)
        seq = text(np.concatenate(parts))
        assert len(seq) == 150
        out.append(("s%d" % i, seq if i < n_forward else revcomp(seq)))
    return out
