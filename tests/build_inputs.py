"""Seeded inputs for the database BUILD at its edges (build_gpu.hip), and a plain numpy model of what BUILD makes of an input whose
references all carry ONE label.  The generator of golden/reference_runs.json (`make_golden.py reference_runs build_edges`), the CPU tests
(test_build_edges_cpu.py) and the GPU tests (test_gpu_build_edges.py) make the inputs here, so every one of them runs on the very bytes the
genuine builders ran on (util.reference_run checks the hashes).

Every builder returns a Case: FASTA bytes, map bytes, and what it planted.  K = 4 W bases per word, kv = K - 1 + lv (lv = complevel): a
reference of `length` bases has max(0, length - kv) positions; position p is the lv filter bases at p .. p+lv-1 (they must read A, G, C, T)
followed by the k-mer at p+lv .. p+kv.
"""
import hashlib
from collections import namedtuple

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = np.full(256, 255, dtype=np.uint8)                # the reference's C2Xb (itree.c:110-121): exactly ACGTacgt are bases
for _c, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    CODE[_c] = _v
FILTER = (0, 2, 1, 3)                                   # codes of A, G, C, T: the complevel filter (itree.c:605-616)
N_BUCKETS = 4096                                        # build_gpu.hip passes: ranges of the words' top 12 bits
U64 = np.uint64

LA = "k__A;p__B;c__C;o__D"
LB = "k__A;p__B;c__C;o__E"                              # LA then LB: cut to "k__A;p__B;c__C"
LX = "k__A;p__B;c__X"                                   # ... then LX: cut to "k__A;p__B"; LX second instead: "k__A;p__B", then BAD
LC = "k__A;p__B;c__Q;o__F"                              # LA / LB then LC: "k__A;p__B"
LD = "k__Z;p__Y"                                        # shares no ';' with the others: BAD
LE = "k__A;p__B;c__C;o__D;f__G;g__H"
LF = "k__A;p__B;c__C;o__D;f__G;g__I"                    # LE then LF: "k__A;p__B;c__C;o__D;f__G"
C3, C2, C5 = "k__A;p__B;c__C", "k__A;p__B", "k__A;p__B;c__C;o__D;f__G"
ONE = "k__One;p__Label;c__Only"

Case = namedtuple("Case", "fa map planted")
Model = namedtuple("Model", "valid n_kmers n_distinct hi lo occ_hi occ_lo hist total_pos")


def sha256(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


# ---------------------------------------------------------------- the model ----------------------------------------------------------------
def frame(fa: bytes):
    """(header, sequence) line pairs as the reference reads them (itree.c:585-600): the name is the header line after its first byte, the
    sequence line loses one '\\n' and then one '\\r'.  Returns [(name, sequence)]."""
    out, pos, n = [], 0, len(fa)
    while pos < n:
        e = fa.find(b"\n", pos)
        e = n if e < 0 else e
        name = fa[pos + 1:e]
        pos = e + 1
        assert pos < n, "header without a sequence line"
        e = fa.find(b"\n", pos)
        e = n if e < 0 else e
        seq = fa[pos:e]
        if seq.endswith(b"\r"):
            seq = seq[:-1]
        out.append((name, seq))
        pos = e + 1
    return out


def join(refs, eol=b"\n"):
    return b"".join(b">" + n + eol + s + eol for n, s in refs)


def reverse_refs(case: Case) -> Case:
    """The same references in reverse order (well-formed LF files only)."""
    return Case(join(frame(case.fa)[::-1]), case.map, case.planted)


def positions(seq: bytes, W: int, lv: int):
    """One reference: (valid[p], hi[p], lo[p]) over its positions; the words are only meaningful where valid."""
    K = 4 * W
    kv = K - 1 + lv
    npos = max(0, len(seq) - kv)
    if not npos:
        z = np.zeros(0, dtype=U64)
        return np.zeros(0, dtype=bool), z, z
    c = CODE[np.frombuffer(seq, dtype=np.uint8)]
    cs = np.concatenate([[0], np.cumsum(c == 255)])
    p = np.arange(npos)
    ok = (cs[p + lv + K] - cs[p + lv]) == 0
    for f in range(lv):
        ok &= c[p + f] == FILTER[f]
    hi, lo = np.zeros(npos, dtype=U64), np.zeros(npos, dtype=U64)
    for j in range(K):                                   # first base most significant
        hi = (hi << U64(2)) | (lo >> U64(62))
        lo = (lo << U64(2)) | (c[p + lv + j].astype(U64) & U64(3))
    if W != 16:
        hi[:] = 0
    if W == 4:
        lo &= U64(0xFFFFFFFF)
    return ok, hi, lo


def bucket_of(W: int, hi, lo):
    if W == 4:
        return ((lo >> U64(20)) & U64(N_BUCKETS - 1)).astype(np.int64)
    return ((hi if W == 16 else lo) >> U64(52)).astype(np.int64)


def model(fa: bytes, W: int, lv: int) -> Model:
    """Valid k-mers per position (table lookup of ACGTacgt, complevel filter A, G, C, T), their number, and the sorted distinct words.  For
    an input under one label that is the whole `.ubt` (ubt_bytes)."""
    valid, his, los, tot = [], [], [], 0
    for _, seq in frame(fa):
        ok, hi, lo = positions(seq, W, lv)
        valid.append(ok)
        his.append(hi[ok])
        los.append(lo[ok])
        tot += len(ok)
    occ_hi, occ_lo = np.concatenate(his), np.concatenate(los)
    order = np.lexsort((occ_lo, occ_hi))
    shi, slo = occ_hi[order], occ_lo[order]
    head = np.ones(len(slo), dtype=bool)
    head[1:] = (shi[1:] != shi[:-1]) | (slo[1:] != slo[:-1])
    hist = np.bincount(bucket_of(W, occ_hi, occ_lo), minlength=N_BUCKETS)
    return Model(valid, len(occ_lo), int(head.sum()), shi[head], slo[head], occ_hi, occ_lo, hist, tot)


def label_lines(label: str, n: int) -> bytes:
    return ("%s\t%d\n" % (label, n)).encode()


def ubt_bytes(m: Model, W: int, I: int, label: str = ONE) -> bytes:
    """The `.ubt` of a one-label input (UT_writeTreeBinary, itree.c:1317-1343): header, (W-byte little-endian word, index 0) ascending, the
    label line.  The log file is the label line alone."""
    n = len(m.lo)
    rec = np.zeros((n, W + I), dtype=np.uint8)
    full = np.concatenate([np.ascontiguousarray(m.lo.astype("<u8")).view(np.uint8).reshape(n, 8),
                           np.ascontiguousarray(m.hi.astype("<u8")).view(np.uint8).reshape(n, 8)], axis=1)
    rec[:, :W] = full[:, :W]
    return np.array([W, 0, I, n], dtype="<u8").tobytes() + rec.tobytes() + label_lines(label, n)


def pass_ranges(hist, limit: int):
    """build_gpu.hip's passes under UTREE_BUILD_PASS_KMERS = limit: [(first bucket, end bucket, occurrences)], the ranges without a k-mer
    included; None where one bucket is over the limit (the build refuses)."""
    out, b = [], 0
    while b < N_BUCKETS:
        cnt, e = int(hist[b]), b + 1
        if cnt > limit:
            return None
        while e < N_BUCKETS and cnt + int(hist[e]) <= limit:
            cnt += int(hist[e])
            e += 1
        out.append((b, e, cnt))
        b = e
    return out


def pass_of(ranges, bucket: int) -> int:
    return next(i for i, (b, e, _) in enumerate(ranges) if b <= bucket < e)


# ---------------------------------------------------------------- the inputs ----------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([20261019] + [int(k) for k in key])


def _bases(rng, n: int, mixed: bool = False) -> bytes:
    b = ACGT[rng.integers(0, 4, n)]
    if mixed:
        b = b | (rng.integers(0, 2, n).astype(np.uint8) << 5)        # per-base random case
    return b.tobytes()


def _one_label_map(names, label=ONE) -> bytes:
    return b"".join(n + b"\t" + label.encode() + b"\n" for n in names)


HOSTILE = [b for b in range(1, 128) if b != 10]


def bytes_case(W: int, lv: int) -> Case:
    """Base coding (code4 / eval_pos): a random ACGT backbone with per-base random case, in which every byte 0x01-0x7F except '\\n' stands
    once inside a window whose filter bases are right (at every offset modulo 4 over the bytes, K+8 bases apart), and once more in each of
    the lv filter slots in front of an otherwise valid k-mer.  IUPAC letters, digits, blanks, a mid-line '\\r', and the letters that share
    their 2-bit code bits with a base ('U'/'T', 'E', 'B', 'Q', ...) are all among them.  One label; three references: one LF, one whose
    header and sequence end in CRLF, and a last one without a final newline.
    NUL and bytes >= 0x80 are left out: the reference cuts a line at NUL (strlen, itree.c:598) and indexes its table with a signed char
    (itree.c:606-619), so it defines no result for either."""
    rng = _rng(1, W, lv)
    K = 4 * W
    motif = b"AGCT"[:lv]

    def cased(s):
        return bytes(c | (int(rng.integers(0, 2)) << 5) for c in s)
    parts = []
    for n, b in enumerate(HOSTILE):
        a = (5 * n + 3) % K                                           # where in the k-mer it stands: every residue modulo 4, all dwords
        parts.append(cased(motif) + _bases(rng, a, True) + bytes([b]) + _bases(rng, K - 1 - a, True) + _bases(rng, 8, True))
    for f in range(lv):
        for b in HOSTILE:
            m = bytearray(cased(motif))
            m[f] = b
            parts.append(bytes(m) + _bases(rng, K + 2, True))
    order = rng.permutation(len(parts))
    parts = [parts[i] for i in order]
    a, b = int(len(parts) * 0.6), int(len(parts) * 0.8)
    seqs = [b"".join(p) + _bases(rng, 4) for p in (parts[:a], parts[a:b], parts[b:])]      # a last '\r' would be lopped off: end on bases
    fa = b">b0 main\n" + seqs[0] + b"\n" + b">b1 crlf\r\n" + seqs[1] + b"\r\n" + b">b2 open end\n" + seqs[2]
    mp = _one_label_map([b"b1 crlf\r", b"b2 open end", b"b0 main"])
    return Case(fa, mp, {"label": ONE, "bytes": HOSTILE, "lv": lv, "n_refs": 3})


SHAPE_TARGETS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def shape_case(W: int, target: int, lv: int = 0, many: bool = False) -> Case:
    """Position -> reference and the ordered compaction: total_pos is exactly `target`.  References without a position (1, kv-1 and kv bases)
    stand first, last and three in a row; references with one position (kv+1 bases) stand between them; one longer reference supplies the
    rest.  many: every reference under a label of its own (plain BUILD then writes each reference's position count into the log, the
    position-less ones as labels with no node).  A reference of 0 bases stays out: the reference reads src[-1] there (itree.c:599)."""
    rng = _rng(2, W, target, lv)
    kv = 4 * W - 1 + lv
    singles, rest = min(target, 3), target - min(target, 3)
    lens = [1, kv - 1, kv]
    lens += [kv + 1] if singles >= 1 else []
    lens += [kv]
    lens += [kv + 1] if singles >= 2 else []
    lens += [1]
    lens += [kv + rest] if rest else []
    lens += [kv - 1]
    lens += [kv + 1] if singles >= 3 else []
    lens += [kv, kv - 1, 1]
    refs = [(b"s%d" % i, _bases(rng, L)) for i, L in enumerate(lens)]
    if many:
        mp = b"".join(n + b"\tk__S;p__H;c__R%d\n" % i for i, (n, _) in reversed(list(enumerate(refs))))
    else:
        mp = _one_label_map([n for n, _ in refs])
    return Case(join(refs), mp, {"label": ONE, "total_pos": target, "lens": lens, "many": many})


SPARSE_TOTAL = 3 * 256 + 10
SPARSE_VALID = (63, 256, 512 + 127, SPARSE_TOTAL - 1)     # last lane of a wavefront, first lane of a block, last lane of a block's 2nd wavefront, the last position


def sparse_case(W: int) -> Case:
    """One valid window per block of 256 positions, each the only set bit of its wavefront's ballot: the rest of the long reference is 'N'.
    Two references without a position come first, so the positions are the long reference's offsets."""
    rng = _rng(3, W)
    K = 4 * W
    kv = K - 1
    s = bytearray(b"N" * (SPARSE_TOTAL + kv))
    for g in SPARSE_VALID:
        s[g:g + K] = _bases(rng, K)
    refs = [(b"z0", b"A"), (b"z1", _bases(rng, kv)), (b"sparse", bytes(s)), (b"z2", _bases(rng, kv - 1))]
    return Case(join(refs), _one_label_map([n for n, _ in refs]), {"label": ONE, "total_pos": SPARSE_TOTAL, "valid": SPARSE_VALID, "ref": 2})


def extremes_case(W: int, n_labels: int = 1) -> Case:
    """The all-A word (0, bucket 0) and the all-T word (bucket 4095), each with far more than 256 occurrences (a run longer than a block in
    fold_k), then once more under a second and once under a third label.  n_labels = 3: LA, LB, LX in that order leave both words at
    "k__A;p__B"; any other order of the three ends BAD."""
    rng = _rng(4, W)
    kv = 4 * W - 1
    labs = [ONE] * 3 if n_labels == 1 else [LA, LB, LX]
    refs = [(b"polyA", b"A" * 1000, 0), (b"polyT", b"T" * 1000, 0), (b"mid0", b"G" + _bases(rng, 200), 0),
            (b"A2", b"a" * (kv + 1), 1), (b"T2", b"t" * (kv + 1), 1), (b"A3", b"A" * (kv + 1), 2), (b"T3", b"T" * (kv + 1), 2),
            (b"mid1", b"C" + _bases(rng, 200), 2)]
    mp = b"".join(n + b"\t" + labs[l].encode() + b"\n" for n, _, l in refs)
    return Case(join([(n, s) for n, s, _ in refs]), mp, {"label": ONE, "n_labels": n_labels, "occ": 1000 - kv + 2, "survivor": C2})


def clock_case(W: int) -> Case:
    """Label numbering follows the input position, not the pass:
      X (bucket 0xFFE, a late pass) is cut to C3 early in reference c2, Y (bucket 1, the first pass) is cut to C2 later in c2;
      c3 carries C3 itself, c7 carries C2: labels a cut created before a reference brought them;
      Z is cut to C5 in c5 and goes BAD in c6: C5 keeps its number with no node.
    Filler words start with G or C, so bucket 4095 and the buckets next to X's and Y's stay empty."""
    rng = _rng(5, W)
    K = 4 * W
    X = b"TTTTTG" + _bases(rng, K - 6)
    Y = b"AAAAAC" + _bases(rng, K - 6)
    Z = b"CCCCCC" + _bases(rng, K - 6)

    def F():
        return (b"G" if rng.integers(0, 2) else b"C") + b"A" + _bases(rng, K - 2)     # "CA...", "GA...": not Z's bucket
    refs = [(b"c0", LA, [F(), X, F()]), (b"c1", LC, [F(), Y]), (b"c2", LB, [X, F(), Y]), (b"c3", C3, [F(), X]),
            (b"c4", LE, [Z, F()]), (b"c5", LF, [F(), Z]), (b"c6", LD, [Z, F()]), (b"c7", C2, [F()])]
    mp = b"".join(n + b"\t" + l.encode() + b"\n" for n, l, _ in refs[::-1])
    words = {"X": X, "Y": Y, "Z": Z}
    return Case(join([(n, b"N".join(k)) for n, _, k in refs]), mp,
                {"labels": [LA, LC, LB, C3, C2, LE, LF, C5, LD], "words": words, "empty_label": C5})


def stability_case() -> Case:
    """k = 64 (W = 16), the two-pass sort: 8 x 8 64-mers H_h + L_l (ties in the high half with different low halves, and the reverse), each
    once under LA, LB, LX in that input order, every reference listing them in another order.  A sort that keeps equal words in input order
    leaves all 64 at "k__A;p__B"; any other order of the three occurrences ends BAD."""
    rng = _rng(6)
    H = [_bases(rng, 32) for _ in range(8)]
    L = [_bases(rng, 32) for _ in range(8)]
    M = [h + l for h in H for l in L]
    refs = [(b"fill", LA, [b"G" + _bases(rng, 99)])]
    for n, lab in ((b"r1", LA), (b"r2", LB), (b"r3", LX)):
        refs.append((n, lab, [M[i] for i in rng.permutation(len(M))]))
    mp = b"".join(n + b"\t" + l.encode() + b"\n" for n, l, _ in refs)
    return Case(join([(n, b"N".join(k)) for n, _, k in refs]), mp, {"words": M, "survivor": C2, "places": len(M)})


NO_KMERS = {"short": 0, "n_only": 0, "no_ag": 2}           # name -> complevel


def no_kmers_case(W: int, which: str) -> Case:
    """Inputs without a single k-mer: every reference shorter than k (no position at all), long references of N only (positions, none
    valid), and complevel 2 on sequences that never read AG."""
    rng = _rng(7, W)
    K = 4 * W
    if which == "short":
        seqs = [b"A", _bases(rng, K - 2), _bases(rng, K - 1)]
    elif which == "n_only":
        seqs = [b"N" * 300, b"n" * (K + 1)]
    else:
        seqs = []
        for _ in range(2):
            s = bytearray(_bases(rng, 400, True))
            for i in range(1, len(s)):
                if s[i - 1] in b"Aa" and s[i] in b"Gg":
                    s[i] = ord("C")
            seqs.append(bytes(s))
    refs = [(b"n%d" % i, s) for i, s in enumerate(seqs)]
    return Case(join(refs), _one_label_map([n for n, _ in refs]), {"lv": NO_KMERS[which]})


# ---------------------------------------------------------------- the runs ----------------------------------------------------------------
Run = namedtuple("Run", "key make W lv gg one_label")
WS = (4, 8, 16)


def runs():
    """Every (input, W, complevel, mode) the edge tests build; `make_golden.py reference_runs build_edges` records what the genuine builder
    of that PACKSIZE did on each (I = 2).  one_label: the numpy model gives the whole `.ubt`."""
    out = []

    def add(name, make, W, lv, modes, one):
        for gg in modes:
            out.append(Run("build_edges_%s_W%d_c%d_%s" % (name, W, lv, "gg" if gg else "plain"), make, W, lv, gg, one))
    for W in WS:
        for lv in range(5):
            add("bytes", lambda W=W, lv=lv: bytes_case(W, lv), W, lv, (1, 0) if lv in (0, 4) else (1,), True)
        for t in SHAPE_TARGETS:
            add("shape%d" % t, lambda W=W, t=t: shape_case(W, t), W, 0, (1,), True)
        for t in (1, 64, 257, 513):
            add("shapemany%d" % t, lambda W=W, t=t: shape_case(W, t, many=True), W, 0, (0,), False)
        add("shape257", lambda W=W: shape_case(W, 257, lv=3), W, 3, (0,), True)
        add("sparse", lambda W=W: sparse_case(W), W, 0, (1, 0), True)
        add("extremes1", lambda W=W: extremes_case(W, 1), W, 0, (1,), True)
        add("extremes3", lambda W=W: extremes_case(W, 3), W, 0, (1, 0), False)
        add("clock", lambda W=W: clock_case(W), W, 0, (1, 0), False)
        for which, lv in NO_KMERS.items():
            add("none_" + which, lambda W=W, which=which: no_kmers_case(W, which), W, lv, (1,), True)
    add("stability", stability_case, 16, 0, (1, 0), False)
    return out


def reference_binary(W: int, gg: int) -> str:
    """The genuine builder of oracle/Makefile for this PACKSIZE and mode (IXTYPE uint16_t)."""
    return ("utree-buildGG" if gg else "utree-build") + {4: "-k16", 8: "", 16: "-k64"}[W]
