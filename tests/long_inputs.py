"""Reads up to the reference's line limit (LINELEN = 16 777 216, itree.c:836), and the databases that make them hit.

A sequence line of LMAX = LINELEN - 2 bases is the longest fgets(…, LINELEN) returns whole (LMAX bytes and the newline); one base more and the
reference reads the line in two.  Everything between the suite's 200 kb reads and that limit exists only here: thousands of pieces per read,
per-label counts beyond 2^16, 2^19, 2^20 and 2^24, a record carried whole across a chunk boundary, the serial framing of fasta.c.

Databases (build): a few ten thousand random filler k-mers and the k-mers of five periodic units, one label per unit.  A unit is a random
string of prime length p; a read that repeats it has p distinct windows, all stored, so it hits in EVERY window.  Unit 0's reverse complement
is stored too (both strands hit).  The five labels are two sibling species, their genus, the family above it and a species of another genus.

Reads (read): dense, mixed, striped, sparse, n_every at MID = 2^20 forward windows and at LMAX.  Files (files): the records at the limit, one
past it, five of them in a row, a maximal header, a last line without newline, lower case with CRLF.

Everything is seeded numpy; nothing is stored.  Sequences are numpy uint8 arrays of ASCII (a Python str of 16 M characters costs too much).
"""
from dataclasses import dataclass
from typing import List

import numpy as np

from utree_amd import ctrfile

LINELEN = 1 << 24                   # itree.c:836
LMAX = LINELEN - 2                  # bases of the longest line fgets returns whole
LCAP = 160                          # bases a lane of the lane pass holds (csrc/lanes_core.hpp)

# name: (k, I, seed): one per image kind the search dispatches on
KINDS = {"k32": (32, 2, 3201), "k32u32": (32, 4, 3202), "k64": (64, 2, 3203), "k64u32": (64, 4, 3204), "k16": (16, 2, 3205)}
LANE_PASS = {"k32": 1, "k32u32": 1, "k64": 1, "k64u32": 0, "k16": 0}       # what DeviceTree.info.lane_pass must say
PERIODS = {16: (37, 41, 43, 47, 53), 32: (37, 41, 43, 47, 53), 64: (67, 71, 73, 79, 83)}
N_FILLER = 30000
UNIT_LABELS = ["k__B;p__P;c__C;o__O;f__F;g__G0;s__S0", "k__B;p__P;c__C;o__O;f__F;g__G0;s__S1", "k__B;p__P;c__C;o__O;f__F;g__G0",
               "k__B;p__P;c__C;o__O;f__F", "k__B;p__P;c__C;o__O;f__F;g__G1;s__S0"]
FILLER_LABELS = ["k__B;p__P;c__C;o__O;f__F;g__G1", "k__B;p__P;c__C;o__O;f__F;g__G1;s__S1", "k__B;p__P;c__C;o__O2;f__F;g__G;s__S", "k__B;p__Q",
                 "k__B;p__Q;c__C;o__O;f__F;g__G0;s__S0", "k__A"]
READ_KINDS = ("dense", "mixed", "striped", "sparse", "n_every")
N_PERIOD = 2063                     # an N this often: prime, so coprime to every piece length and tile size
SPARSE_STEP = 100_000
STRIPE_EXTRA = 64                   # `striped`: 64 + k bases of a unit, then the next unit
FINE_EXTRA = 2                      # `striped_fine`: 2 + k bases (three hit windows) -- with both strands more than 2^20 hit-map runs at LMAX

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def mid(k):
    """2^20 forward windows: more pieces than a workgroup has threads, and one label's count beyond 2^19 and at 2^20."""
    return (1 << 20) + k - 1


def piece_windows(k):
    """Windows of one piece of the pieces pass (lanes_kernel.hip: PW = 16 lanes of LCAP - k + 1 windows)."""
    return 16 * (LCAP - k + 1)


def n_pieces(length, k):
    return -(-(length - k + 1) // piece_windows(k)) if length >= k else 0


def _pack(codes):
    m = codes.shape[1]
    sh = (2 * (m - 1 - np.arange(m))).astype(np.uint64)
    return (codes.astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64)


def encode(codes, k):
    """[n, k] base codes 0 .. 3 -> (hi, lo), first base most significant (ctrfile.encode_kmers, vectorised)."""
    if k == 64:
        return _pack(codes[:, :32]), _pack(codes[:, 32:])
    return np.zeros(len(codes), np.uint64), _pack(codes)


def rotations(unit, k):
    """The len(unit) windows of the endless repeat of `unit`, as [p, k] codes."""
    p = len(unit)
    t = np.resize(unit, p + k - 1)
    return np.stack([t[j:j + k] for j in range(p)])


@dataclass
class Built:
    name: str
    k: int
    I: int
    ctr: str
    labels: List[str]
    units: List[np.ndarray]         # base codes of the five units
    filler: np.ndarray              # [N_FILLER, k] base codes
    filler_ix: np.ndarray


def build(name, tmp):
    """The .ctr of one kind (ctrfile.write_ctr): filler k-mers on random labels, the rotations of units 0 .. 4 on labels 0 .. 4, the rotations
    of unit 0's reverse complement on label 0 too.  No word twice."""
    k, I, seed = KINDS[name]
    rng = np.random.default_rng(seed)
    units = []
    for p in PERIODS[k]:
        u = rng.integers(0, 4, p).astype(np.uint8)
        assert len(set(u.tolist())) > 1
        units.append(u)
    labels = UNIT_LABELS + FILLER_LABELS
    filler = rng.integers(0, 4, (N_FILLER, k)).astype(np.uint8)
    filler_ix = rng.integers(0, len(labels), N_FILLER).astype(np.uint32)
    codes = [filler] + [rotations(u, k) for u in units] + [rotations((3 - units[0])[::-1], k)]
    ix = np.concatenate([filler_ix] + [np.full(len(u), i, np.uint32) for i, u in enumerate(units)] + [np.zeros(len(units[0]), np.uint32)])
    hi, lo = encode(np.concatenate(codes), k)
    o = np.lexsort((lo, hi))
    hi, lo, ix = hi[o], lo[o], ix[o]
    assert not ((hi[1:] == hi[:-1]) & (lo[1:] == lo[:-1])).any(), "a word twice: take another seed"
    ctr = str(tmp / ("long_%s.ctr" % name))
    ctrfile.write_ctr(ctr, k // 4, I, hi, lo, ix, labels)
    return Built(name, k, I, ctr, labels, units, filler, filler_ix)


# ---- reads ----------------------------------------------------------------------------------------------------------------------------
def _tile(unit, n):
    return _ACGT[np.resize(unit, n)]


def _stripes(b, n, extra):
    s = b.k + extra
    block = np.concatenate([np.resize(u, s) for u in b.units])
    return _ACGT[np.resize(block, n)]


def read(b, kind, n):
    """One read of n bases as a uint8 array.
    dense: unit 0 throughout; mixed: units 0, 1, 2, 3 in stretches of 9 : 3 : 3 : 1 sixteenths (the windows across a junction miss);
    striped / striped_fine: the five units in turn, 64 + k / 2 + k bases each; sparse: random bases with a filler k-mer in the first window, in
    the last one and about every 100 000 bases; n_every: dense with an N every 2063 bases; lower: mixed in lower case."""
    if kind == "dense":
        return _tile(b.units[0], n)
    if kind in ("mixed", "lower"):
        a, c = 9 * n // 16, 3 * n // 16
        s = np.concatenate([_tile(b.units[0], a), _tile(b.units[1], c), _tile(b.units[2], c), _tile(b.units[3], n - a - 2 * c)])
        return s | 0x20 if kind == "lower" else s
    if kind == "striped":
        return _stripes(b, n, STRIPE_EXTRA)
    if kind == "striped_fine":
        return _stripes(b, n, FINE_EXTRA)
    if kind == "sparse":
        rng = np.random.default_rng(KINDS[b.name][2] * 7 + n % 1000)
        s = _ACGT[rng.integers(0, 4, n, dtype=np.uint8)]
        at = [0, n - b.k] + [int(p + rng.integers(0, 1000)) for p in range(SPARSE_STEP, n - 2 * b.k - 1000, SPARSE_STEP)]
        for j, p in enumerate(at):
            s[p:p + b.k] = _ACGT[b.filler[(j * 7919) % N_FILLER]]
        return s
    if kind == "n_every":
        s = _tile(b.units[0], n).copy()
        s[N_PERIOD - 1::N_PERIOD] = ord("N")
        return s
    raise ValueError(kind)


def short_reads(b, n, seed, length=150):
    """n reads of `length` bases: filler k-mers and random bases."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = _ACGT[rng.integers(0, 4, length, dtype=np.uint8)]
        for p in range(0, length - b.k + 1, b.k + 5):
            if rng.random() < 0.7:
                s[p:p + b.k] = _ACGT[b.filler[int(rng.integers(0, N_FILLER))]]
        out.append(s)
    return out


def fasta(records, nl=b"\n", last_newline=True):
    """records: [(name bytes, uint8 array or bytes)]"""
    parts = []
    for name, s in records:
        parts += [b">", name, nl, s.tobytes() if isinstance(s, np.ndarray) else s, nl]
    if not last_newline:
        parts.pop()
    return b"".join(parts)


FILES = ("one_max", "max_plus_one", "five_max", "max_header", "max_header_plus", "last_no_newline", "lower_crlf", "lower_crlf_whole")
SPLITS = ("max_plus_one", "max_header_plus", "lower_crlf")          # a line of LINELEN - 1 bytes or more: the reference reads it in two


def file_bytes(b, name):
    """short, maximal, short -- and its variants:
    one_max           a `mixed` record of LMAX bases
    max_plus_one      the same with LMAX + 1 bases: the line splits
    five_max          dense, mixed, striped, sparse, n_every at LMAX with 150-base reads between them (84 MB: records straddle 64 MiB)
    max_header        a header line of LINELEN - 2 bytes (and its newline) without a space
    max_header_plus   one byte more: the reference reads the header's remainder as the sequence
    last_no_newline   a maximal last line without newline
    lower_crlf        lower case, CRLF: LMAX bases and "\\r\\n" split; lower_crlf_whole: one base less does not"""
    sh = short_reads(b, 8, KINDS[b.name][2] + 50)
    s = lambda i: (b"s%d" % i, sh[i])
    if name == "one_max":
        return fasta([s(0), s(1), (b"max mixed", read(b, "mixed", LMAX)), s(2), s(3)])
    if name == "max_plus_one":
        return fasta([s(0), s(1), (b"plus", read(b, "mixed", LMAX + 1)), s(2), s(3)])
    if name == "five_max":
        rec = []
        for i, kind in enumerate(READ_KINDS):
            rec += [s(i), (kind.encode(), read(b, kind, LMAX))]
        return fasta(rec + [s(5)])
    if name in ("max_header", "max_header_plus"):
        n = LINELEN - 3 + (name == "max_header_plus")                  # with '>' in front: LINELEN - 2 bytes, or one more
        hdr = np.resize(np.frombuffer(b"header_", dtype=np.uint8), n).tobytes()
        return fasta([s(0), (hdr, read(b, "mixed", 4000)), s(1), s(2)])
    if name == "last_no_newline":
        return fasta([s(0), s(1), (b"last", read(b, "dense", LMAX))], last_newline=False)
    if name in ("lower_crlf", "lower_crlf_whole"):
        return fasta([s(0), (b"lower", read(b, "lower", LMAX - (name == "lower_crlf_whole"))), s(1), s(2)], nl=b"\r\n")
    raise ValueError(name)


def batch_fasta(b, n):
    """The five read kinds at n bases as one FASTA."""
    return fasta([(kind.encode(), read(b, kind, n)) for kind in READ_KINDS])


def mixed_batch(b):
    """One LMAX read among 4000 reads of 150 bases and a few of 3 .. 12 kb: the class lists, then pieces, then left-overs in one launch."""
    rng = np.random.default_rng(KINDS[b.name][2] + 99)
    sh = short_reads(b, 4000, KINDS[b.name][2] + 60)
    rec = [(b"s%d" % i, x) for i, x in enumerate(sh[:2000])]
    rec.append((b"max", read(b, "mixed", LMAX)))
    for i, L in enumerate((3000, 4097, 8191, 12000, 5000)):
        rec.append((b"m%d" % i, read(b, READ_KINDS[i], L)))
    rec += [(b"s%d" % (2000 + i), x) for i, x in enumerate(sh[2000:])]
    order = rng.permutation(len(rec))
    return fasta([rec[j] for j in order])


# ---- what the reference is run on (tests/golden/make_golden.py reference_runs long) ----------------------------------------------------
# kind: the files the classifying search (xtree-searchGG) runs on it, both strand modes each
SEARCH_RUNS = {name: FILES for name in KINDS}
# kind: the files the rank-specific search (xtree-search) runs on it (the reference has no PACKSIZE=16 and no k = 64 / u32 build of it)
RANK_RUNS = {"k32": FILES, "k64": FILES, "k32u32": FILES}


def run_key(name, fname, rc, rank=False):
    return "long_%s%s_%s%s" % ("rank_" if rank else "", name, fname, "_rc" if rc else "")


def reference_binary(k, I, rank=False):
    return ("xtree-search" if rank else "xtree-searchGG") + {16: "-k16", 32: "", 64: "-k64"}[k] + ("-ix32" if I == 4 else "")
