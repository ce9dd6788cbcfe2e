"""The tile contract in plain Python (include/utree_amd.h, utree_tiles_*): the tiles of a query, the pre-split FASTA a user would make by
hand, the per-tile lines as the CPU oracle gives them for each tile as a read of its own, and the segments merged from them.  Used by
tests/golden/make_golden_tiles.py (which runs the genuine reference on the split FASTA) and by the tests, so both see the same bytes; the
manifest pins their SHA-256."""
import gzip
import hashlib
import json
import os

import numpy as np

import util

FIXTURES = ("vote", "k64", "ix32")
REF_BINARY = {"vote": "xtree-searchGG", "k64": "xtree-searchGG-k64", "ix32": "xtree-searchGG-ix32"}
PARAMS = {"vote": (150, 75), "k64": (200, 200), "ix32": (100, 33)}     # (W, S): an even overlap, none, an odd one
K = {"vote": 32, "k64": 64, "ix32": 32}
TILE_MAX_BP = 16777214


def n_tiles(L, W, S):
    """the closed form of the contract"""
    return 1 if L <= W else 1 + -(-(L - W) // S)


def tiles(L, W, S):
    """[(start, end)], 0-based and half open, by walking: a tile starts every S bases until one reaches the query's end"""
    out, a = [], 0
    while True:
        out.append((a, min(a + W, L)))
        if a + W >= L:
            return out
        a += S


def query_lengths(name):
    """the edges of the fixture's (W, S), and one query of about 3 kb"""
    W, S = PARAMS[name]
    k = K[name]
    return [1, k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 3 * W + 1, 3001]


def make_contigs(name):
    """[(name, sequence)]: reads of the fixture in a row, cut to the lengths of query_lengths(), with some N and lower-case stretches"""
    data = util.fixture_bytes(name + "_reads.fa.gz")
    _, off, ln = util.parse_fasta(data)
    rng = np.random.default_rng(20261021 + len(name))
    recs = []
    for qi, L in enumerate(query_lengths(name)):
        parts, have = [], 0
        while have < L:
            j = int(rng.integers(0, len(off)))
            s = data[int(off[j]):int(off[j]) + int(ln[j])]
            parts.append(s); have += len(s)
        seq = bytearray(b"".join(parts)[:L])
        if L > 40:
            for _ in range(1 + L // 700):
                seq[int(rng.integers(0, L))] = 0x4E                                    # an N breaks the windows across it
            for _ in range(1 + L // 1000):
                a = int(rng.integers(0, L - 20)); b = a + int(rng.integers(5, 120))
                seq[a:b] = bytes(seq[a:b]).lower()
        recs.append((b"ctg%d_len%d" % (qi, L), bytes(seq)))
    return recs


def fasta(recs):
    return b"".join(b">%s\n%s\n" % (n, s) for n, s in recs)


def parse(data):
    names, off, ln = util.parse_fasta(data)
    return [(n, data[int(o):int(o) + int(l)]) for n, o, l in zip(names, off, ln)]


def tile_name(name, a, b):
    """1-based, inclusive: the region syntax of samtools faidx"""
    return b"%s:%d-%d" % (name, a + 1, b)


def split_records(recs, W, S):
    """one record per tile, named <name>:<start>-<end>"""
    return [(tile_name(n, a, b), s[a:b]) for n, s in recs for a, b in tiles(len(s), W, S)]


class Tile:
    __slots__ = ("q", "t", "a", "b", "res", "line", "taxon")


def classify(o, recs, W, S, rc):
    """every tile as a read of its own through the CPU oracle: [Tile], in query order then tile order"""
    out = []
    for q, (n, s) in enumerate(recs):
        for t, (a, b) in enumerate(tiles(len(s), W, S)):
            x = Tile()
            x.q, x.t, x.a, x.b = q, t, a, b
            x.res = o.classify_read(s[a:b], rc=rc)
            x.line = o.format(tile_name(n, a, b), x.res) if x.res.found else b""
            x.taxon = x.line.split(b"\t")[1] if x.line else None                       # the TEXT the line prints: what a class is compared by
            out.append(x)
    return out


def tiles_tsv(tl):
    return b"".join(x.line for x in tl)


def segments_tsv(recs, tl):
    """maximal runs of consecutive tiles of one query and one class: both unclassified, or the same taxon text"""
    out, run = [], None
    for x in tl + [None]:
        if run is not None and (x is None or x.q != run[0] or x.taxon != run[4]):
            q, a, b, n, tax, found = run
            out.append(b"%s\t%d\t%d\t%d\t%s\t%s\t%d\n" % (recs[q][0], a + 1, b, n, b"U" if tax is None else b"C", tax or b"", found))
            run = None
        if x is None:
            break
        if run is None:
            run = [x.q, x.a, x.b, 1, x.taxon, int(x.res.found)]
        else:
            run[2] = x.b; run[3] += 1; run[5] += int(x.res.found)
    return b"".join(out)


def results_array(tl):
    """the tiles' results as the library's utree_result records"""
    from utree_amd.search import RESULT_DTYPE
    a = np.zeros(len(tl), dtype=RESULT_DTYPE)
    for i, x in enumerate(tl):
        a[i] = (x.res.label, x.res.cut, x.res.found, x.res.uix, x.res.sl, x.res.ol)
    return a


def numpy_views(off, ln, W, S):
    """(tile_first, toff, tlen, tquery, tindex) of a batch, restated with numpy"""
    ln64 = ln.astype(np.int64)
    cnt = np.where(ln64 <= W, 1, 1 + -(-(ln64 - W) // S)).astype(np.uint64) if len(ln) else np.zeros(0, dtype=np.uint64)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    tq = np.repeat(np.arange(len(ln), dtype=np.uint32), cnt.astype(np.int64))
    ti = (np.arange(int(first[-1]), dtype=np.uint64) - first[:-1][tq]).astype(np.uint32) if len(ln) else np.zeros(0, dtype=np.uint32)
    start = ti.astype(np.int64) * S
    tl = np.minimum(ln64[tq] - start, W).astype(np.uint32)
    return first, (off.astype(np.uint64)[tq] + start.astype(np.uint64)), tl, tq, ti


def plan_np(ln, W, S):
    """tile_first of a batch: uint64 [n + 1], exact past 2^32"""
    ln64 = np.asarray(ln).astype(np.uint64)
    cnt = np.uint64(1) + (np.maximum(ln64, np.uint64(W)) - np.uint64(W) + np.uint64(S - 1)) // np.uint64(S)
    first = np.zeros(len(ln64) + 1, dtype=np.uint64)
    np.cumsum(cnt, out=first[1:])
    return first


def views_range(off, ln, W, S, f0, n, first=None):
    """(toff, tlen, tquery, tindex) of tiles [f0, f0 + n) of a batch without materialising the batch: the query of tile g is the last one
    whose first tile is <= g (searchsorted on the uint64 cumulative sum), the rest is the closed form.  uint64 throughout: the batch's
    tiles, f0 and the offsets may lie past 2^32.  first: plan_np(ln, W, S), when the caller has it already."""
    first = plan_np(ln, W, S) if first is None else first
    assert 0 <= f0 and f0 + n <= int(first[-1])
    g = np.uint64(f0) + np.arange(n, dtype=np.uint64)
    q = np.searchsorted(first, g, "right") - 1
    t = g - first[q]
    start = t * np.uint64(S)
    tl = np.minimum(np.asarray(ln).astype(np.uint64)[q] - start, np.uint64(W))
    return np.asarray(off).astype(np.uint64)[q] + start, tl.astype(np.uint32), q.astype(np.uint32), t.astype(np.uint32)


# ---- the tiles of a batch classified as views, and their two files, without a Python step per tile ------------------------------------------

def classify_views(o, buf, toff, tlen, rc, threads=0):
    """the oracle on the views themselves: OracleDB.classify_batch takes any (off, len), so tiles that overlap in buf are reads like any
    other.  One utree_result record per tile."""
    return o.classify_batch(buf, toff, tlen, rc=rc, threads=threads)


def view_tiles(o, names, seq_len, W, S, tquery, tindex, res):
    """[Tile] of the views' records, as classify() gives them; o.format is called for tiles with `found` only.  For batches of a size at
    which a Python object per tile is affordable; view_files needs none."""
    out = []
    for j in range(len(res)):
        x = Tile()
        x.q, x.t = int(tquery[j]), int(tindex[j])
        x.a = x.t * S
        x.b = min(x.a + W, int(seq_len[x.q]))
        x.res = orc_result(res[j])
        x.line = o.format(tile_name(names[x.q], x.a, x.b), x.res) if x.res.found else b""
        x.taxon = x.line.split(b"\t")[1] if x.line else None
        out.append(x)
    return out


def orc_result(r):
    from oracle import orc
    return orc.Result(*[int(r[f]) for f in ("label", "cut", "found", "uix", "sl", "ol")])


def view_files(o, names, seq_len, W, S, tquery, tindex, res):
    """(tiles.tsv, segments.tsv, lines, segments) of the views' records: tiles_tsv and segments_tsv restated on arrays.  Python runs once
    per classified tile and once per segment; the runs themselves are found with numpy."""
    n = len(res)
    found = res["found"].astype(np.uint64)
    hit = np.flatnonzero(found > 0)
    lines, taxa, cls = [], {}, np.full(n, -1, dtype=np.int64)              # the class of a tile: -1 unclassified, else its taxon TEXT's number
    for j in hit:
        q, a = int(tquery[j]), int(tindex[j]) * S
        line = o.format(tile_name(names[q], a, min(a + W, int(seq_len[q]))), orc_result(res[j]))
        lines.append(line)
        cls[j] = taxa.setdefault(line.split(b"\t")[1], len(taxa))
    text = sorted(taxa, key=taxa.get)
    if n == 0:
        return b"", b"", 0, 0
    tq = np.asarray(tquery).astype(np.int64)
    head = np.flatnonzero(np.concatenate([[True], (tq[1:] != tq[:-1]) | (cls[1:] != cls[:-1])]))       # the first tile of every run
    last = np.concatenate([head[1:], [n]]) - 1
    L = np.asarray(seq_len).astype(np.int64)
    a = np.asarray(tindex).astype(np.int64)[head] * S + 1
    b = np.minimum(np.asarray(tindex).astype(np.int64)[last] * S + W, L[tq[last]])
    fsum = np.add.reduceat(found, head)
    seg = [b"%s\t%d\t%d\t%d\t%s\t%s\t%d\n" % (names[tq[h]], a[i], b[i], last[i] - h + 1, b"U" if cls[h] < 0 else b"C",
                                              b"" if cls[h] < 0 else text[cls[h]], fsum[i]) for i, h in enumerate(head)]
    return b"".join(lines), b"".join(seg), len(lines), len(seg)


# ---- contigs at the sizes the file run and the classify passes change their ways (tests/test_gpu_tiles_scale.py) ----------------------------

LANES_CAP, MID_CAP = 160, 2112                                             # csrc/utree_internal.h: UTREE_LANES_CAP, UTREE_MID_CAP


def lanes_cap(k, c):
    """csrc/lanes_kernel.hip: lanes_cap -- the bases a read of 2^c lanes holds"""
    return ((1 << c) - 1) * (LANES_CAP - k + 1) + LANES_CAP


def pieces_min_rc():
    """csrc/dev_image.c: lanes_long_min with both strands -- the last width whose two strands the wave-per-read pass stages"""
    return (MID_CAP - 1) // 2


def make_long_contigs(name, lengths, seed, islands=None):
    """[(name, sequence)] of the given lengths by make_contigs' recipe: reads of the fixture in a row with some N and lower-case stretches.
    islands: {contig number: [(position, read number), ...]} -- such a contig is uniformly random bases with those fixture reads pasted at
    those positions (cut at the contig's end), so that only the tiles on an island can hit."""
    data = util.fixture_bytes(name + "_reads.fa.gz")
    _, off, ln = util.parse_fasta(data)
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = []
    for qi, L in enumerate(lengths):
        if islands and qi in islands:
            seq = bytearray(acgt[rng.integers(0, 4, L)].tobytes())
            for pos, j in islands[qi]:
                s = data[int(off[j]):int(off[j]) + int(ln[j])][:L - pos]
                seq[pos:pos + len(s)] = s
        else:
            parts, have = [], 0
            while have < L:
                j = int(rng.integers(0, len(off)))
                s = data[int(off[j]):int(off[j]) + int(ln[j])]
                parts.append(s); have += len(s)
            seq = bytearray(b"".join(parts)[:L])
            if L > 40:
                for _ in range(1 + L // 700):
                    seq[int(rng.integers(0, L))] = 0x4E
                for _ in range(1 + L // 1000):
                    a = int(rng.integers(0, L - 20)); b = a + int(rng.integers(5, 120))
                    seq[a:b] = bytes(seq[a:b]).lower()
        recs.append((b"ctg%d_len%d" % (qi, L), bytes(seq)))
    return recs


PASS_LENGTHS = [120000, 1, 2095, 2096, 40000]
FILE_LENGTHS = [60000, 1, 33000]
FILE_WS = (64, 4)
SPLIT_TILES = (1 << 21) + 5000                                             # one contig, W = 32, S = 1: two sub-batches by the default split
SPLIT_WS = (32, 1)
SPLIT_ISLANDS = [(0, 2), ((1 << 21) - 40, 2), (SPLIT_TILES + 31 - 98, 1)]      # (reads 1 and 2: k-mers every 33 bases, an N between; the last ends the contig)
FRAMING_RECORD = 9                                                         # the record of the committed vote contigs whose '>' is broken


def pass_contigs():
    """test B's queries: one of 120 kb, the shortest there is, one on either side of sixteen lanes / pieces at k = 32, one of 40 kb"""
    return make_long_contigs("vote", PASS_LENGTHS, 20261022)


def pass_params(k):
    """{key: (W, S)}: the widths of test B that the reference was also run on"""
    return {"default": (1000, 500), "pieces": (lanes_cap(k, 4) + 1, 1000), "wide": (20000, 7001)}


def file_contigs():
    """test C's queries; the first one's name is 300 bytes long, which makes tiles.tsv several MiB"""
    recs = make_long_contigs("vote", FILE_LENGTHS, 20261023)
    return [(recs[0][0] + b"_" + b"x" * (299 - len(recs[0][0])), recs[0][1])] + recs[1:]


def split_contig():
    """one query of SPLIT_TILES tiles at SPLIT_WS, random but for three fixture reads: at its start, across tile 2^21 and at its end"""
    return make_long_contigs("vote", [SPLIT_TILES + SPLIT_WS[0] - 1], 20261024, islands={0: SPLIT_ISLANDS})


def framed_arrays(recs):
    """(FASTA bytes as uint8, names, seq_off, seq_len) of two-line records, as the framing gives them"""
    data = fasta(recs)
    names, off, ln = util.parse_fasta(data)
    return np.frombuffer(data, dtype=np.uint8), names, off, ln


def broken_header(data, record):
    """the FASTA with the '>' of its record `record` (1-based) replaced"""
    lines = data.split(b"\n")
    i = 2 * (record - 1)
    assert lines[i].startswith(b">")
    return b"\n".join(lines[:i] + [b"no_header_here"] + lines[i + 1:])


def manifest():
    return json.load(open(os.path.join(util.GOLD, "tiles_manifest.json")))


def golden(name, rc):
    """the genuine reference's output on the split FASTA of the committed contigs (make_golden_tiles.py)"""
    return util.fixture_bytes("tiles_%s_out%s.txt.gz" % (name, "_rc" if rc else ""))


def contigs(name):
    """the committed contigs; they must be the ones make_contigs() builds"""
    return util.fixture_bytes("tiles_%s_contigs.fa.gz" % name)


def sha256(b):
    return hashlib.sha256(b).hexdigest()


def gz(b):
    return gzip.compress(b, 1)
