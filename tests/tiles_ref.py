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
