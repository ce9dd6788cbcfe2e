"""The hit-map contract (include/utree_amd.h, utree_hitmap_*) in plain Python: (.ctr, queries, rc) -> per query its list of runs, and the
bytes of the hit-map file and of its .labels.  Uses only the CPU oracle: orc.windows for the valid windows, OracleDB.lookup per window."""
import numpy as np

from oracle import orc

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
MISS, INVALID = 0xFFFFFFFF, 0xFFFFFFFE


def query(seq, rc):
    """the byte string the reference searches (itree.c:891-898); non-ACGT bytes stay non-ACGT under reverse complement: they break the
    windows of both strands (coverage_ref / pairs_ref conventions: a pair is joined BEFORE this, seq1 + b"N" + seq2)"""
    return seq + b"N" + seq[::-1].translate(COMP) if rc else seq


def codes(o, seq, rc):
    """one code per window of the query, in window order (numpy uint32)"""
    q, k = query(seq, rc), o.k
    n = len(q) - k + 1 if len(q) >= k else 0
    out = np.full(n, INVALID, dtype=np.uint32)
    if n:
        # orc.windows gives the position of a window's LAST base (utree_oracle.c: for_each_window calls back with end_pos = i, the index
        # of the base that completes the window), so the window starts at pos - k + 1
        pos, hi, lo = orc.windows(q, k)
        nl = o.n_labels
        for p, h, l in zip(pos.tolist(), hi.tolist(), lo.tolist()):
            ix = o.lookup(h, l)
            out[p - k + 1] = ix if ix < nl else MISS
    return out


def query_array(seq, rc):
    """query() on a uint8 array (bytes are taken too): no Python object per base"""
    s = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else seq
    if not rc:
        return s
    comp = np.arange(256, dtype=np.uint8)
    comp[np.frombuffer(b"ACGTacgt", dtype=np.uint8)] = np.frombuffer(b"TGCAtgca", dtype=np.uint8)
    return np.concatenate([s, np.frombuffer(b"N", dtype=np.uint8), comp[s[::-1]]])


def codes_batch(o, seq, rc):
    """codes() with one lookup call for all windows (OracleDB.lookup_batch): for reads of millions of windows"""
    q, k = query_array(seq, rc), o.k
    n = len(q) - k + 1 if len(q) >= k else 0
    out = np.full(n, INVALID, dtype=np.uint32)
    if n:
        pos, hi, lo = orc.windows(q, k)
        ix = o.lookup_batch(hi, lo)
        out[pos.astype(np.int64) - (k - 1)] = np.where(ix < o.n_labels, ix, MISS).astype(np.uint32)
    return out


def runs_arrays(c):
    """runs_of() as arrays (code uint32, count int64)"""
    if not len(c):
        return np.zeros(0, np.uint32), np.zeros(0, np.int64)
    cut = np.flatnonzero(c[1:] != c[:-1]) + 1
    starts = np.concatenate([[0], cut])
    return c[starts], np.diff(np.concatenate([starts, [len(c)]]))


def runs_of(c):
    """maximal stretches of equal code: [(code, count), ...]"""
    if not len(c):
        return []
    cut = np.flatnonzero(c[1:] != c[:-1]) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(c)]])
    return [(int(c[a]), int(b - a)) for a, b in zip(starts.tolist(), ends.tolist())]


def hitmap(ctr_path, seqs, rc, o=None):
    """[runs of query 0, runs of query 1, ...]"""
    o = o or orc.OracleDB.load(ctr_path)
    return [runs_of(codes(o, s, rc)) for s in seqs]


def flat(maps):
    """(run_off [n + 1], runs [total, 2] as (code, count)) the way utree_hitmap_batch lays them out"""
    off = np.zeros(len(maps) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(m) for m in maps])
    runs = np.array([r for m in maps for r in m], dtype=np.uint32).reshape(-1, 2)
    return off, runs


def found_uix(runs):
    """(column 3, column 4) of the query's output line: hit windows, distinct hit labels"""
    hit = [(c, n) for c, n in runs if c < INVALID]
    return sum(n for _, n in hit), len({c for c, _ in hit})


def token(code, count):
    return b"%s:%d" % (b"-" if code == MISS else b"N" if code == INVALID else b"%d" % code, count)


def file_bytes(names, maps):
    """one line for EVERY query: name \\t n_windows \\t found \\t tokens \\n"""
    return b"".join(b"%s\t%d\t%d\t%s\n" % (nm, sum(n for _, n in m), found_uix(m)[0], b" ".join(token(c, n) for c, n in m))
                    for nm, m in zip(names, maps))


def labels_bytes(ctr_path, o=None):
    """<hitmap>.labels: line i is the text of label index i"""
    o = o or orc.OracleDB.load(ctr_path)
    return b"".join(o.label(i) + b"\n" for i in range(o.n_labels))
