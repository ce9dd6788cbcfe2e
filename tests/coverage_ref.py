"""The coverage contract in plain Python: (.ctr, reads, rc) -> coverage file bytes.  Uses only the CPU oracle and the .ctr reader."""
import hashlib
import numpy as np
from oracle import orc
from utree_amd import ctrfile

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def probe(d, suf, hi, lo):
    """itree.c:720-730 with 699-707 over the node dump: position of the record the lookup ends on, or -1"""
    if d.W == 8: p, q = lo >> 40, lo & ((1 << 40) - 1)
    elif d.W == 16: p, q = hi >> 40, ((hi & ((1 << 40) - 1)) << 64) | lo
    else: p, q = lo >> 8, lo & 0xFF
    s, e = int(d.binix[p]), int(d.binix[p + 1])
    if s >= e:
        return -1
    pos, size = s, e - s - 1
    while size:
        w = size >> 1
        if suf[pos + w + 1] <= q: pos, size = pos + w + 1, size - w - 1
        else: size = w
    return pos if suf[pos] == q else -1


def coverage_counts(ctr_path, seqs, rc):
    """per label index: db_kmers, covered, hits (numpy int64 arrays), and the label texts"""
    o = orc.OracleDB.load(ctr_path)
    d = ctrfile.read_ctr(ctr_path)
    nl = o.n_labels
    shi, slo = d.suffixes()
    suf = [(int(h) << 64) | int(l) for h, l in zip(shi.tolist(), slo.tolist())]
    ix = d.ix()
    db = np.bincount(ix[ix < nl].astype(np.int64), minlength=nl)
    hits = np.zeros(nl, dtype=np.int64)
    nodes = set()
    for s in seqs:
        q = s + b"N" + s[::-1].translate(COMP) if rc else s       # non-ACGT bytes stay non-ACGT: they break windows on both strands
        _, hi, lo = orc.windows(q, o.k)
        for h, l in zip(hi.tolist(), lo.tolist()):
            lab = o.lookup(h, l)
            if lab < nl:
                p = probe(d, suf, h, l)
                assert p >= 0 and int(ix[p]) == lab
                hits[lab] += 1
                nodes.add(p)
    cov = np.bincount(ix[sorted(nodes)].astype(np.int64), minlength=nl) if nodes else np.zeros(nl, dtype=np.int64)
    return db, cov, hits, [o.label(i) for i in range(nl)]


def coverage_counts_batch(ctr_path, seqs, rc):
    """coverage_counts() with one lookup call per read (OracleDB.lookup_batch gives label and record position): for reads of millions of
    windows.  seqs: bytes or uint8 arrays."""
    import hitmap_ref
    o = orc.OracleDB.load(ctr_path)
    d = ctrfile.read_ctr(ctr_path)
    nl = o.n_labels
    ix = d.ix()
    db = np.bincount(ix[ix < nl].astype(np.int64), minlength=nl)
    hits = np.zeros(nl, dtype=np.int64)
    seen = np.zeros(len(ix), dtype=bool)
    for s in seqs:
        _, hi, lo = orc.windows(hitmap_ref.query_array(s, rc), o.k)
        lab, pos = o.lookup_batch(hi, lo, positions=True)
        hit = lab < nl
        assert (pos[hit] >= 0).all() and np.array_equal(ix[pos[hit]], lab[hit])
        hits += np.bincount(lab[hit].astype(np.int64), minlength=nl)
        seen[pos[hit]] = True
    cov = np.bincount(ix[seen].astype(np.int64), minlength=nl)
    return db, cov, hits, [o.label(i) for i in range(nl)]


def coverage_file(db, cov, hits, texts, n_reads):
    own, clade = {}, {}
    for t, a, b, c in zip(texts, db.tolist(), cov.tolist(), hits.tolist()):
        r = own.setdefault(t, [0, 0, 0]); r[0] += a; r[1] += b; r[2] += c
    rows = set()
    for t, r in own.items():
        if r[2]:
            rows.add(t)
            rows.update(t[:i] for i, ch in enumerate(t) if ch == 0x3B)
    for t, r in own.items():                                         # every label of the database, hit or not
        for s in [t] + [t[:i] for i, ch in enumerate(t) if ch == 0x3B]:
            if s in rows:
                c = clade.setdefault(s, [0, 0, 0]); c[0] += r[0]; c[1] += r[1]; c[2] += r[2]
    out = [b"# reads\t%d\thits\t%d\tcovered\t%d\tdb_kmers\t%d\n# taxon\tdb_kmers\tcovered\thits\tclade_db_kmers\tclade_covered\tclade_hits\n"
           % (n_reads, int(hits.sum()), int(cov.sum()), int(db.sum()))]
    for s in sorted(rows):
        a = own.get(s, [0, 0, 0])
        out.append(b"%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (s, a[0], a[1], a[2], clade[s][0], clade[s][1], clade[s][2]))
    return b"".join(out)
