"""The redistribution contract (include/utree_amd.h, utree_redist_*) in plain Python: (.ctr, reads, rc) -> candidate sets -> passes ->
redistribution file bytes.  Uses only the CPU oracle."""
from collections import Counter

from oracle import orc

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def candidate_sets(ctr_path, seqs, rc):
    """per read (or joined pair) the sorted tuple of file-order label indices tied for its highest hit count; () without a hit.
    Returns (sets, label texts)."""
    o = orc.OracleDB.load(ctr_path)
    nl = o.n_labels
    sets = []
    for s in seqs:
        q = s + b"N" + s[::-1].translate(COMP) if rc else s       # non-ACGT bytes stay non-ACGT: they break windows on both strands
        _, hi, lo = orc.windows(q, o.k)
        c = Counter()
        for h, l in zip(hi.tolist(), lo.tolist()):
            lab = o.lookup(h, l)
            if lab < nl:
                c[lab] += 1
        top = max(c.values()) if c else 0
        sets.append(tuple(sorted(l for l, v in c.items() if v == top)))
    return sets, [o.label(i) for i in range(nl)]


def multiset(sets):
    """{sorted set: reads} over the reads that have a candidate"""
    return Counter(s for s in sets if s)


def win(s, tally):
    """the richest candidate; on equal tallies the smallest file-order index"""
    best = s[0]
    for l in s[1:]:
        if tally.get(l, 0) > tally.get(best, 0) or (tally.get(l, 0) == tally.get(best, 0) and l < best):
            best = l
    return best


def solve(sets, n_reads, max_passes=100):
    """-> (assigned, unique, passes, ambiguous, changes): Counters by label index, the passes run, reads with more than one candidate,
    the list of every pass's `changes`"""
    ms = multiset(sets)
    tally = Counter()
    for s, n in ms.items():
        for l in s:
            tally[l] += n
    changes, passes = [], 0
    while True:
        nxt = Counter()
        for s, n in ms.items():
            nxt[win(s, tally)] += n
        ch = sum(abs(nxt.get(l, 0) - tally.get(l, 0)) for l in set(nxt) | set(tally))
        tally = nxt
        passes += 1
        changes.append(ch)
        if passes >= max_passes or ch <= n_reads // 100000:
            break
    assigned, unique = Counter(), Counter()
    for s, n in ms.items():
        assigned[win(s, tally)] += n                                # one more evaluation, not T_P itself
        if len(s) == 1:
            unique[s[0]] += n
    ambiguous = sum(n for s, n in ms.items() if len(s) > 1)
    return assigned, unique, passes, ambiguous, changes


def redist_file(assigned, unique, texts, n_reads, ambiguous, passes):
    """assigned / unique: {label index: reads}"""
    own, clade = {}, {}
    for l in set(assigned) | set(unique):
        r = own.setdefault(texts[l], [0, 0]); r[0] += assigned.get(l, 0); r[1] += unique.get(l, 0)
    rows = set()
    for t, r in own.items():
        if r[0]:
            rows.add(t)
            rows.update(t[:i] for i, ch in enumerate(t) if ch == 0x3B)
    for t, r in own.items():
        for s in [t] + [t[:i] for i, ch in enumerate(t) if ch == 0x3B]:
            if s in rows:
                c = clade.setdefault(s, [0, 0]); c[0] += r[0]; c[1] += r[1]
    g = sum(assigned.values())
    out = [b"# reads\t%d\tclassified\t%d\tunclassified\t%d\tambiguous\t%d\tpasses\t%d\n# taxon\tassigned\tunique\tclade_assigned\tclade_unique\n"
           % (n_reads, g, n_reads - g, ambiguous, passes)]
    for s in sorted(rows):
        a = own.get(s, [0, 0])
        out.append(b"%s\t%d\t%d\t%d\t%d\n" % (s, a[0], a[1], clade[s][0], clade[s][1]))
    return b"".join(out)


def reference_file(ctr_path, seqs, rc, max_passes=100):
    sets, texts = candidate_sets(ctr_path, seqs, rc)
    assigned, unique, passes, ambiguous, _ = solve(sets, len(seqs), max_passes)
    return redist_file(assigned, unique, texts, len(seqs), ambiguous, passes)
