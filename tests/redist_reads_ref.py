"""Each read's redistributed label (include/utree_amd.h: utree_redist_assign, utree_redist_reads_format) in plain Python, on top of
tests/redist_ref.py: candidate sets per read -> the label every read is assigned to after the passes, and the report's bytes.  Uses only the
CPU oracle."""
from collections import Counter

import redist_ref


def assign(sets, n_reads, max_passes=100):
    """sets: per read the sorted tuple of candidates, () without a hit.  -> (label per read or None, candidates per read, T_P):
    label = win(set, T_P), T_P the tally after the last pass run -- redist_ref.solve's loop, repeated so that the final tally is at hand."""
    ms = redist_ref.multiset(sets)
    tally = Counter()
    for s, n in ms.items():
        for l in s:
            tally[l] += n
    passes = 0
    while True:
        nxt = Counter()
        for s, n in ms.items():
            nxt[redist_ref.win(s, tally)] += n
        ch = sum(abs(nxt.get(l, 0) - tally.get(l, 0)) for l in set(nxt) | set(tally))
        tally = nxt
        passes += 1
        if passes >= max_passes or ch <= n_reads // 100000:
            break
    winner = {s: redist_ref.win(s, tally) for s in ms}
    labels = [winner[s] if s else None for s in sets]
    ncand = [len(s) for s in sets]
    # the per-read labels are the reads redist_ref.solve counts: the same histogram, label by label
    a, u, p, _, _ = redist_ref.solve(sets, n_reads, max_passes)
    assert p == passes
    assert Counter(l for l in labels if l is not None) == +a
    assert Counter(l for l, c in zip(labels, ncand) if c == 1) == +u
    return labels, ncand, tally


def reads_file(names, labels, ncand, texts):
    """one line per read that has a label: name, the label's whole text, its number of candidates"""
    return b"".join(b"%s\t%s\t%d\n" % (nm, texts[l], c) for nm, l, c in zip(names, labels, ncand) if l is not None)
