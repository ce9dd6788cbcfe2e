"""The per-sample redistribution contract (include/utree_amd.h, utree_sredist_*) in plain Python:
(.ctr, reads, names, rc, delimiter) -> candidate sets -> every sample solved on its own -> file bytes.  Uses only the CPU oracle.

Restated from the header:
  sample id      the printed name before its LAST delimiter byte (samples_ref.sample_id); a name without it is its own id; an id may be empty
  candidate set  { l : c[l] == max c } over file-order label indices (redist_ref.candidate_sets); () without a hit
  per sample s   redist_ref.solve on the sample's reads R_s alone, N_s = |R_s| in the stopping rule: a sample stops on its own, P_s is its own
                 pass count; assigned_s is one more evaluation under T_{P_s}
  file           '#' lines: totals; ids; reads; unclassified; ambiguous; passes -- then one line per label TEXT with assigned > 0 in some sample,
                 samples and taxa in bytes order, ids escaped as the sample table escapes them, no ';'-prefix rows
"""
from collections import Counter

import redist_ref
from samples_ref import escape_id, sample_id

THREE = [b"PlateA.well7", b"s_1", b"ctrl"]


def deal_names(n, deal, samples=THREE):
    """names <sample>_<i> of n reads dealt to the samples in blocks (i * S // n) or round-robin (i % S)"""
    S = len(samples)
    return [samples[i * S // n if deal == "block" else i % S] + b"_%d" % i for i in range(n)]


def by_sample(sets, ids):
    """{sample id: the candidate sets of its reads, in read order}"""
    out = {}
    for s, i in zip(sets, ids):
        out.setdefault(i, []).append(s)
    return out


def solve(sets, ids, max_passes=100):
    """{sample id: (assigned, unique, passes, ambiguous, n_reads)} -- every sample's reads solved as if they were the reads searched"""
    out = {}
    for i, ss in by_sample(sets, ids).items():
        a, u, p, amb, _ = redist_ref.solve(ss, len(ss), max_passes)
        out[i] = (a, u, p, amb, len(ss))
    return out


def solve_multiset(ms, n_reads, max_passes=100):
    """redist_ref.solve on a multiset {sorted set: reads} instead of a list of reads (the same loop: counts too large to write out as reads);
    -> (assigned, unique, passes, ambiguous)"""
    tally = Counter()
    for s, c in ms.items():
        for l in s:
            tally[l] += c
    passes = 0
    while True:
        nxt = Counter()
        for s, c in ms.items():
            nxt[redist_ref.win(s, tally)] += c
        ch = sum(abs(nxt.get(l, 0) - tally.get(l, 0)) for l in set(nxt) | set(tally))
        tally = nxt
        passes += 1
        if passes >= max_passes or ch <= n_reads // 100000:
            break
    assigned, unique = Counter(), Counter()
    for s, c in ms.items():
        assigned[redist_ref.win(s, tally)] += c
        if len(s) == 1:
            unique[s[0]] += c
    return assigned, unique, passes, sum(c for s, c in ms.items() if len(s) > 1)


def multisets(sets, ids):
    """{sample id: {sorted set: reads}}, every sample a key (a sample of unclassified reads has an empty multiset)"""
    return {i: dict(redist_ref.multiset(ss)) for i, ss in by_sample(sets, ids).items()}


def pooled_assignment(sets, ids, max_passes=100):
    """{sample id: Counter(label -> reads)} when every read is assigned under the POOLED final tally: what combining the two existing
    reports would have to mean, and not what this report writes"""
    n = len(sets)
    ms = redist_ref.multiset(sets)
    tally = Counter()
    for s, c in ms.items():
        for l in s:
            tally[l] += c
    passes = 0
    while True:
        nxt = Counter()
        for s, c in ms.items():
            nxt[redist_ref.win(s, tally)] += c
        ch = sum(abs(nxt.get(l, 0) - tally.get(l, 0)) for l in set(nxt) | set(tally))
        tally = nxt
        passes += 1
        if passes >= max_passes or ch <= n // 100000:
            break
    out = {}
    for s, i in zip(sets, ids):
        c = out.setdefault(i, Counter())
        if s:
            c[redist_ref.win(s, tally)] += 1
    return out, passes


def table_bytes(solved, texts):
    """solved: {sample id: (assigned {label index: reads}, unique, passes, ambiguous, n_reads)}"""
    samples = sorted(solved)                                     # bytes order: unsigned bytewise, shorter first on a tie
    N = sum(v[4] for v in solved.values())
    G = sum(sum(v[0].values()) for v in solved.values())
    A = sum(v[3] for v in solved.values())
    cells = Counter()
    for i, v in solved.items():
        for l, r in v[0].items():
            if r:
                cells[(texts[l], i)] += r                        # labels of equal text are one row
    taxa = sorted({t for t, _ in cells})

    def row(first, vals):
        return first + b"".join(b"\t" + v for v in vals) + b"\n"
    out = [b"# reads\t%d\tclassified\t%d\tunclassified\t%d\tambiguous\t%d\tsamples\t%d\n" % (N, G, N - G, A, len(samples)),
           row(b"# taxon", [escape_id(s) for s in samples]),
           row(b"# reads", [b"%d" % solved[s][4] for s in samples]),
           row(b"# unclassified", [b"%d" % (solved[s][4] - sum(solved[s][0].values())) for s in samples]),
           row(b"# ambiguous", [b"%d" % solved[s][3] for s in samples]),
           row(b"# passes", [b"%d" % solved[s][2] for s in samples])]
    for t in taxa:
        out.append(row(t, [b"%d" % cells[(t, s)] for s in samples]))
    return b"".join(out)


def file_from_sets(sets, texts, names, delim=b"_", max_passes=100):
    return table_bytes(solve(sets, [sample_id(nm, delim) for nm in names], max_passes), texts)


def reference_file(ctr_path, seqs, names, rc, delim=b"_", max_passes=100):
    sets, texts = redist_ref.candidate_sets(ctr_path, seqs, rc)
    return file_from_sets(sets, texts, names, delim, max_passes)


def parse(tab):
    """(N, G, A, S, ids as printed, n_j, u_j, a_j, P_j, {taxon: [assigned_j]}) of a file"""
    lines = tab.split(b"\n")
    assert lines[-1] == b"" and len(lines) >= 7
    h = lines[0].split(b"\t")
    assert h[0::2] == [b"# reads", b"classified", b"unclassified", b"ambiguous", b"samples"] and len(h) == 10
    N, G, U, A, S = (int(x) for x in h[1::2])
    assert U == N - G
    heads = [ln.split(b"\t") for ln in lines[1:6]]
    assert [x[0] for x in heads] == [b"# taxon", b"# reads", b"# unclassified", b"# ambiguous", b"# passes"]
    assert all(len(x) == S + 1 for x in heads)
    rows = {}
    for ln in lines[6:-1]:
        f = ln.split(b"\t")
        taxon = b"\t".join(f[:len(f) - S])
        assert taxon not in rows and not taxon.startswith(b"#")
        rows[taxon] = [int(x) for x in f[len(f) - S:]]
    ints = lambda x: [int(v) for v in x[1:]]
    return N, G, A, S, heads[0][1:], ints(heads[1]), ints(heads[2]), ints(heads[3]), ints(heads[4]), rows


def check_invariants(tab):
    """what the header says a reader can check of the file alone; returns the parsed file"""
    N, G, A, S, ids, n, u, a, P, rows = p = parse(tab)
    assert sum(n) == N and sum(a) == A
    for j in range(S):
        assert sum(r[j] for r in rows.values()) == n[j] - u[j]                # column j sums to n_j - u_j
        assert a[j] <= n[j] - u[j] and P[j] >= 1
    assert sum(sum(r) for r in rows.values()) == G
    assert all(sum(r) > 0 for r in rows.values()) and list(rows) == sorted(rows)
    return p
