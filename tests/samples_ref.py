"""The sample-table contract (include/utree_amd.h, utree_samples_write) in plain Python:
(per-read output bytes, names in read order, n_reads, delimiter) -> table bytes.

A read's sample id is its name up to the LAST delimiter byte (the whole name without one; it may be empty); its taxon is the second column of
its output line (profile_ref.line_taxa), a read without a line is unclassified.  Written from the header's text, not from the code under test."""
from collections import Counter

from profile_ref import line_taxa


def sample_id(name: bytes, delim: bytes = b"_") -> bytes:
    i = name.rfind(delim)
    return name if i < 0 else name[:i]


def escape_id(s: bytes) -> bytes:
    return s.replace(b"\\", b"\\\\").replace(b"\t", b"\\t").replace(b"\r", b"\\r")


def lines_of(out: bytes, names) -> list:
    """index into `names` of the read each output line belongs to (the walk of profile_ref.line_taxa: lines are in read order and begin
    with their read's name and a TAB)"""
    idx, j = [], 0
    for line in out.split(b"\n")[:-1]:
        while not line.startswith(names[j] + b"\t"):
            j += 1
        idx.append(j)
        j += 1
    return idx


def table_from(ids, taxa_of_classified, n_reads: int) -> bytes:
    """ids: the sample id of every read, in read order; taxa_of_classified: [(read index, taxon)] of the reads with a line"""
    assert len(ids) == n_reads
    n = Counter(ids)
    cells = Counter((t, ids[r]) for r, t in taxa_of_classified)
    cl = Counter(ids[r] for r, _ in taxa_of_classified)
    samples = sorted(n)                                          # bytes order: unsigned bytewise, shorter first on a tie
    taxa = sorted({t for t, _ in cells})
    g = len(taxa_of_classified)

    def row(first, vals):
        return first + b"".join(b"\t" + v for v in vals) + b"\n"
    out = [b"# reads\t%d\tclassified\t%d\tunclassified\t%d\tsamples\t%d\n" % (n_reads, g, n_reads - g, len(samples)),
           row(b"# taxon", [escape_id(s) for s in samples]),
           row(b"# reads", [b"%d" % n[s] for s in samples]),
           row(b"# unclassified", [b"%d" % (n[s] - cl[s]) for s in samples])]
    for t in taxa:
        out.append(row(t, [b"%d" % cells[(t, s)] for s in samples]))
    return b"".join(out)


def samples_ref(out: bytes, names, n_reads: int, delim: bytes = b"_") -> bytes:
    assert len(names) == n_reads
    idx = lines_of(out, names)
    taxa = line_taxa(out, names)
    assert len(idx) == len(taxa)
    return table_from([sample_id(nm, delim) for nm in names], list(zip(idx, taxa)), n_reads)


def parse_table(tab: bytes):
    """(N, G, S, ids as printed, n_j, u_j, {taxon: [c_j]}) of a table file"""
    lines = tab.split(b"\n")
    assert lines[-1] == b"" and len(lines) >= 5
    h = lines[0].split(b"\t")
    assert h[0] == b"# reads" and h[2] == b"classified" and h[4] == b"unclassified" and h[6] == b"samples" and len(h) == 8
    N, G, U, S = int(h[1]), int(h[3]), int(h[5]), int(h[7])
    assert U == N - G
    ids, n, u = lines[1].split(b"\t"), lines[2].split(b"\t"), lines[3].split(b"\t")
    assert ids[0] == b"# taxon" and n[0] == b"# reads" and u[0] == b"# unclassified"
    assert len(ids) == len(n) == len(u) == S + 1
    rows = {}
    for ln in lines[4:-1]:
        f = ln.split(b"\t")
        assert len(f) >= S + 1
        taxon = b"\t".join(f[:len(f) - S])                      # (a taxon could hold a TAB; the S counts are the last S fields)
        assert taxon not in rows
        rows[taxon] = [int(x) for x in f[len(f) - S:]]
    return N, G, S, ids[1:], [int(x) for x in n[1:]], [int(x) for x in u[1:]], rows


def check_invariants(tab: bytes):
    """what the header says a reader can check of the file alone; returns the parsed table"""
    N, G, S, ids, n, u, rows = p = parse_table(tab)
    assert sum(n) == N
    for j in range(S):
        assert sum(r[j] for r in rows.values()) == n[j] - u[j]
    assert sum(sum(r) for r in rows.values()) == G
    assert all(sum(r) > 0 for r in rows.values())
    assert list(rows) == sorted(rows)
    return p


def rename_reads(data: bytes, out: bytes, old_names, new_names):
    """A two-lines-per-read FASTA and its per-read output under other read names: the name only reaches column 1 of the output, so the
    expected output of the renamed reads is the given output with the names substituted."""
    assert len(old_names) == len(new_names)
    lines = data.split(b"\n")
    for i, (o, nw) in enumerate(zip(old_names, new_names)):
        assert lines[2 * i][1:1 + len(o)] == o
        lines[2 * i] = b">" + nw + lines[2 * i][1 + len(o):]
    outl = out.split(b"\n")
    for k, j in enumerate(lines_of(out, old_names)):
        outl[k] = new_names[j] + outl[k][len(old_names[j]):]
    return b"\n".join(lines), b"\n".join(outl)


def round_robin_names(n: int, samples):
    return [samples[i % len(samples)] + b"_%d" % i for i in range(n)]


def block_names(n: int, samples):
    per = (n + len(samples) - 1) // len(samples)
    return [samples[i // per] + b"_%d" % i for i in range(n)]


SEVEN = [b"PlateA.well7", b"PlateA.well8", b"ctrl", b"s_1", b"s_10", b"x", b"neg.ctrl-2"]
