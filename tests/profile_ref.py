"""The profile contract (include/utree_amd.h, utree_profile_write) in plain Python: per-read output bytes -> profile bytes.

A read's taxon is the second column of its output line; a read without a line is unclassified.  The line's read name is known
from the input (names in read order), so the taxon is what follows that name and one TAB -- a name may itself hold a TAB
(the reference's name ends at the first space, itree.c:881), so the line is not split at its first TAB."""
from collections import Counter


def line_taxa(out: bytes, names) -> list:
    taxa, j = [], 0
    for line in out.split(b"\n")[:-1]:
        while not line.startswith(names[j] + b"\t"):
            j += 1
        taxa.append(line[len(names[j]) + 1:].split(b"\t", 1)[0])
        j += 1
    return taxa


def profile_from_taxa(taxa, n_reads: int) -> bytes:
    assigned = Counter(taxa)
    rows = {}                                                    # text -> [assigned, clade]
    for t, a in assigned.items():
        rows.setdefault(t, [0, 0])[0] += a
        rows[t][1] += a
        for i, ch in enumerate(t):
            if ch == 0x3B:                                       # every ';'-prefix: t starts with prefix + ";"
                rows.setdefault(t[:i], [0, 0])[1] += a
    g = sum(assigned.values())
    out = [b"# reads\t%d\tclassified\t%d\tunclassified\t%d\n# taxon\tassigned\tclade\n" % (n_reads, g, n_reads - g)]
    for s in sorted(rows):                                       # bytes order: unsigned bytewise, shorter first on a tie
        out.append(b"%s\t%d\t%d\n" % (s, rows[s][0], rows[s][1]))
    return b"".join(out)


def profile_ref(out: bytes, names, n_reads: int) -> bytes:
    return profile_from_taxa(line_taxa(out, names), n_reads)


def fasta_names(data: bytes) -> list:
    """read names in order as the reference takes them (itree.c:866-881): two lines per read, the name is the header line after its
    '>' up to the first space, newline or NUL.  Written out here rather than taken from the framing under test."""
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines.pop()
    names = []
    for i in range(0, len(lines) - 1, 2):
        name = lines[i][1:]
        for stop in (b" ", b"\0"):
            j = name.find(stop)
            if j >= 0:
                name = name[:j]
        names.append(name)
    return names
