"""Paired-end inputs made from a fixture's reads, and the pair contract in plain Python (include/utree_amd.h, utree_search_pairs_file):
read i of the fixture is mate 1 of pair i, read i + n // 2 its mate 2, and the pair's answer is that of the single query named by mate 1
whose sequence is seq1 + "N" + seq2.  Used by tests/golden/make_golden_pairs.py (which runs the genuine reference on the joined FASTA)
and by the tests, so both see the same bytes; the manifest pins their SHA-256."""
import gzip
import hashlib
import json
import os

import numpy as np

import util

FIXTURES = ("toy", "vote", "k64")
REF_BINARY = {"toy": "xtree-searchGG", "vote": "xtree-searchGG", "k64": "xtree-searchGG-k64"}


class Pairs:
    def __init__(self, name):
        data = util.fixture_bytes(name + "_reads.fa.gz")
        names, off, ln = util.parse_fasta(data)
        h = len(names) // 2
        seqs = [data[int(o):int(o) + int(l)] for o, l in zip(off, ln)]
        self.name, self.n = name, h
        self.names1, self.names2 = names[:h], names[h:2 * h]
        self.seq1, self.seq2 = seqs[:h], seqs[h:2 * h]

    def joined_seqs(self):
        return [a + b"N" + b for a, b in zip(self.seq1, self.seq2)]

    def joined_fasta(self, n=None):
        """what the reference is run on: one record per pair, mate 1's name"""
        return b"".join(b">%s\n%s\n" % (nm, s) for nm, s in list(zip(self.names1, self.joined_seqs()))[:n])

    # mate 2's headers are deliberately longer than mate 1's (and carry text behind a space): the two files' chunks fall out of step
    def reads_fasta(self, n=None):
        return b"".join(b">%s\n%s\n" % (nm, s) for nm, s in list(zip(self.names1, self.seq1))[:n])

    def mates_fasta(self, n=None):
        return b"".join(b">%s/2 the second mate of pair %d, with a longer header\n%s\n" % (nm, i, s)
                        for i, (nm, s) in enumerate(list(zip(self.names2, self.seq2))[:n]))

    def interleaved_fasta(self, n_records=None):
        recs = []
        for i in range(self.n):
            recs.append(b">%s\n%s\n" % (self.names1[i], self.seq1[i]))
            recs.append(b">%s/2 mate\n%s\n" % (self.names2[i], self.seq2[i]))
        return b"".join(recs[:n_records])

    def reads_fastq(self):
        return b"".join(b"@%s 1:N:0\n%s\n+\n%s\n" % (nm, s, b"I" * len(s)) for nm, s in zip(self.names1, self.seq1))

    def mates_fastq(self):
        return b"".join(b"@%s 2:N:0 and more header text\n%s\n+%s\n%s\n" % (nm, s, nm, b"#" * len(s)) for nm, s in zip(self.names2, self.seq2))


def wrap(fasta, width):
    """the same records as multi-line FASTA: sequence lines of at most `width` bytes (an empty sequence keeps its empty line)"""
    out = []
    for rec in fasta.split(b">")[1:]:
        hdr, seq = rec.split(b"\n", 1)
        seq = seq.rstrip(b"\n")
        out.append(b">" + hdr + b"\n" + (b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width)) or b"\n"))
    return b"".join(out)


def numpy_join(blob1, off1, len1, blob2, off2, len2):
    """(joined bytes, joff, jlen): mate 1 + 'N' + mate 2 per pair, tight -- the join restated with numpy, one pair at a time"""
    b1, b2 = np.frombuffer(blob1, dtype=np.uint8), np.frombuffer(blob2, dtype=np.uint8)
    jlen = len1.astype(np.uint64) + 1 + len2.astype(np.uint64)
    joff = np.concatenate([[0], np.cumsum(jlen)[:-1]]).astype(np.uint64) if len(jlen) else np.zeros(0, dtype=np.uint64)
    out = np.empty(int(jlen.sum()), dtype=np.uint8)
    for i in range(len(jlen)):
        o, a, b = int(joff[i]), int(len1[i]), int(len2[i])
        out[o:o + a] = b1[int(off1[i]):int(off1[i]) + a]
        out[o + a] = 0x4E
        out[o + a + 1:o + a + 1 + b] = b2[int(off2[i]):int(off2[i]) + b]
    return out, joff, jlen.astype(np.uint32)


def lines_by_name(out, names):
    """{index of the read: its output line} (a read without a hit has no line; names may repeat, lines keep the input order)"""
    got, j = {}, 0
    for line in out.split(b"\n")[:-1]:
        while not line.startswith(names[j] + b"\t"):
            j += 1
        got[j] = line
        j += 1
    return got


def manifest():
    return json.load(open(os.path.join(util.GOLD, "pairs_manifest.json")))


def golden(name, rc):
    """the genuine reference's output on joined_fasta() (make_golden_pairs.py); the input it ran on must be the one built here"""
    return util.fixture_bytes("pairs_%s_out%s.txt.gz" % (name, "_rc" if rc else ""))


def sha256(b):
    return hashlib.sha256(b).hexdigest()


def gz(b):
    return gzip.compress(b, 1)
