"""Seeded inputs of the PACKSIZE=16 (k = 16, W = 4) runs: the generator of golden/k16_runs.json (golden/make_golden_k16.py) and the
tests (test_k16_cpu.py, test_gpu_k16.py) make them here, so the tests can check that they run on the very bytes the reference ran on."""
import hashlib

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
COMP[:] = ord("N")
for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[a] = b

# the committed BUILD input sets (golden/build_<set>.{fa,map}.gz)
BUILD_SETS = ["corner", "rel", "err_missing", "err_map_no_newline", "err_no_kmers", "err_missing_seq"]
RANDOM_SEEDS = [161, 162, 163, 164]
CHAIN_SEED = 1616


def sha256(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def random_refs(seed: int, n_refs: int = 160, lo: int = 10, hi: int = 1500, n_leaves: int = 24):
    """Colliding references under hostile GG labels: five root sequences with 1 % mutations; labels of 1-8 ranks, some with fewer than
    two ';' (no cut survives them), some that extend others by one rank, some whose ranks are prefixes of each other's; N's and
    lowercase sprinkled in, references shorter than k.  Returns (fasta bytes, map bytes), the map in another order than the FASTA."""
    rng = np.random.default_rng(seed)
    toks = ["k__0", "p__1", "p__12", "c__", "", "o__o", "o__oo", "f__x" * 3, "g__G1", "g__G10", "s__S"]
    leaves = []
    for _ in range(n_leaves):
        depth = int(rng.integers(1, 9))
        leaves.append(";".join(toks[int(rng.integers(0, len(toks)))] if d else "k__0" for d in range(depth)))
    for _ in range(n_leaves // 3):
        leaves.append(leaves[int(rng.integers(0, len(leaves)))] + ";" + toks[int(rng.integers(0, len(toks)))])
    roots = [rng.integers(0, 4, hi, dtype=np.uint8) for _ in range(5)]
    fa, mp = [], []
    for i in range(n_refs):
        L = int(rng.integers(lo, hi))
        a = int(rng.integers(0, hi - L + 1))
        s = roots[int(rng.integers(0, 5))][a:a + L].copy()
        mut = rng.random(L) < 0.01
        s[mut] = rng.integers(0, 4, int(mut.sum()), dtype=np.uint8)
        b = ACGT[s].copy()
        if rng.random() < 0.2:
            b[rng.integers(0, L, 3)] = ord("N")
        if rng.random() < 0.1:
            b = np.frombuffer(bytes(b).lower(), dtype=np.uint8)
        name = "ref %d x" % i
        fa.append(b">" + name.encode() + b"\n" + bytes(b) + b"\n")
        mp.append(name.encode() + b"\t" + leaves[int(rng.integers(0, len(leaves)))].encode() + b"\n")
    return b"".join(fa), b"".join(mp[i] for i in rng.permutation(n_refs))


def chain_refs(seed: int = CHAIN_SEED, n_refs: int = 300, lo: int = 20_000, hi: int = 100_000):
    """Related genomes: 12 ancestors of 100 kb; a reference is a stretch of one, mutated 0.3-3 % (closer relatives share more 16-mers),
    labelled with an 8-rank taxonomy under which ancestors and mutation rates nest.  Returns (fasta bytes, map bytes, [reference bytes])."""
    rng = np.random.default_rng(seed)
    anc = [rng.integers(0, 4, hi, dtype=np.uint8) for _ in range(12)]
    ranks = "kpcofgst"
    fa, mp, seqs = [], [], []
    for i in range(n_refs):
        g = int(rng.integers(0, len(anc)))
        L = int(rng.integers(lo, hi + 1))
        a = int(rng.integers(0, hi - L + 1))
        rate = float(rng.choice([0.003, 0.01, 0.03]))
        s = anc[g][a:a + L].copy()
        mut = rng.random(L) < rate
        s[mut] = rng.integers(0, 4, int(mut.sum()), dtype=np.uint8)
        b = ACGT[s].tobytes()
        path = [g // 6, g // 3, g, int(rate * 1000), int(rng.integers(0, 3)), int(rng.integers(0, 3)), i % 7, i]
        depth = int(rng.integers(5, 9))
        lab = ";".join("%s__%s%d" % (ranks[d], ranks[d].upper(), path[d]) for d in range(depth))
        fa.append(b">g%d\n" % i + b + b"\n")
        mp.append(b"g%d\t" % i + lab.encode() + b"\n")
        seqs.append(b)
    return b"".join(fa), b"".join(mp), seqs


def chain_reads(seqs, seed: int = CHAIN_SEED + 1, n: int = 100_000, length: int = 150):
    """n reads of `length` bases drawn from the references, 1 % substitutions, half of them reverse complemented, one in 50 with an N."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, len(seqs), n)
    out = []
    for i in range(n):
        s = seqs[int(src[i])]
        a = int(rng.integers(0, len(s) - length + 1))
        r = np.frombuffer(s[a:a + length], dtype=np.uint8).copy()
        mut = rng.random(length) < 0.01
        r[mut] = ACGT[rng.integers(0, 4, int(mut.sum()))]
        if i % 2:
            r = COMP[r[::-1]]
        if i % 50 == 7:
            r[int(rng.integers(0, length))] = ord("N")
        out.append(b">q%d\n" % i + r.tobytes() + b"\n")
    return b"".join(out)


def rank_reads(words: np.ndarray, seed: int, n: int = 1500) -> bytes:
    """Reads of 1 bp .. 40 kb built from a k = 16 database's words (so they hit), random filler, N's, lowercase stretches and CRLF line
    ends.  `words`: uint64 array of 32-bit words."""
    rng = np.random.default_rng(seed)
    pick = words[rng.integers(0, len(words), 6000)]
    kmers = [ACGT[[(int(w) >> (30 - 2 * j)) & 3 for j in range(16)]].tobytes() for w in pick]
    recs = []
    for i in range(n):
        L = int(rng.choice([int(rng.integers(1, 40)), int(rng.integers(40, 400)), int(rng.integers(400, 4000))], p=[0.2, 0.7, 0.1]))
        if i in (100, 900):
            L = 40_000 if i == 100 else 17_000
        parts, m = [], 0
        while m < L:
            s = kmers[int(rng.integers(0, len(kmers)))] if rng.random() < 0.6 else ACGT[rng.integers(0, 4, int(rng.integers(1, 24)))].tobytes()
            if rng.random() < 0.04:
                s += b"N"
            if rng.random() < 0.05:
                s = s.lower()
            parts.append(s)
            m += len(s)
        eol = b"\r\n" if i % 9 == 4 else b"\n"
        recs.append(b">r%d some text" % i + eol + b"".join(parts)[:L] + eol)
    return b"".join(recs)


def db_words(d) -> np.ndarray:
    """The 32-bit words of a k = 16 database loaded with ctrfile (CtrData)."""
    hi, lo = d.words()
    return lo.astype(np.uint64)
