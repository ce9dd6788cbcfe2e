"""Inputs for the bucket-addressing tests (test_geometry_cpu.py, test_gpu_geometry.py): region tables shaped like production ones on
databases of a few hundred thousand nodes, and k-mers planted on the edges of their slots.

A k-mer's bucket is found through the image's 256-entry region table (csrc/utree_internal.h: utree_image_header.regions): region r = the
top 8 bits of the minimizer hash has nb_r slots, slot = (h24 * nb_r) >> 24, a slot is sub_r pairs of buckets.  csrc/dev_image.c sizes a
region from the node count, so every database of suite size gets nb_r = 2^16 everywhere -- a power of two, sub = 1.  UTREE_BUCKET_TARGET
takes a fraction: with a few thousandths of a node per bucket a small database gets the table of a thousand times larger one.

Plain Python and numpy; nothing here runs on the GPU.  The truth of every test is the CPU oracle: the minimizer below only CHOOSES inputs.
"""
import math
import struct

import numpy as np

from utree_amd import ctrfile

M32 = 0xFFFFFFFF
NB_BITS, SUB_BITS = 25, 9                     # utree_internal.h: regions[r] = base << 34 | sub << 25 | nb
IMG_MAGIC = 0x31474d4945525455                # "UTREIMG1"
MIN_LOW_BITS = 9                              # device_common.hpp: 16-mers are ranked by their hash without its low 9 bits


# ---- the size model: dev_image.c, compute_regions_sub and what it calls, line by line ------------------------------------------------
def pois_tail_nodes(lam, cap):
    if lam <= 0:
        return 0.0
    p, s = math.exp(-lam), 0.0
    for k in range(1, cap + 1):
        p *= lam / k
        s += k * p
    s = 1.0 - s / lam
    return 0.0 if s < 0 else s


def lumpy_overflow(nb, expect, cap):
    v, lam1 = 16777216.0 / nb, expect / 16777216.0
    if v > 48.0:
        return pois_tail_nodes(expect / (2.0 * nb), cap)
    lo = int(math.floor(v))
    fr = v - lo
    tot = totw = 0.0
    for which in range(2):
        V = lo + which
        w = fr if which else 1.0 - fr
        if not V or w <= 0:
            continue
        pn = math.pow(0.5, V)
        for n in range(0, min(V, 64) + 1):
            mean = n * lam1
            tot += w * pn * mean * pois_tail_nodes(mean, cap)
            totw += w * pn * mean
            pn = pn * float(V - n) / float(n + 1)
    return tot / totw if totw > 0 else 0.0


def rec_words(W, I):
    return (2 if W == 16 else 1) * (2 if I == 4 else 1)


def regions_model(n_nodes, W, I, bucket_words, F, target, slack=1.5, sub=None):
    """compute_regions_sub: ([(nb, sub)] * 256, n_slots).  target: UTREE_BUCKET_TARGET (None: the default load); sub: UTREE_TEST_SUB, with
    the sub-slices on (k = 64, F >= 8) -- whether the library keeps them under UTREE_TABLE_MAX_GB is compute_regions' business."""
    margin = 2 if W == 16 else 0
    m = 4.0 * W - 15.0 - 2.0 * margin
    cap_entries = bucket_words // rec_words(W, I)
    if target is None or target <= 0:
        target = (0.5625 if bucket_words == 16 else 0.375) * cap_entries
    sub_on = W == 16 and F >= 8
    p0 = pois_tail_nodes(target, cap_entries)
    nb_max, nb_min = 1 << (16 + min(F, 8)), 1 << 16
    out, base = [], 0
    for r in range(256):
        expect = float(n_nodes) * (math.pow(1.0 - r / 256.0, m) - math.pow(1.0 - (r + 1) / 256.0, m))
        want = math.ceil(expect / (2.0 * target))
        nb, s = (nb_max if want >= float(nb_max) else int(want)), 1
        nb = min(max(nb, nb_min), nb_max)
        if slack > 0:
            while nb < nb_max and lumpy_overflow(float(nb), expect, cap_entries) > slack * p0 + 1e-4:
                nb = min(nb + nb // 20 + 1, nb_max)
        if sub_on and nb == 1 << 24:
            per_value = expect / 16777216.0
            while s < 256 and pois_tail_nodes(per_value * math.ceil(256.0 / s) / 256.0, cap_entries) > slack * p0 + 1e-4:
                s += 1
        if sub_on and sub is not None and 1 <= sub <= 256:
            s = sub
        out.append((nb, s))
        base += nb * s
    return out, 2 * base


def pick_fine_bits(n_nodes, W, I, bucket_words, target, cap_gb):
    """utree_pick_fine_bits on automatic: the finest table within the cap"""
    F = 8
    while F > 0 and regions_model(n_nodes, W, I, bucket_words, F, target)[1] * 8.0 * bucket_words > cap_gb * 1073741824.0:
        F -= 1
    return F


def align_up(x, a):
    return (x + a - 1) // a * a


def layout_bytes(n_nodes, W, I, bucket_words, n_slots, label_lens):
    """dev_image.c: layout() -- the bytes an image is built in (u32 bin offsets, buckets: not PACKSIZE=16)"""
    rw = rec_words(W, I)
    off = 4096
    off = align_up(off + n_slots * 8 * bucket_words, 4096)
    off = align_up(off + (n_nodes + n_nodes // 8 + 65536 + 8) * rw * 8, 4096)      # MIN records + room for second views
    off = align_up(off + ((1 << 24) + 1) * 4, 256)
    off = align_up(off + (1 << 24) // 8, 256)
    off = align_up(off + (len(label_lens) + 1) * 4, 256)
    off = align_up(off + sum(l + 1 for l in label_lens) + 64, 256)
    off = align_up(off + len(label_lens) * 4, 256)
    off = align_up(off + len(label_lens) * 32, 4096)                                 # utk_vote_rec
    off = align_up(off + (n_nodes + 8) * rw * 8, 4096)
    return off


# ---- the tables: id -> how the image is asked for, and the figures the table must show ------------------------------------------------
class Table:
    def __init__(self, k, I, bucket_bytes, fine_bits, target, n_nodes=300_000, max_gb=None, test_sub=None, gib=None, nb0=None, capped=None):
        self.k, self.W, self.I, self.bucket_bytes, self.fine_bits, self.target, self.n_nodes = k, k // 4, I, bucket_bytes, fine_bits, target, n_nodes
        self.max_gb, self.test_sub, self.gib, self.nb0, self.capped = max_gb, test_sub, gib, nb0, capped

    def env(self):
        """the variables the image is built under (everything else that sizes a table must be unset: CLEAR)"""
        e = {"UTREE_BUCKET_TARGET": repr(self.target), "UTREE_BUCKET_BYTES": str(self.bucket_bytes)}
        if self.fine_bits is not None:
            e["UTREE_FINE_BITS"] = str(self.fine_bits)
        if self.max_gb is not None:
            e["UTREE_TABLE_MAX_GB"] = str(self.max_gb)
        if self.test_sub is not None:
            e["UTREE_TEST_SUB"] = str(self.test_sub)
        return e

    def model(self, n_nodes=None):
        """(regions, n_slots, fine_bits) for a database of n_nodes nodes (default: the nominal count)"""
        n = self.n_nodes if n_nodes is None else n_nodes
        bw = self.bucket_bytes // 8
        F = self.fine_bits if self.fine_bits is not None else pick_fine_bits(n, self.W, self.I, bw, self.target, self.max_gb or 96.0)
        reg, ns = regions_model(n, self.W, self.I, bw, F, self.target, sub=self.test_sub)
        return reg, ns, F


CLEAR = ("UTREE_BUCKET_TARGET", "UTREE_BUCKET_BYTES", "UTREE_FINE_BITS", "UTREE_TABLE_MAX_GB", "UTREE_TEST_SUB", "UTREE_LUMP_SLACK", "UTREE_SUB_SLICES",
         "UTREE_BUCKET128_NODES")

# gib: the table's size; nb0: slots of region 0; capped: regions at 2^(16 + fine_bits), where the table is meant to have some
TABLES = {
    "A": Table(32, 2, 64, 8, 0.003, gib=7.4, nb0=3_218_552),
    "A5": Table(32, 2, 64, 5, 0.003, gib=6.9, capped=7),
    "A3": Table(32, 2, 64, 3, 0.003, gib=4.1, capped=28),
    "A1": Table(32, 2, 64, 1, 0.003, gib=2.4, capped=47),
    "Aauto": Table(32, 2, 64, None, 0.003, max_gb=5),
    "A128": Table(32, 2, 128, 8, 0.003, gib=14.9, nb0=3_218_552),
    "Ai4": Table(32, 4, 64, 8, 0.003, gib=7.4, nb0=3_218_552),
    "B": Table(64, 2, 64, 8, 0.003, gib=7.7, nb0=8_074_362),
    "Bi4": Table(64, 4, 64, 8, 0.003, gib=7.7, nb0=8_074_362),
    "C64": Table(64, 2, 64, 8, 0.00047, n_nodes=100_000, gib=14.4, nb0=1 << 24, capped=1),
    "C64sub": Table(64, 2, 64, 8, 0.00047, n_nodes=100_000, test_sub=3, gib=43.0, nb0=1 << 24, capped=1),
    "C32": Table(32, 2, 64, 8, 0.00055, gib=33.7, nb0=1 << 24, capped=1),
}


def figures(regions, fine_bits):
    """what the issue asks of a table: regions whose nb is no power of two, regions at the cap, regions at the floor"""
    nbs = [nb for nb, _ in regions]
    return dict(odd=sum(1 for nb in nbs if nb & (nb - 1)), capped=sum(1 for nb in nbs if nb == 1 << (16 + fine_bits) and fine_bits > 0),
                floor=sum(1 for nb in nbs if nb == 1 << 16))


def check_figures(t, regions, n_slots, fine_bits):
    """the figures every test asserts before it trusts a table (CPU: on the model; GPU: on the image's own header)"""
    f = figures(regions, fine_bits)
    # (A1 caps 47 of the 56 regions it has above the floor at 2^17, a power of two: the other 9 are all that can be odd)
    assert f["odd"] >= (9 if fine_bits == 1 else 20) and f["floor"] >= 150, f
    if t.capped is not None:
        assert f["capped"] >= 1, f
        if t.capped > 1:
            assert f["capped"] == t.capped, f
    if t.nb0 is not None:
        assert abs(regions[0][0] - t.nb0) <= t.nb0 // 50, (regions[0], t.nb0)        # (nb follows the node count, which is the nominal one +- 1 %)
        if t.nb0 == 1 << 24:
            assert regions[0][0] == 1 << 24
    if t.test_sub is not None:
        assert regions[0] == (1 << 24, t.test_sub)
    if t.gib is not None:
        assert abs(n_slots * t.bucket_bytes / 2.0**30 - t.gib) < 0.06 * t.gib, n_slots * t.bucket_bytes / 2.0**30
    if t.max_gb is not None:
        assert n_slots * t.bucket_bytes <= t.max_gb * 2**30 and fine_bits < 8


def read_regions(tree):
    """The image's own header (utree_internal.h: utree_image_header, decoded by its field layout) from the first 4096 bytes of
    tree.image_tensor(): dict(n_slots, fine_bits, bucket_words, regions = [(base, sub, nb)] * 256)."""
    raw = tree.image_tensor()[:4096].cpu().numpy().tobytes()
    magic, version, W, I, k, fine_bits, rw, n_labels, flags, n_nodes, n_slots, n_min = struct.unpack_from("<Q8IQQQ", raw, 0)
    offs = struct.unpack_from("<8Q", raw, 64)                     # off_table, off_mrecs, off_recs, off_coarse, off_irreg, off_label_off, off_label_blob, off_rank2ix
    label_blob_bytes, n_irregular, total_bytes, off_vote, bucket_words, pad0 = struct.unpack_from("<4Q2I", raw, 128)
    ent = struct.unpack_from("<256Q", raw, 168)
    assert magic == IMG_MAGIC, hex(magic)
    assert total_bytes == tree.info.image_bytes, (total_bytes, tree.info.image_bytes)
    assert W * 4 == k and rw == rec_words(W, I) and offs[0] == 4096
    regions = [(e >> (NB_BITS + SUB_BITS), (e >> NB_BITS) & ((1 << SUB_BITS) - 1), e & ((1 << NB_BITS) - 1)) for e in ent]
    base = 0
    for b, s, nb in regions:                                      # the bases are the running sum of nb * sub
        assert b == base, (b, base)
        base += nb * s
    assert 2 * base == n_slots
    return dict(n_slots=n_slots, fine_bits=fine_bits, bucket_words=bucket_words, regions=regions, n_nodes=n_nodes, W=W, I=I)


# ---- the minimizer hash and its inverse -----------------------------------------------------------------------------------------------
MUL1, MUL2 = 0x9E3779B1, 0x85EBCA6B
INV1, INV2 = pow(MUL1, -1, 1 << 32), pow(MUL2, -1, 1 << 32)


def mix32(x):
    x = (x * MUL1) & M32
    x ^= x >> 15
    return (x * MUL2) & M32


def unmix32(h):
    x = (h * INV2) & M32
    x ^= x >> 15
    x ^= x >> 30
    return (x * INV1) & M32


def rc16(m):
    r = 0
    for j in range(16):
        r = (r << 2) | (3 - ((m >> (2 * j)) & 3))
    return r


def mer_str(m):
    return "".join("ACGT"[(m >> (30 - 2 * j)) & 3] for j in range(16))


def mer_int(s):
    v = 0
    for c in s:
        v = (v << 2) | "ACGT".index(c)
    return v


COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def minimizer(kmer, k):
    """(position, hash of the canonical 16-mer) of the k-mer's minimizer: the leftmost 16-mer of the smallest mix32(canonical) >> 9;
    k = 64 counts positions 2 .. 46 only (UTREE_MIN_MARGIN)."""
    j0 = 2 if k == 64 else 0
    v = mer_int(kmer[j0:j0 + 16])
    best = None
    for j in range(j0, k - 16 - j0 + 1):
        if j > j0:
            v = ((v << 2) & M32) | "ACGT".index(kmer[j + 15])
        h = mix32(min(v, rc16(v)))
        if best is None or (h >> MIN_LOW_BITS) < (best[1] >> MIN_LOW_BITS):
            best = (j, h)
    return best


# ... and the same on arrays: k-mers as rows of base codes (uint8, A C G T = 0 1 2 3)
def _rc16_np(m):
    m = ((m >> np.uint32(2)) & np.uint32(0x33333333)) | ((m & np.uint32(0x33333333)) << np.uint32(2))
    m = ((m >> np.uint32(4)) & np.uint32(0x0F0F0F0F)) | ((m & np.uint32(0x0F0F0F0F)) << np.uint32(4))
    return ~m.byteswap()


def _mix32_np(x):
    x = x * np.uint32(MUL1)
    x ^= x >> np.uint32(15)
    return x * np.uint32(MUL2)


def minimizers(codes, k):
    """minimizer() of every row: (positions, hashes)"""
    j0 = 2 if k == 64 else 0
    n = len(codes)
    c = codes.astype(np.uint32)
    v = np.zeros(n, np.uint32)
    for i in range(16):
        v = (v << np.uint32(2)) | c[:, j0 + i]
    pos, best = np.full(n, j0, np.int64), None
    for j in range(j0, k - 16 - j0 + 1):
        if j > j0:
            v = (v << np.uint32(2)) | c[:, j + 15]
        h = _mix32_np(np.minimum(v, _rc16_np(v)))
        if best is None:
            best = h
        else:
            less = (h >> np.uint32(MIN_LOW_BITS)) < (best >> np.uint32(MIN_LOW_BITS))
            best = np.where(less, h, best)
            pos = np.where(less, j, pos)
    return pos, best


def codes_of(seqs, k):
    a = np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), k)
    lut = np.zeros(256, np.uint8)
    lut[[ord(c) for c in "ACGT"]] = [0, 1, 2, 3]
    return lut[a]


def strs_of(codes):
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [r.tobytes().decode() for r in a]


def pack(codes):
    """rows of base codes -> (hi, lo) as ctrfile.encode_kmers packs them: the first base in the top bits"""
    n, k = codes.shape
    lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for i in range(k):
        if k == 64 and i < 32:
            hi = (hi << np.uint64(2)) | codes[:, i].astype(np.uint64)
        else:
            lo = (lo << np.uint64(2)) | codes[:, i].astype(np.uint64)
    return hi, lo


def unpack(hi, lo, k):
    n = len(lo)
    codes = np.zeros((n, k), np.uint8)
    for i in range(k):
        src, sh = (hi, 2 * (31 - i)) if (k == 64 and i < 32) else (lo, 2 * (k - 1 - i))
        codes[:, i] = ((src >> np.uint64(sh)) & np.uint64(3)).astype(np.uint8)
    return codes


def canonical(h):
    """is hash value h some canonical 16-mer's (its preimage no larger than the preimage's reverse complement)?"""
    c = unmix32(h)
    return c <= rc16(c)


def slot_of(h, nb):
    return ((h & 0xFFFFFF) * nb) >> 24


def first_of_slot(s, nb):
    """the smallest 24-bit hash value of slot s: ceil(s * 2^24 / nb)"""
    return -((-s << 24) // nb)


# ---- the database --------------------------------------------------------------------------------------------------------------------
LABELS = (["k__A;p__P%d;c__C%d;o__O%d" % (a, b, c) for a in range(3) for b in range(3) for c in range(4)] +
          ["k__A;p__P%d;c__C%d" % (a, b) for a in range(3) for b in range(3)] + ["k__A;p__P%d" % a for a in range(3)])   # test_gpu_lanes.py: OwnDB
MARGIN_POS = (0, 1, 47, 48)                   # k = 64: positions the margin excludes -- a 16-mer there is never the minimizer


def planted_regions(regions):
    """{0, 1, a mid region whose nb is no power of two, the last region above the floor, the first region at the floor}"""
    nbs = [e[0] for e in regions]
    above = [r for r in range(256) if nbs[r] > 1 << 16]
    odd = [r for r in above if nbs[r] & (nbs[r] - 1)]
    pick = [0, 1, odd[len(odd) // 2], above[-1], above[-1] + 1]
    assert nbs[pick[4]] == 1 << 16
    return sorted(set(pick))


def planted_hashes(r, nb):
    """[(edge kind, h)]: the hash values of region r the planted k-mers sit on -- the region's ends, the first value of eight slots spread over
    the region and the last value of the slots before them, and each of those plus 256 (the same low 8 bits: the record key cannot tell it from
    h, the bucket must); a value that is no canonical 16-mer's hash moves to the nearest one on the same side of its edge that is"""
    out = []
    top = (1 << 24) - 1

    def keep(kind, v, step):
        while 0 <= v <= top and not canonical(r << 24 | v):
            v += step
        if 0 <= v <= top:
            out.append((kind, r << 24 | v))
    for kind, v, step in (("region_first", 0, 1), ("region_second", 1, 1), ("region_last_but_one", top - 1, -1), ("region_last", top, -1)):
        keep(kind, v, step)
    slots = sorted({1, nb // 7, nb // 3, nb // 2 + 1, (2 * nb) // 3, nb - nb // 5, nb - 2, nb - 1})
    assert len(slots) == 8
    for n, s in enumerate(slots):
        v = first_of_slot(s, nb)
        assert slot_of(v, nb) == s and slot_of(v - 1, nb) == s - 1
        keep("slot%d_first" % n, v, 1)
        keep("slot%d_last" % n, v - 1, -1)
        keep("slot%d_first+256" % n, v + 256, 1)
        keep("slot%d_last+256" % n, v - 1 + 256, -1)
    return out


def plant_all(rng, k, mer, positions):
    """{pos: (k-mer as a row of codes, live)} -- the 16-mer `mer` (an integer) at every one of `positions` between random flanks, redrawn until
    minimizers() picks that 16-mer there (live = False: no draw did, or the position is one the margin excludes)"""
    mc = np.array([(mer >> (30 - 2 * j)) & 3 for j in range(16)], np.uint8)
    h = np.uint32(mix32(min(mer, rc16(mer))))
    out, todo, n = {}, list(positions), 8
    for _ in range(8):
        c = rng.integers(0, 4, (len(todo), n, k), dtype=np.uint8)
        for i, pos in enumerate(todo):
            c[i, :, pos:pos + 16] = mc
        p, hh = minimizers(c.reshape(-1, k), k)
        p, hh = p.reshape(len(todo), n), hh.reshape(len(todo), n)
        left = []
        for i, pos in enumerate(todo):
            ok = np.flatnonzero((p[i] == pos) & (hh[i] == h))
            if len(ok):
                out[pos] = (c[i, ok[0]], True)
            else:
                out[pos] = (c[i, 0], False)
                if not (k == 64 and pos in MARGIN_POS):
                    left.append(pos)
        todo, n = left, min(8 * n, 8192)
        if not todo:
            break
    return out


def plant(rng, k, mer, pos, check):
    return plant_all(rng, k, mer, [pos])[pos]


def related_seqs(rng, roots, length, relatives):
    """the sequences of test_gpu_lanes.related_db (which also writes a database of them: not wanted here), as rows of base codes: `relatives`
    mutated copies -- 3 % substitutions, every fifth 10 % -- of each of `roots` random roots"""
    seqs = []
    for r in range(roots):
        root = rng.integers(0, 4, length)
        for c in range(relatives):
            s = root.copy()
            mut = rng.random(length) < (0.10 if c % 5 == 4 else 0.03)
            s[mut] = rng.integers(0, 4, int(mut.sum()))
            seqs.append(s.astype(np.uint8))
    return seqs


def boundary_db(regions, k, I, seed, path, n_nodes):
    """Writes the .ctr -- bulk + crowded + planted k-mers + one heavy value on a slot edge at the median of the hashes, n_nodes nodes (+- a few
    duplicates) -- and returns a dict: ctr, k, hi / lo / ix (the nodes in file order), planted = {(region, edge kind, orientation, position):
    [k-mers]}, live = the planted classes with a k-mer whose planted 16-mer IS its minimizer, siblings = [(k-mer, its h + 1 sibling or None, its
    h + 256 sibling or None)] (in the database, under other labels), absent = the k-mers with the neighbours' 16-mers that are NOT in the
    database, seqs = the crowded part's sequences, heavy = what test_geometry_cpu.py checks of the heavy value."""
    rng = np.random.default_rng(seed)
    n_lab = len(LABELS)
    rows, labs, seen = [], [], set()                               # the special k-mers

    def add(c, lab):
        key = c.tobytes()
        if key in seen:
            return False
        seen.add(key); rows.append(c); labs.append(lab)
        return True
    planted, live, siblings, absent = {}, set(), [], []
    j0 = 2 if k == 64 else 0
    inner = (5, 11) if k == 32 else (17, 30)
    positions = [j0, k - 16 - j0] + list(inner) + (list(MARGIN_POS) if k == 64 else [])
    for r in planted_regions(regions):
        for kind, h in planted_hashes(r, regions[r][0]):
            cm = unmix32(h)
            assert cm <= rc16(cm) and mix32(cm) == h
            nbr = []
            for d in (1, 256):                                     # the neighbours: the next canonical value above h, and above h in steps of 256
                h2 = h + d
                while h2 >> 24 == r and not canonical(h2):
                    h2 += d
                nbr.append(unmix32(h2) if h2 >> 24 == r else None)
            for o, mer in ((0, cm), (1, rc16(cm))):
                for pos, (c, ok) in plant_all(rng, k, mer, positions).items():
                    lab = int(rng.integers(0, n_lab))
                    if not add(c, lab):
                        continue
                    planted.setdefault((r, kind, o, pos), []).append(c)
                    if ok:
                        live.add((r, kind, o, pos))
                    sib = [c]
                    for n, c2 in enumerate(nbr):                   # the same flanks around the neighbour 16-mer
                        if c2 is None:
                            sib.append(None)
                            continue
                        m2 = c2 if o == 0 else rc16(c2)
                        s2 = c.copy()
                        s2[pos:pos + 16] = [(m2 >> (30 - 2 * j)) & 3 for j in range(16)]
                        if pos in inner:                           # inner positions: the neighbours stay out of the database -- lookups that must miss
                            absent.append(s2)
                            sib.append(None)
                        else:                                      # end positions: in the database under another label
                            sib.append(s2 if add(s2, (lab + 1 + n) % n_lab) else None)
                    if sib[1] is not None or sib[2] is not None:
                        siblings.append(tuple(sib))
    # crowded: every k-mer of mutated relatives -- buckets with many entries and overflow runs behind the addressing under test
    # (30 relatives of two roots are some 100 000 k-mers: where that is more than a third of the nodes the table is sized for, 8 relatives)
    seqs = related_seqs(rng, roots=2, length=2000, relatives=30 if n_nodes >= 300_000 else 8)
    for ci, s in enumerate(seqs):
        w = np.lib.stride_tricks.sliding_window_view(s, k)
        for c in w:
            add(c, ci % n_lab)
    seqs = strs_of(np.array(seqs, np.uint8))
    # bulk: random k-mers up to the wanted node count (the table depends on it), less the heavy value's
    n_heavy = n_nodes // 25
    n_bulk = n_nodes - len(rows) - n_heavy
    assert n_bulk > n_nodes // 2, (len(rows), n_nodes)
    codes = np.concatenate([np.array(rows, np.uint8), rng.integers(0, 4, (n_bulk, k), dtype=np.uint8)])
    ix = np.concatenate([np.array(labs, np.uint32), rng.integers(0, n_lab, n_bulk).astype(np.uint32)])
    # heavy: one hash value with n_nodes / 25 k-mers, at the median of the nodes' hashes -- where a build in 2 (or 64) parts cuts --, the FIRST value
    # of its slot, with nodes on the value below it (the last of the slot before) and on a smaller value of that slot: a cut that is not rounded
    # up to the slot's first value parts those two
    _, hs = minimizers(codes, k)
    hm = int(np.sort(hs)[len(hs) // 2])
    r, nb = hm >> 24, regions[hm >> 24][0]
    heavy = None
    for s in range(slot_of(hm, nb) + 1, nb):
        v = first_of_slot(s, nb)
        lows = [w for w in range(first_of_slot(s - 1, nb), v - 1) if canonical(r << 24 | w)]
        if canonical(r << 24 | v) and canonical(r << 24 | (v - 1)) and lows:
            heavy = dict(region=r, nb=nb, slot=s, h=r << 24 | v, last=r << 24 | (v - 1), low=r << 24 | lows[0], median_before=hm)
            break
    assert heavy is not None
    hrows, hlabs = [], []
    for name, per in (("last", 6), ("low", 6)):
        cm = unmix32(heavy[name])
        got = []
        for o, mer in ((0, cm), (1, rc16(cm))):
            for _ in range(per):
                c, ok = plant(rng, k, mer, int(rng.integers(j0, k - 16 - j0 + 1)), True)
                if ok:
                    got.append(c); hrows.append(c); hlabs.append(int(rng.integers(0, n_lab)))
        heavy[name + "_kmers"] = got
    cm = unmix32(heavy["h"])
    mcs = [np.array([(m >> (30 - 2 * j)) & 3 for j in range(16)], np.uint8) for m in (cm, rc16(cm))]
    while len(hrows) < n_heavy:
        c = rng.integers(0, 4, (4096, k), dtype=np.uint8)
        p = rng.integers(j0, k - 16 - j0 + 1, 4096)
        o = rng.integers(0, 2, 4096)
        for j in range(16):
            c[np.arange(4096), p + j] = np.where(o == 1, mcs[1][j], mcs[0][j])
        pp, hh = minimizers(c, k)
        good = c[(pp == p) & (hh == np.uint32(heavy["h"]))][: n_heavy - len(hrows)]
        hrows += list(good)
        hlabs += [int(x) for x in rng.integers(0, n_lab, len(good))]
    heavy["n"] = len(hrows)
    codes = np.concatenate([codes, np.array(hrows, np.uint8)])
    ix = np.concatenate([ix, np.array(hlabs, np.uint32)])
    hi, lo = pack(codes)
    order = np.lexsort((lo, hi))
    hi, lo, ix = hi[order], lo[order], ix[order]
    keep = np.ones(len(lo), bool)
    keep[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    hi, lo, ix = hi[keep], lo[keep], ix[keep]
    ctrfile.write_ctr(path, k // 4, I, hi, lo, ix, LABELS)
    as_str = lambda d: {key: strs_of(np.array(v, np.uint8)) for key, v in d.items()}
    sib = [tuple(None if c is None else strs_of(c[None, :])[0] for c in t) for t in siblings]
    for name in ("last_kmers", "low_kmers"):
        heavy[name] = strs_of(np.array(heavy[name], np.uint8))
    return dict(ctr=path, k=k, I=I, hi=hi, lo=lo, ix=ix, labels=LABELS, planted=as_str(planted), live=live, siblings=sib,
                absent=strs_of(np.array(absent, np.uint8)), seqs=seqs, heavy=heavy)


class Words:
    """what test_gpu_parity.random_reads wants of a database"""

    def __init__(self, db):
        self.k, self._hi, self._lo = db["k"], db["hi"], db["lo"]

    def words(self):
        return self._hi, self._lo


def rand_seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def geometry_reads(db, rng):
    """[(name, sequence)]: random reads of every length class (1 to 160 bases, 161 to 2095, a few of 3 to 9 kb), every planted k-mer, sibling and
    absent neighbour between random flanks of 0 to 40 bases, half of them reverse-complemented, reads that join two siblings, reads cut from
    the crowded relatives and reads over the heavy value and its neighbours"""
    from test_gpu_parity import random_reads
    d = Words(db)
    reads = random_reads(rng, d, 1500, 1, 160, hit_frac=0.8) + random_reads(rng, d, 120, 161, 2095, hit_frac=0.8) + random_reads(rng, d, 4, 3000, 9000, hit_frac=0.8)
    every = [s for v in db["planted"].values() for s in v] + [s for t in db["siblings"] for s in t[1:] if s] + db["absent"]
    every += db["heavy"]["last_kmers"] + db["heavy"]["low_kmers"]
    n = 0
    for s in every:
        t = rand_seq(rng, int(rng.integers(0, 41))) + s + rand_seq(rng, int(rng.integers(0, 41)))
        reads.append(("p%d" % n, t if n % 2 else revcomp(t)))
        n += 1
    for t in db["siblings"]:
        a = [s for s in t if s]
        for x, y in zip(a, a[1:]):
            j = x + rand_seq(rng, int(rng.integers(0, 9))) + y
            reads.append(("j%d" % n, j if n % 2 else revcomp(j)))
            n += 1
    seqs = db["seqs"]
    for i in range(300):
        s = seqs[int(rng.integers(0, len(seqs)))]
        p = int(rng.integers(0, len(s) - 150))
        reads.append(("c%d" % i, s[p:p + 150] if i % 3 else revcomp(s[p:p + 150])))
    return [reads[i] for i in rng.permutation(len(reads))]


def fasta_bytes(reads):
    return b"".join(b">" + n.encode() + b"\n" + s.encode() + b"\n" for n, s in reads)


def neighbour_queries(db, rng):
    """(hi, lo) of the words a lookup test asks for beyond the database's own: the absent neighbours of the planted k-mers (misses by
    construction), the planted k-mers and siblings again, and 5 000 random words"""
    k = db["k"]
    seqs = db["absent"] + [s for t in db["siblings"] for s in t if s]
    hi, lo = pack(codes_of(seqs, k))
    rlo = rng.integers(0, 1 << 63, 5000).astype(np.uint64)
    rhi = rng.integers(0, 1 << 63, 5000).astype(np.uint64) if k == 64 else np.zeros(5000, np.uint64)
    return np.concatenate([hi, rhi]), np.concatenate([lo, rlo]), len(db["absent"])


def oracle_lookup(o, hi, lo):
    """OracleDB.lookup word by word: the label index, all ones for a miss"""
    nl = o.n_labels
    out = np.empty(len(lo), np.uint32)
    for j, (h, l) in enumerate(zip(hi.tolist(), lo.tolist())):
        w = o.lookup(h, l)
        out[j] = w if w < nl else 0xFFFFFFFF
    return out
