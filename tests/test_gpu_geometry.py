"""Bucket addressing on region tables shaped like production ones.

A k-mer's bucket is found through the image's 256-entry region table: region r has nb_r slots, slot = (h24 * nb_r) >> 24, a slot is sub_r
pairs of buckets (csrc/utree_internal.h).  The arithmetic is written out four times -- pair_of / bucket_of (device_common.hpp: the image
build, and lookup_word: get_ix, the hit map, the rank-specific search), locate (kernels.hip: the wave-per-read kernels), bucket_index
(lanes_core.hpp: the lane pass, in 32 bits) and the part cuts of a build in parts (image_build.hip) --, and every database of suite size gets
nb_r = 2^16 in all 256 regions: a power of two, sub = 1, the cap never reached.  Here UTREE_BUCKET_TARGET takes a few thousandths of a node
per bucket, so that databases of 100 000 to 300 000 nodes get the tables of a thousand times larger ones (geometry_inputs.TABLES): slot
counts that are no power of two, regions at the cap of every fine_bits, one hash value per slot, several pairs per slot.  The databases
hold k-mers planted on the first and last hash values of slots and regions (geometry_inputs.boundary_db; test_geometry_cpu.py shows they
sit where they are meant to), and everything is compared with the CPU oracle byte for byte.

Run on the MI355X box:  python -m pytest tests/test_gpu_geometry.py -m gpu -q
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import ctrfile, lib
from utree_amd.search import CtrDB, DeviceTree, classify_fasta_bytes, search_rank
import geometry_inputs as g
import hitmap_ref
from test_gpu_hitmap import assert_map, device_reads


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


class Case:
    """One table's database, reads and the oracle's answers: made once, shared by every test on that table, never changed."""

    def __init__(self, name, tmp):
        self.name, self.t = name, g.TABLES[name]
        t = self.t
        self.regions, _, _ = t.model()
        self.db = g.boundary_db(self.regions, t.k, t.I, 7, os.path.join(tmp, name + ".ctr"), t.n_nodes)
        self.n = len(self.db["lo"])
        self.ctr = CtrDB.open(self.db["ctr"])
        self.o = orc.OracleDB.load(self.db["ctr"])
        reads = g.geometry_reads(self.db, np.random.default_rng(5))
        self.reads = {"short": [r for r in reads if len(r[1]) <= 160], "mixed": [r for r in reads if len(r[1]) > 160]}
        assert len(self.reads["short"]) > 3000 and len(self.reads["mixed"]) >= 100 and max(len(s) for _, s in self.reads["mixed"]) >= 3000
        self.fasta = {w: g.fasta_bytes(r) for w, r in self.reads.items()}
        self.tmp = tmp
        self._want, self._ix = {}, None

    def path(self, which):
        p = os.path.join(self.tmp, "%s_%s.fa" % (self.name, which))
        if not os.path.exists(p):
            open(p, "wb").write(self.fasta[which])
        return p

    def want(self, which, rc):
        """the oracle's output file for the reads, computed once"""
        if (which, rc) not in self._want:
            out = os.path.join(self.tmp, "%s_%s_%d.txt" % (self.name, which, rc))
            code, nr, good, err = self.o.search_file(self.path(which), out, threads=8, rc=rc)
            assert code == 0 and nr == len(self.reads[which])
            self._want[(which, rc)] = open(out, "rb").read()
            assert self._want[(which, rc)].count(b"\n") > len(self.reads[which]) // 3       # the reads do hit
        return self._want[(which, rc)]

    def queries(self):
        """(hi, lo, the oracle's answer) for every database word, the planted k-mers' absent neighbours, siblings and 5 000 random words"""
        if self._ix is None:
            qhi, qlo, n_absent = g.neighbour_queries(self.db, np.random.default_rng(3))
            hi, lo = np.concatenate([self.db["hi"], qhi]), np.concatenate([self.db["lo"], qlo])
            want = g.oracle_lookup(self.o, hi, lo)
            assert np.array_equal(want[:self.n], self.db["ix"]) and (want[self.n:self.n + n_absent] == 0xFFFFFFFF).all() and n_absent > 500
            self._ix = (hi, lo, want)
        return self._ix


_CASES = {}


def case_of(name, tmp_path_factory):
    if name not in _CASES:
        _CASES[name] = Case(name, str(tmp_path_factory.mktemp("geo_" + name)))
    return _CASES[name]


def build(torch, case, extra=None):
    """The image of the case's database under the table's environment (+ extra), in a tensor of torch's (read_regions reads its header);
    the table's figures and the model's very regions are asserted on the image before anything is searched."""
    t = case.t
    saved = {v: os.environ.get(v) for v in set(g.CLEAR) | set(extra or {})}
    try:
        for v in g.CLEAR:
            os.environ.pop(v, None)
        os.environ.update(t.env())
        os.environ.update(extra or {})
        raw = np.fromfile(case.db["ctr"], dtype=np.uint8)
        sz = t.W - 3 + t.I
        b0, r0 = 32, 32 + 4 * ctrfile.NUMBINS
        d_binix = torch.from_numpy(raw[b0:r0].copy()).cuda()
        d_records = torch.from_numpy(raw[r0:r0 + case.n * sz].copy()).cuda()
        torch.cuda.empty_cache()
        tree = DeviceTree.build_from_device(case.ctr, d_binix, d_records, 0)
        torch.cuda.synchronize()
    finally:
        for v, old in saved.items():
            if old is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = old
    hdr = g.read_regions(tree)
    slack0 = (extra or {}).get("UTREE_LUMP_SLACK") == "0"
    regions, n_slots, F = t.model(case.n)
    if slack0:
        regions, n_slots = g.regions_model(case.n, t.W, t.I, t.bucket_bytes // 8, F, t.target, slack=0.0)
    got = [(nb, sub) for _, sub, nb in hdr["regions"]]
    g.check_figures(t, got, hdr["n_slots"], hdr["fine_bits"])
    assert got == regions and hdr["n_slots"] == n_slots and hdr["fine_bits"] == F == tree.info.fine_bits
    assert hdr["bucket_words"] * 8 == t.bucket_bytes == tree.info.bucket_bytes and hdr["n_nodes"] == case.n
    return tree


def close(torch, tree):
    tree.close()
    tree._keep = None
    torch.cuda.empty_cache()


def table_bytes(t):
    return t.model()[1] * t.bucket_bytes


@pytest.fixture(scope="module", params=list(g.TABLES))
def table(request, torch_cuda, tmp_path_factory):
    """(case, tree) of one table: built once for the tests on it, closed before the next table is built"""
    t = g.TABLES[request.param]
    if request.param in ("C32", "C64sub"):
        free, _ = torch_cuda.cuda.mem_get_info()
        need = table_bytes(t) + (8 << 30)
        if free < need:
            pytest.skip("%s: hipMemGetInfo shows %.1f GiB of free HBM, the table plus 8 GiB is %.1f GiB" % (request.param, free / 2.0**30, need / 2.0**30))
    case = case_of(request.param, tmp_path_factory)
    tree = build(torch_cuda, case)
    yield case, tree
    close(torch_cuda, tree)


def check_classify(case, tree, monkeypatch, modes=(("1", "1"), ("1", "0"), ("0", "1")), sets=("short", "mixed")):
    """classify_fasta_bytes == the oracle's file, both strand modes, through the lane pass (one- and two-pass) and the wave-per-read kernels;
    the kernel names show which copy of the addressing ran"""
    t = case.t
    lanes = tree.info.lane_pass == 1
    assert lanes == (not (t.k == 64 and t.I == 4))
    nl = t.bucket_bytes // 64
    for lane_pass, bs in modes:
        if lane_pass == "1" and not lanes:
            continue                                                         # (k = 64 with u32 labels: the wave-per-read kernels only)
        monkeypatch.setenv("UTREE_LANE_PASS", lane_pass)
        monkeypatch.setenv("UTREE_LANES_BS", bs)
        for which in sets:
            for rc in (False, True):
                got = classify_fasta_bytes(case.ctr, tree, case.fasta[which], rc=rc)
                name = tree.kernel_name()
                if lane_pass == "1":
                    both = "true" if rc and bs == "1" and nl == 1 and tree.info.strand_views else "false"
                    head = "classify_lanes_k<%d, %d, %s," % (t.W, t.I, "1" if which == "short" else "16")
                    assert name.startswith(head) and name.endswith(", %d, %s>" % (nl, both)), name
                else:
                    assert ("classify_short_k" if which == "short" else "classify_long_k") in name, name
                assert got == case.want(which, rc), (case.name, lane_pass, bs, which, rc)
    tree.poll()


def check_get_ix(torch, case, tree):
    hi, lo, want = case.queries()
    t_lo = torch.from_numpy(lo.view(np.int64)).cuda()
    t_hi = torch.from_numpy(hi.view(np.int64)).cuda() if case.t.k == 64 else None
    got = tree.get_ix(t_hi, t_lo).cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (case.name, len(bad), [(hex(int(hi[j])), hex(int(lo[j])), int(got[j]), int(want[j])) for j in bad[:5]])


def test_classify_equals_the_oracle(table, monkeypatch):
    case, tree = table
    check_classify(case, tree, monkeypatch)


def test_get_ix_equals_the_oracle(table, torch_cuda):
    """every database word, the planted words with their 16-mer swapped for the h + 1 and h + 256 neighbours (absent: misses), 5 000 random words"""
    case, tree = table
    check_get_ix(torch_cuda, case, tree)


def test_hit_map_and_rank_search_equal_their_references(table, torch_cuda):
    """lookup_word's other callers: the hit map of the planted reads against hitmap_ref (the oracle per window), both strand modes, and the
    rank-specific search of all short reads against the oracle's, file to file"""
    case, tree = table
    torch = torch_cuda
    rng = np.random.default_rng(11)
    reads = case.reads["short"]
    planted = [r for r in reads if r[0][0] in "pj"]
    pick = [planted[int(i)] for i in rng.permutation(len(planted))[:500]] + [r for r in reads if r[0][0] in "rc"][:300] + case.reads["mixed"][:6]
    seqs = [s.encode() for _, s in pick]
    for rc in (False, True):
        maps = hitmap_ref.hitmap(case.db["ctr"], seqs, rc, o=case.o)
        assert sum(hitmap_ref.found_uix(m)[0] for m in maps) > 500
        assert_map(tree.hitmap(*device_reads(torch, seqs), rc=rc), maps)
    want = os.path.join(case.tmp, "rank_want.txt")
    out = os.path.join(case.tmp, "rank_got.txt")
    code, nr, good, err = orc.rank_search_file(case.o, case.path("short"), want, rc=True)
    assert code == 0 and nr == len(reads) and good > 300
    code, st = search_rank(case.ctr, tree, case.path("short"), out, rc=True, threads=4)
    assert code == lib.OK and st.n_reads == len(reads)
    assert open(out, "rb").read() == open(want, "rb").read()


@pytest.mark.parametrize("parts", [2, 7, 64])
@pytest.mark.parametrize("name", ["A", "B"])
def test_image_built_in_parts_on_slot_edges_that_are_no_power_of_two(torch_cuda, name, parts, tmp_path_factory, monkeypatch):
    """UTREE_BUILD_PARTS: the (hash, position, rest) order in parts cut on slot edges, each cut the smallest hash of a slot: ceil(slot * 2^24 / nb).
    The database's heavy value sits at the median of the hashes -- where 2 and 64 parts cut -- on the first value of its slot, with nodes on the
    last value of the slot before: every node must be found, and the reads classify as the oracle has them."""
    case = case_of(name, tmp_path_factory)
    tree = build(torch_cuda, case, {"UTREE_BUILD_PARTS": str(parts)})
    try:
        hi, lo, want = case.queries()
        n = case.n
        t_lo = torch_cuda.from_numpy(lo[:n].view(np.int64)).cuda()
        t_hi = torch_cuda.from_numpy(hi[:n].view(np.int64)).cuda() if case.t.k == 64 else None
        got = tree.get_ix(t_hi, t_lo).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, case.db["ix"]), "%d of %d nodes are not found" % (int((got != case.db["ix"]).sum()), n)
        check_classify(case, tree, monkeypatch, modes=(("1", "1"), ("0", "1")), sets=("short",))
    finally:
        close(torch_cuda, tree)


@pytest.mark.parametrize("variant", ["off64", "ovf_chains", "lump_slack0"])
def test_other_build_variants_on_table_A(torch_cuda, variant, tmp_path_factory, monkeypatch):
    """UTREE_FORCE_OFF64 (the 64-bit-offset instantiations), UTREE_OVF_CHAINS=1 (heavy runs as chains: the crowded part and the heavy value provide
    them) and UTREE_LUMP_SLACK=0 (at this load the same slot counts as the default: build() asserts the model's) on table A"""
    case = case_of("A", tmp_path_factory)
    extra = {"off64": {"UTREE_FORCE_OFF64": "1"}, "ovf_chains": {"UTREE_OVF_CHAINS": "1"}, "lump_slack0": {"UTREE_LUMP_SLACK": "0"}}[variant]
    tree = build(torch_cuda, case, extra)
    try:
        if variant == "ovf_chains":
            assert tree.info.overflow_chains == 1 and tree.info.overflow_bytes > 0
        if variant == "lump_slack0":
            assert [(nb, sub) for _, sub, nb in g.read_regions(tree)["regions"]] == case.t.model(case.n)[0]
            check_classify(case, tree, monkeypatch, modes=(("1", "1"),), sets=("short",))
        else:
            check_classify(case, tree, monkeypatch, sets=("short",))
            check_get_ix(torch_cuda, case, tree)
    finally:
        close(torch_cuda, tree)
