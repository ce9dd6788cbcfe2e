"""The inputs of the bucket-addressing tests (test_gpu_geometry.py), checked where no GPU is needed: the Python port of the region sizing
(geometry_inputs.regions_model) against the library's own image size, the figures each table is meant to show -- regions whose slot count is no
power of two, regions at the cap, at the floor, one value per slot --, the inverse of the minimizer hash, and the planted k-mers: every class
of them holds a k-mer whose planted 16-mer IS its minimizer (else the GPU tests would prove nothing about that edge), and the oracle finds
every database k-mer under its own label."""
import numpy as np
import pytest

from oracle import orc
from utree_amd import lib
from utree_amd.search import CtrDB
import geometry_inputs as g


def set_env(monkeypatch, t):
    for v in g.CLEAR:
        monkeypatch.delenv(v, raising=False)
    for key, v in t.env().items():
        monkeypatch.setenv(key, v)


@pytest.mark.parametrize("name", sorted(g.TABLES))
def test_region_model_equals_the_library_and_tables_show_their_figures(name, monkeypatch):
    """utree_dev_image_bytes under the table's environment = layout() over the model's n_slots, at the nominal node count and 1 % off it; the
    automatic width under UTREE_TABLE_MAX_GB is the model's pick."""
    t = g.TABLES[name]
    set_env(monkeypatch, t)
    L = lib.load()
    bins = np.zeros((1 << 24) + 1, dtype=np.uint64)
    for n in (t.n_nodes, t.n_nodes - t.n_nodes // 100, t.n_nodes + t.n_nodes // 100):
        regions, n_slots, F = t.model(n)
        bins[-1] = n
        db = CtrDB.from_memory(t.W, t.I, n, bins, None, b"k__A;p__B\t1\n")
        got = L.utree_dev_image_bytes(db._h, lib.FINE_AUTO)
        db.close()
        assert got == g.layout_bytes(n, t.W, t.I, t.bucket_bytes // 8, n_slots, [9]), (name, n)
        g.check_figures(t, regions, n_slots, F)
    regions, n_slots, F = t.model()
    if t.nb0 is not None and t.nb0 != 1 << 24:
        assert regions[0][0] == t.nb0                                       # at the nominal count: the issue's figure to the slot
    if name == "Aauto":
        assert F == 3 and regions == g.TABLES["A3"].model()[0]              # (a different size from fine_bits 8 proves the library coarsened too)


def test_lump_slack_zero_gives_the_same_table_at_this_load():
    t = g.TABLES["A"]
    assert g.regions_model(t.n_nodes, t.W, t.I, 8, 8, t.target, slack=0.0) == t.model()[:2]


def test_hash_inverse_and_the_two_minimizers_agree():
    rng = np.random.default_rng(1)
    for x in [0, 1, 0xFFFFFFFF, 0x80000000] + [int(v) for v in rng.integers(0, 1 << 32, 2000)]:
        assert g.unmix32(g.mix32(x)) == x and g.mix32(g.unmix32(x)) == x
        assert g.rc16(g.rc16(x)) == x
    assert g.mer_str(g.rc16(g.mer_int("ACGTTTGACCAGTCAA"))) == g.revcomp("ACGTTTGACCAGTCAA")
    for k in (32, 64):
        c = rng.integers(0, 4, (300, k), dtype=np.uint8)
        p, h = g.minimizers(c, k)
        for s, pp, hh in zip(g.strs_of(c), p, h):
            assert g.minimizer(s, k) == (int(pp), int(hh))
        hi, lo = g.pack(c)
        assert np.array_equal(g.unpack(hi, lo, k), c)
    # k = 64: positions 0, 1, 47, 48 never count
    s = g.mer_str(g.unmix32(0)) + g.rand_seq(rng, 48)
    assert g.minimizer(s, 64)[0] >= 2 and g.minimizer(s[:32], 32) == (0, 0)


@pytest.mark.parametrize("name", ["A", "B", "C64"])
def test_boundary_db_is_live(name, tmp_path):
    t = g.TABLES[name]
    regions, n_slots, F = t.model()
    db = g.boundary_db(regions, t.k, t.I, 7, str(tmp_path / "b.ctr"), t.n_nodes)
    n = len(db["lo"])
    assert abs(n - t.n_nodes) <= t.n_nodes // 100                           # the table depends on the node count
    assert abs(t.model(n)[0][0][0] - regions[0][0]) <= regions[0][0] // 100
    # every planted class but the margin's holds a k-mer whose planted 16-mer is its minimizer, at the planted hash value
    classes = db["planted"]
    want_regions = g.planted_regions(regions)
    assert {key[0] for key in classes} == set(want_regions) and len(want_regions) == 5
    for (r, kind, o, pos), kmers in classes.items():
        exempt = t.k == 64 and pos in g.MARGIN_POS
        assert exempt or (r, kind, o, pos) in db["live"], (r, kind, o, pos)
        for s in kmers:
            m = g.mer_int(s[pos:pos + 16])
            h = g.mix32(min(m, g.rc16(m)))
            assert h >> 24 == r and (m > g.rc16(m)) == bool(o)
            assert exempt or g.minimizer(s, t.k) == (pos, h)
    kinds = {key[1] for key in classes}
    assert {"region_first", "region_last"} <= kinds and sum(1 for x in kinds if x.endswith("_first")) == 9 and sum(1 for x in kinds if x.endswith("+256")) >= 14
    # the slot edges are edges: first / last values of adjacent slots, and + 256 is another slot with the same low 8 bits
    for r in want_regions:
        nb = regions[r][0]
        for kind, h in g.planted_hashes(r, nb):
            if kind.endswith("_first") and kind.startswith("slot"):
                s = g.slot_of(h, nb)
                assert g.first_of_slot(s, nb) <= (h & 0xFFFFFF) and g.slot_of(g.first_of_slot(s, nb) - 1, nb) == s - 1
    # the heavy value: first of its slot, its neighbours in the slot before, and the median of the nodes' hashes is on it
    hv = db["heavy"]
    nb = hv["nb"]
    assert nb == regions[hv["region"]][0] and nb & (nb - 1)                  # no power of two there
    assert g.first_of_slot(hv["slot"], nb) == hv["h"] & 0xFFFFFF and hv["last"] == hv["h"] - 1
    assert g.slot_of(hv["last"], nb) == g.slot_of(hv["low"], nb) == hv["slot"] - 1 and hv["low"] < hv["last"]
    assert (hv["h"] << 24) % nb != 0                                         # floor and ceil of the edge differ
    for key in ("last", "low"):
        assert len(hv[key + "_kmers"]) >= 4
        for s in hv[key + "_kmers"]:
            assert g.minimizer(s, t.k)[1] == hv[key]
    _, hs = g.minimizers(g.unpack(db["hi"], db["lo"], t.k), t.k)
    hs = np.sort(hs)
    assert int(hs[len(hs) // 2]) == hv["h"] and int((hs == np.uint32(hv["h"])).sum()) >= hv["n"] - 24
    # the oracle finds every node under its own label, and none of the absent neighbours
    o = orc.OracleDB.load(db["ctr"])
    assert np.array_equal(g.oracle_lookup(o, db["hi"], db["lo"]), db["ix"])
    qhi, qlo, n_absent = g.neighbour_queries(db, np.random.default_rng(3))
    assert n_absent > 500 and (g.oracle_lookup(o, qhi[:n_absent], qlo[:n_absent]) == 0xFFFFFFFF).all()
    reads = g.geometry_reads(db, np.random.default_rng(5))
    assert 3000 < len(reads) < 20000 and max(len(s) for _, s in reads) >= 3000
