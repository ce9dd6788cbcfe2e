"""tests/ovf_inputs.py on the CPU: the hash inverse, the chosen cores, the builder's counts, the designed k-mers and their near misses
against the CPU oracle, and the image model against two specs counted by hand."""
import numpy as np
import pytest

from oracle import orc
import ovf_inputs as ov

CONFIGS = [(W, I, bb) for W, I in ((8, 2), (8, 4), (16, 2), (16, 4)) for bb in (64, 128)]


def test_hash_inverse_round_trips():
    rng = np.random.default_rng(1)
    for x in [0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFF, 0x8000] + [int(v) for v in rng.integers(0, 1 << 32, 5000)]:
        assert ov.unmix32(ov.mix32(x)) == x and ov.mix32(ov.unmix32(x)) == x
    # the numpy restatements agree with the scalar ones
    xs = rng.integers(0, 1 << 32, 2000).astype(np.uint64)
    assert np.array_equal(ov._mix32_np(xs.copy()), np.array([ov.mix32(int(x)) for x in xs], dtype=np.uint64))


def test_small_hashes_have_canonical_preimages():
    per_slot = [len(ov.cores_in_slot(s)) for s in range(64)]
    assert ov.unmix32(0) == 0 and ov.rc16(0) == 0xFFFFFFFF               # hash 0 is A^16's, canonical: 8320 values with it; it is skipped
    assert sum(per_slot) == 8320 - 1 and min(per_slot) >= 115
    for s in (1, 17, 63):
        for h, x in ov.cores_in_slot(s):
            assert h >> 8 == s and h != 0 and ov.mix32(x) == h and x < ov.rc16(x) and ov.rc16(ov.rc16(x)) == x


@pytest.mark.parametrize("W,I,bb", CONFIGS)
def test_chosen_cores_are_canonical_and_sit_in_their_slots(W, I, bb):
    for specs, slots in ((ov.thresholds_specs(W, I, bb), list(range(1, 13)) + [5, 12]), (ov.not_heavy_specs(W, I, bb), [20, 20, 21, 21]),
                         (ov.positions_specs(W, I, bb), [30, 31, 32, 33]), (ov.stretch_specs(W, I, bb), [34]), (ov.sixteen_bits_specs(W, I, bb), [40, 41]),
                         (ov.many_runs_specs(W, I, bb), [50 + b // 2 for b in range(200)])):
        assert len(specs) == len(slots)
        for s, slot in zip(specs, slots):
            assert s.core < ov.rc16(s.core) and s.hash >> 8 == slot and s.hash == ov.mix32(s.core)
            assert set(s.counts) <= set(ov.positions(4 * W))
        assert len({(s.core, s.orient) for s in specs}) == len(specs)
    CAP = ov.cap(W, I, bb)
    th = ov.thresholds_specs(W, I, bb)
    assert [s.n for s in th[:4]] == [CAP - 1, CAP, CAP + 1, CAP + 2] and [s.n - (CAP - 1) for s in th[4:12]] == list(ov.RUN_LENGTHS)
    assert (th[12].core, th[12].orient) == (th[4].core, 1 - th[4].orient) and len({ov.bucket_of(s) for s in th}) == len(th)
    nh = ov.not_heavy_specs(W, I, bb)
    assert nh[0].hash >> 8 == nh[1].hash >> 8 and nh[0].hash & 0xFF != nh[1].hash & 0xFF and nh[0].orient == nh[1].orient


def _placed_counts(built):
    v = ov.views(built.bases)
    got = {}
    for h, o, p, s in zip(v["hf"], v["of"], v["pf"], built.spec_of):
        if s >= 0:
            got[(int(h), int(o), int(p))] = got.get((int(h), int(o), int(p)), 0) + 1
    return got


@pytest.fixture(scope="module")
def small_dbs(tmp_path_factory):
    """thresholds + not heavy + positions, k = 32 and 64, with filler: built once."""
    out = {}
    d = tmp_path_factory.mktemp("ovf")
    for W in (8, 16):
        specs = ov.thresholds_specs(W, 2, 64) + ov.not_heavy_specs(W, 2, 64) + ov.positions_specs(W, 2, 64) + ov.stretch_specs(W, 2, 64)
        b = ov.build(4 * W, specs, seed=W, filler=3000)
        out[W] = (b, b.write(str(d / ("cpu%d.ctr" % W)), 2))
    return out


@pytest.mark.parametrize("W", [8, 16])
def test_builder_places_the_counts_of_the_spec(small_dbs, W):
    b, _ = small_dbs[W]
    want = {(s.hash, s.orient, p): n for s in b.specs for p, n in s.counts.items() if n}
    assert _placed_counts(b) == want
    assert b.n_designed == sum(s.n for s in b.specs) and len(b.bases) == b.n_designed + 3000
    v = ov.views(b.bases[b.spec_of < 0])
    assert int(v["hf"].min()) >= 1 << 20                                 # no filler k-mer in a designed bucket
    assert len(set(zip(b.hi.tolist(), b.lo.tolist()))) == len(b.lo)      # all distinct


@pytest.mark.parametrize("W", [8, 16])
def test_oracle_finds_every_placed_kmer_and_no_near_miss(small_dbs, W):
    b, ctr = small_dbs[W]
    o = orc.OracleDB.load(ctr)
    reads, rows, third, miss = ov.reads_for(b, seed=5)
    assert len(rows) == b.n_designed and len(miss) >= len(third)         # (two per k-mer asked for; at least half could be made)
    for r in rows:
        assert o.lookup(int(b.hi[r]), int(b.lo[r])) == int(b.ix[r]), r
    hi, lo = ov.pack(miss)
    for a, c in zip(hi, lo):
        assert o.lookup(int(a), int(c)) == 0xFFFFFFFF
    # a near miss keeps its k-mer's minimizer: hash, orientation and position all occur among the designed ones
    placed = set(_placed_counts(b))
    v = ov.views(miss)
    assert all((int(h), int(oo), int(p)) in placed for h, oo, p in zip(v["hf"], v["of"], v["pf"]))
    # the first and the last k-mer of every (spec, position) in key order, whatever the sample
    edge = ov.boundary_rows(b)
    groups = {(int(s_), int(p)) for s_, p in zip(b.spec_of[rows], b.pos_of[rows])}
    assert set(edge) <= set(rows) and {(int(b.spec_of[r]), int(b.pos_of[r])) for r in edge} == groups and len(groups) <= len(edge) <= 2 * len(groups)
    few = ov.reads_for(b, seed=5, sample=50)
    assert set(edge) <= set(few[1]) and set(edge) <= set(few[2]) and len(few[1]) <= 50 + len(edge)
    rest = {int(r): ov.text(np.delete(b.bases[r], np.arange(b.pos_of[r], b.pos_of[r] + 16))) for r in rows}
    for s_, p in groups:
        grp = [int(r) for r in rows if b.spec_of[r] == s_ and b.pos_of[r] == p]
        assert min(grp, key=rest.get) in edge and max(grp, key=rest.get) in edge
    # the reads: (a) .. (c) and as many reverse complements, then the random ones
    names = [n for n, _ in reads]
    n_abc = sum(1 for n in names if n[0] in "abc")
    assert n_abc == sum(1 for n in names if n.startswith("d_")) and sum(1 for n in names if n[0] == "e") == 300
    k = 4 * W
    sliding = [s for n, s in reads if n.startswith("c")]
    assert sliding and all(len(s) == k + k - 16 for s in sliding)
    assert len(sliding) == sum(len(s.counts) + 1 for s in b.specs)
    o.close()


def test_model_equals_two_hand_computed_specs():
    # (1) k = 32, u16 labels, 64-byte buckets: CAP = 8, one-word records, a directory of 18 offsets = 36 bytes = 5 slots.
    #     39 k-mers: 7 inline + a run of 32 (not heavy: 32 slots).  40 k-mers: 7 inline + a run of 33 (heavy: 33 + 5 slots).  70 slots, 560 bytes.
    specs = [ov.Spec(ov._pick(3), 0, ov.spread(32, 39)), ov.Spec(ov._pick(4), 1, ov.spread(32, 40))]
    b = ov.build(32, specs, seed=9)
    m = ov.model(b, 2, 64)
    assert m["slots"] == 70 and m["bytes"] == 560 and [(r[2], r[3], r[4]) for r in m["runs"]] == [(32, False, 32), (33, True, 38)]
    assert ov.model(b, 2, 64, dir_on=False)["slots"] == 65
    assert m["ovf_scan"] == 16                                            # 70 * 4 > 79 nodes
    #     the same k-mers with u32 labels in 128-byte buckets: CAP = 8 again (two-word records), 3 directory slots, 16-byte slots
    m = ov.model(b, 4, 128)
    assert m["slots"] == 32 + 33 + 3 and m["bytes"] == 68 * 16
    #     k = 64, u32 labels, 128-byte buckets: CAP = 4, four-word records, 50 offsets = 100 bytes = 4 slots
    specs = [ov.Spec(ov._pick(3), 0, ov.spread(64, 35)), ov.Spec(ov._pick(4), 1, ov.spread(64, 36))]
    m = ov.model(ov.build(64, specs, seed=10), 4, 128)
    assert m["slots"] == 32 + 33 + 4 and m["bytes"] == 69 * 32
    # (2) no heavy run: 20 + 20 k-mers of two hash values in one bucket (7 inline, a run of 33 that holds both values: 33 slots, no
    #     directory), a bucket of 8 (all inline: nothing), a bucket of 9 (7 inline, a run of 2).  35 slots, 280 bytes.
    two = ov.cores_in_slot(6)
    specs = [ov.Spec(two[0][1], 1, ov.spread(32, 20)), ov.Spec(two[1][1], 1, ov.spread(32, 20)),
             ov.Spec(ov._pick(7), 0, ov.spread(32, 8)), ov.Spec(ov._pick(8), 0, ov.spread(32, 9))]
    b = ov.build(32, specs, seed=11, filler=500)
    m = ov.model(b, 2, 64)
    assert m["slots"] == 35 and m["bytes"] == 280 and sorted((r[2], r[3]) for r in m["runs"]) == [(2, False), (33, False)]
    assert ov.model(b, 2, 64, dir_on=False)["slots"] == 35 and m["ovf_scan"] == 32            # 35 * 4 <= 549 nodes
    #     ... and were the 20 + 20 one hash value's, the run would be heavy
    specs[1] = ov.Spec(ov._pick(9), 1, ov.spread(32, 20))
    specs[0] = ov.Spec(two[0][1], 1, ov.spread(32, 40))
    assert ov.model(ov.build(32, specs, seed=12), 2, 64)["slots"] == 33 + 5 + 13 + 2


def test_directory_appears_between_32_and_33_in_every_configuration():
    for W, I, bb in CONFIGS:
        specs = ov.thresholds_specs(W, I, bb)
        m = ov.model(ov.build(4 * W, specs, seed=3), I, bb)
        by_bucket = {r[0]: r for r in m["runs"]}
        CAP, D = ov.cap(W, I, bb), ov.dir_slots(W, I)
        for s in specs:
            c = s.n - (CAP - 1)
            r = by_bucket.get(ov.bucket_of(s))
            if s.n <= CAP:
                assert r is None
            else:
                assert r[1:] == (s.n, c, c > 32, c + (D if c > 32 else 0)), (W, I, bb, s.name)
        assert D == {(8, 2): 5, (8, 4): 3, (16, 2): 7, (16, 4): 4}[(W, I)]


def test_chain_model_on_a_run_counted_by_hand():
    # k = 32, u16 labels, 64-byte buckets.  One stretch and its sibling: 17 + 16 k-mers; key order is position, then outer bases, so the 7 inline
    # records are the one at position 0, the two at 1, 2 and 3: the run holds positions 4 .. 16 of both, 26 records -- not heavy.  Three
    # stretches: 99 k-mers, 7 inline (position 0: three, position 1: four of the six), a run of 92.  Its chains: each stretch's and each
    # sibling's records at 2 .. 16 follow one another (6 chains); the two records left at position 1 start chains of their own only if
    # nothing follows them at position 2 -- but a record at 2 follows the record at 1 of its own stretch, so they are the heads of two of the
    # six.  6 chains: 12 words, 92 ranks of 2 bytes: 23 words.  35 slots against 92 + 5 behind a directory.
    s1 = ov.stretch_spec(32, ov._pick(34), 0, 1, 1, "one")
    assert s1.n == 33 and s1.counts[0] == 1 and all(s1.counts[p] == 2 for p in range(1, 17))
    m = ov.model(ov.build(32, [s1], seed=1), 2, 64, chains=True)
    assert [(r[2], r[3], r[4]) for r in m["runs"]] == [(26, False, 26)]
    s3 = ov.stretch_spec(32, ov._pick(34), 0, 3, 2, "three")
    b = ov.build(32, [s3], seed=2)
    assert [(r[2], r[3], r[4]) for r in ov.model(b, 2, 64)["runs"]] == [(92, True, 97)]
    assert [(r[2], r[3], r[4]) for r in ov.model(b, 2, 64, chains=True)["runs"]] == [(92, True, 35)]
    # u32 labels: two-word slots, 12 + 46 words = 29 slots
    assert [(r[2], r[3], r[4]) for r in ov.model(b, 4, 128, chains=True)["runs"]] == [(92, True, 29)]
    # every record a chain of its own (random flanks): 40 records, 33 in the run, 66 + 9 words
    r = ov.build(32, [ov.Spec(ov._pick(4), 1, ov.spread(32, 40))], seed=9)
    assert ov.model(r, 2, 64, chains=True)["slots"] == 75
