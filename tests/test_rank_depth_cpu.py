"""The inputs of tests/test_gpu_rank_depth.py, checked without a GPU: (a) the layout conditions that make the depth file
reach every level of the rank kernels' max tree, asserted from the ORACLE's hit counts; (b) the oracle held to the genuine
`xtree-search` binaries on those files (SHA-256 recorded in golden/reference_runs.json from oracle/_ref; the inputs come
from the committed seeds)."""
import numpy as np
import pytest

from oracle import orc
import rank_inputs as ri
import util

BATCHES = (300000, 262144, 262145, 4096, 65537)           # the batch sizes of the GPU test


def test_depth_case_shape():
    c = ri.depth_case(1)
    assert c.n >= 2 * 262144 + 4096 + 64 + 1 and c.n % 64 and (c.n // 64) % 64      # a part block, a part group, a part supergroup
    nh = c.records["found"]
    assert 0.68 < np.mean(nh == 1) < 0.72 and 0.28 < np.mean(nh == 0) < 0.32
    assert 200 <= int(np.sum(nh == 2)) <= 400
    assert int(nh.max()) == 45 and set(range(2, 43)) <= set(nh.tolist())            # the staircases
    assert len(np.unique(c.own1[c.own1 >= 0])) == 48 and np.bincount(c.own1[c.own1 >= 0]).min() > 1000
    assert 16e6 < len(c.data) < 20e6


def test_depth_case_reaches_every_tier():
    """From the oracle's hit counts alone: where each voting read's donor -- the latest earlier read with more hits -- lies
    (monotonic stack), that every tier holds >= 100 voting reads (and tiers 1-4 >= 5 with several hits), and that in every
    tier >= 20 reads get another record if that tier is skipped: if the read picks up from the latest candidate BEFORE its
    block (tier 1), its group (2), its supergroup (3), or from the untouched array (4); for tier 5, if the entry matched
    none of the read's labels.  The records this model gives for the true donors are the oracle's, read for read.
    What is counted is a change of the read's OUTPUT LINE -- any of printed, label, most, secondMost -- not of the label
    field alone: 99.9 % of the voting reads keep one hit, and such a read's label is its own hit's whatever it picks up
    (a matching entry makes it 2 : 0 and printed, any other 1 : 1 and not printed), so for them the entry decides whether
    the line exists, never which label it names.  By label alone the counts would be 19 / 59 / 16 / 1 / 0."""
    c = ri.depth_case(1)
    nh = c.records["found"].astype(np.int64)
    voting = np.flatnonzero(nh > 0)
    donor = ri.prev_greater(nh)[voting]
    tier = ri.tier_of(voting, donor)
    entry = ri.depth_labels_at(c, donor, nh[voting])
    truth = ri.depth_outcome(c, voting, entry)
    rec = c.records[voting]
    assert np.array_equal(truth[:, 1], rec["most"]) and np.array_equal(truth[:, 2], rec["second"])
    assert np.array_equal(truth[:, 3], rec["printed"]) and np.array_equal(truth[:, 0], rec["label"])
    bound = np.select([tier == 1, tier == 2, tier == 3], [voting & ~63, voting & ~4095, voting & ~262143], 0)
    alt_q = ri.prev_greater_before(nh, voting, bound)
    alt = ri.depth_labels_at(c, alt_q, nh[voting])
    alt[tier == 5] = 48                                   # no label of the database
    changed = np.any(ri.depth_outcome(c, voting, alt) != truth, axis=1)
    for t in (1, 2, 3, 4, 5):
        m = tier == t
        print("tier %d: %d voting reads, %d with several hits, %d change if it is skipped" %
              (t, m.sum(), (m & (nh[voting] > 1)).sum(), (m & changed).sum()))
        assert m.sum() >= 100 and (m & changed).sum() >= 20
        assert t == 5 or (m & (nh[voting] > 1)).sum() >= 5
    # a read with 41 hits in the last supergroup takes from supergroup 0 PAST supergroup 1, whose richest read has 41
    far = voting[(tier == 4) & ((voting >> 18) - (donor >> 18) == 2)]
    assert len(far) >= 1 and nh[far].max() == 41
    # split into batches, the reads whose donor lies before their batch take the entry from the carried array
    for b in BATCHES:
        carried = (donor >= 0) & (donor < voting - voting % b)
        lost = ri.depth_outcome(c, voting[carried], np.zeros(int(carried.sum()), dtype=np.int64))
        n_changed = int(np.any(lost != truth[carried], axis=1).sum())
        print("batches of %d: %d reads take a carried entry, %d change if it reads as 0" % (b, carried.sum(), n_changed))
        assert carried.sum() >= 100 and n_changed >= 20
    assert int(np.flatnonzero(nh > 0)[0]) >= 5            # the GPU test's first batch of zero-hit reads only


def test_vote_split_case_counts():
    v = ri.vote_split_case(1)
    for prm in (dict(slack=2, sparsity=4, tolerance=2), dict(slack=1, sparsity=4, tolerance=1)):
        r = ri.oracle_records("rk", v.data, **prm)
        cnt = np.bincount(r["found"][v.targets])
        assert set(np.flatnonzero(cnt).tolist()) == {62, 63, 64, 65} and cnt[62:66].min() >= 100
        assert int(np.sum(r["found"] >= 64)) > 2300      # the GPU test needs more of these than n_cu * 8 (2 048 on 256 CUs)
        p = r["printed"][v.targets]
        assert (prm["slack"] == 1 and p.all()) or 0.3 < p.mean() < 0.7
    # what the planted entry does to the target's record: every mix sees >= 3 different records over its four donors
    r = ri.oracle_records("rk", v.data)
    t = r[v.targets].reshape(-1, 4)                       # [.., which = A, B, C, other]
    assert np.mean([len(set(map(tuple, row.tolist()))) >= 3 for row in t]) > 0.9
    assert any(row[0]["label"] != row[1]["label"] for row in t)                     # the entry moved the first place


@pytest.mark.parametrize("name", ["rk", "k64"])
def test_edge_and_joint_cases_hit_where_they_should(name):
    e = ri.edge_case(name)
    f, r = ri.oracle_records(name, e.data)["found"], ri.oracle_records(name, e.data, rc=True)["found"]
    assert f[e.fwd].min() >= 2 and r[e.fwd].min() >= 2 and r[e.rc].min() >= 2
    k = ri.db_kmers(name).k
    off, ln = ri.frame(e.data)
    # WHERE the oracle's hits fall, from its hit counts on prefixes: one at the planted window, none until the second
    # one's window (register pair: S .. k-S windows on; run of database windows: k on; overlapping pair: none at the
    # overlapping k-mer, one at the third), or none to the read's end where the read is cut there
    assert sorted(p.read for p in e.planted) == list(range(e.n))
    for p in e.planted:
        s = e.data[int(off[p.read]):int(off[p.read]) + int(ln[p.read])]
        assert ri.planted_ok(name, s + b"N" + ri.revcomp(s) if p.rc else s, k, p.w, p.second, p.base), p
        if p.kind == 1 and p.second >= 0:
            assert k // 4 <= p.second - p.w <= k - 1
    kinds = (0, 1) if k == 32 else (2,)
    whole = lambda rc: {(p.w, p.kind) for p in e.planted if p.rc == rc and p.second >= 0}
    assert whole(False) == {(w, kd) for w in ri.EDGE_STARTS for kd in kinds}
    # on the reverse strand, which starts at window L + 1: every start from 959 on; 63 and 64 with the register pair only
    assert whole(True) >= {(w, kd) for w in ri.EDGE_STARTS[2:] for kd in kinds} | ({(63, 1), (64, 1)} if k == 32 else set())
    assert {(p.w, int(ln[p.read]) - k + 1) for p in e.planted if not p.rc} >= {(w, n) for w in ri.EDGE_STARTS for n in ri.EDGE_WINDOWS if n > w}
    assert {959, 960, 961, 1920, 1921} <= set((ln.astype(np.int64) - k + 1).tolist())
    assert {960, 1920} <= set((2 * ln[e.rc].astype(np.int64) + 2 - k).tolist())
    j = ri.joint_case(name)
    f, r = ri.oracle_records(name, j.data)["found"], ri.oracle_records(name, j.data, rc=True)["found"]
    _, ln = ri.frame(j.data)
    assert np.all(ln[j.short] < k) and np.all(2 * ln[j.short] + 1 >= k) and not r[j.short].any() and not f[j.short].any()
    assert {k - 1, k, k + 1} <= set(ln.tolist())
    assert np.all(f[j.last_fwd] == 1) and np.all(r[j.last_fwd] >= 1)
    assert np.all(f[j.first_rev] == 0) and np.all(r[j.first_rev] == 1)


def test_workspace_case_fills_its_reservations():
    for mixed, want in ((False, {511}), (True, {511, 512, 513})):
        data = ri.workspace_case(mixed)
        _, ln = ri.frame(data)
        reserve = (ln.astype(np.int64) - 31 + 7) // 8     # ceil(windows / 8)
        assert set(reserve.tolist()) == want
        f = ri.oracle_records("rk", data)["found"]
        assert np.array_equal(f[0::2], reserve[0::2])     # the all-'A' reads fill theirs to the last entry
        assert np.all(f[1::2] >= 128)


CASES = {"rank_depth_1": lambda: ri.depth_case(1).data, "rank_split_1": lambda: ri.vote_split_case(1).data}


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank_depth")
    out = {}
    for key, make in CASES.items():
        out[key] = (make(), str(d / (key + ".fa")))
        open(out[key][1], "wb").write(out[key][0])
    return out


@pytest.mark.parametrize("key,sfx,prm", [("rank_depth_1", "", dict()), ("rank_depth_1", "_p32s1t1", dict(slack=1, sparsity=32, tolerance=1)),
                                         ("rank_split_1", "", dict()), ("rank_split_1", "_p32s1t1", dict(slack=1, sparsity=32, tolerance=1)),
                                         ("rank_split_1", "_s1t1", dict(slack=1, sparsity=4, tolerance=1))])
def test_oracle_vs_reference_on_generated_files(key, sfx, prm, case_files, tmp_path):
    """The oracle's whole-file run on the generated files == what the genuine xtree-search, xtree-search-p32s1t1 and (the
    vote-split file, whose GPU test runs SLACK = 1, TOLERANCE = 1) xtree-search-s1t1 binaries wrote on them."""
    data, fa = case_files[key]
    want = util.reference_run(key + sfx, ctr=util.fixture_ctr("rk"), fa=data)
    assert want["exit"] == 0
    got = tmp_path / "orc.txt"
    code, nr, good, err = orc.rank_search_file(ri.oracle_db("rk"), fa, str(got), **prm)
    assert code == 0 and nr == data.count(b">") and good > 1000
    assert util.sha256_of(str(got)) == want["outputs"]["out"]
