"""PACKSIZE=16 (k = 16) without a GPU: the oracle's rank-specific search held to the genuine `xtree-search` built with -D PACKSIZE=16
(golden/k16_runs.json, written by golden/make_golden_k16.py), the seeded inputs of the k = 16 runs, and the BUILD entry point's
acceptance of W = 4.  The GPU side is test_gpu_k16.py."""
import json
import os

import pytest

from oracle import orc
from utree_amd import ctrfile, lib
from utree_amd.search import build
import k16_inputs as K
import util

RUNS = json.load(open(os.path.join(util.GOLD, "k16_runs.json")))


def rank_case_inputs(name, tmp_path):
    """(ctr path, read bytes) of a rank entry of k16_runs.json, regenerated and checked against the hashes the reference ran on."""
    if name in ("k16", "k16_random"):
        ctr = util.fixture_ctr("k16")
        data = util.fixture_bytes("k16_reads.fa.gz") if name == "k16" else K.rank_reads(K.db_words(ctrfile.read_ctr(ctr)), 1617)
    else:
        ctr, data = util.k16_table_cases(str(tmp_path))[name[len("table_"):]]
    return ctr, data


@pytest.mark.parametrize("tag", sorted(RUNS["rank"]))
def test_oracle_rank_search_matches_reference_k16(tag, tmp_path):
    """orc.rank_search_file == `xtree-search` (-D SEARCH -D PACKSIZE=16[, IXTYPE=uint32_t]), byte for byte: the fixture, seeded reads
    on it, and the irregular tables (first-bin quirk, repeated suffixes, a bin table that is not monotone, 4-byte labels)."""
    v = RUNS["rank"][tag]
    ctr, data = rank_case_inputs(tag.rsplit("_rc", 1)[0], tmp_path)
    assert util.sha256_of(ctr) == v["inputs"]["ctr"] and util.sha256_of(data) == v["inputs"]["reads"]
    fa = tmp_path / "r.fa"
    fa.write_bytes(data)
    out = tmp_path / "o.txt"
    o = orc.OracleDB.load(ctr)
    assert o.k == 16
    code, nr, good, err = orc.rank_search_file(o, str(fa), str(out), rc=tag.endswith("_rc1"))
    assert code == v["exit"] == 0, err
    assert util.sha256_of(str(out)) == v["outputs"]["out"]
    assert good == v["lines"]


def test_regenerated_inputs_are_the_reference_runs_inputs():
    """The seeded BUILD sets and the chain's references and reads are the bytes the reference ran on."""
    for seed in K.RANDOM_SEEDS:
        fa, mp = K.random_refs(seed)
        v = RUNS["build"]["random%d_I2_gg_c0" % seed]
        assert (K.sha256(fa), K.sha256(mp)) == (v["inputs"]["fa"], v["inputs"]["map"])
    for nm in K.BUILD_SETS:
        v = RUNS["build"]["%s_I2_gg_c0" % nm]
        assert K.sha256(util.fixture_bytes("build_%s.fa.gz" % nm)) == v["inputs"]["fa"]
    fa, mp, seqs = K.chain_refs()
    ch = RUNS["chain"]["inputs"]
    assert (K.sha256(fa), K.sha256(mp)) == (ch["fa"], ch["map"])
    assert K.sha256(K.chain_reads(seqs)) == ch["reads"]


def test_reference_runs_cover_every_k16_build_mode():
    """Both builders, both label widths, complevel 0-4 on every committed set, and runs that the k = 32 builder refuses but k = 16 does not."""
    b = RUNS["build"]
    assert {(v["I"], v["gg"]) for v in b.values()} == {(2, 1), (2, 0), (4, 1), (4, 0)}
    assert {v["complevel"] for v in b.values() if v["set"] == "rel"} == {0, 1, 2, 3, 4}
    assert b["err_no_kmers_I2_gg_c0"]["exit"] == 0                   # 20 bases: k-mers at k = 16, none at k = 32
    assert all(v["W"] == 4 for v in b.values())


def test_build_file_accepts_w4(tmp_path):
    """utree_build_file(W = 4) is a k = 16 build, not an argument error: with or without a GPU it ends the way a W = 8 call does on the
    same box (here, without a GPU, both fail at the device); an unknown W is still refused."""
    fa, mp = tmp_path / "r.fa", tmp_path / "r.map"
    fa.write_bytes(util.fixture_bytes("build_rel.fa.gz"))
    mp.write_bytes(util.fixture_bytes("build_rel.map.gz"))
    codes = {}
    for W in (8, 4):
        ubt = tmp_path / ("w%d.ubt" % W)
        codes[W], st = build(str(fa), str(mp), str(ubt), W=W, I=2, complevel=1, gg=True)
        assert st.W == W
    assert codes[4] != lib.E_ARG
    assert codes[4] == codes[8]
    for W in (2, 12, 32):
        code, _ = build(str(fa), str(mp), str(tmp_path / "x.ubt"), W=W, I=2, complevel=1, gg=True)
        assert code == lib.E_ARG
