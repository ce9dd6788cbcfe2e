"""PACKSIZE=16 (k = 16, W = 4) on the GPU: BUILD / BUILD_GG (build_gpu.hip) and the rank-specific search (rank_kernels.hip, one
direct-address table load per examined window), against what the genuine reference does at -D PACKSIZE=16 (golden/k16_runs.json,
written by golden/make_golden_k16.py) and against the CPU oracle, which test_k16_cpu.py holds to the same reference.

A k = 16 device image is a table of 2^32 label ranks (8 GiB with 2-byte labels, 16 GiB with 4-byte ones), so trees are closed
as soon as a test is done with them; only the fixture's tree is kept for the module.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import ctrfile, lib
from utree_amd.search import CtrDB, DeviceTree, build, compress, frame_fasta, search_gg, search_rank
import k16_inputs as K
import util

RUNS = json.load(open(os.path.join(util.GOLD, "k16_runs.json")))
EXIT_OF = {lib.BUILD_E_MAP_EMPTY: 1, lib.BUILD_E_MAP: 2, lib.BUILD_E_FASTA: 2, lib.BUILD_E_NO_KMERS: 2, lib.BUILD_E_NAME: 4}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_TREES = {}


def fixture_tree():
    if "k16" not in _TREES:
        db = CtrDB.open(util.fixture_ctr("k16"))
        _TREES["k16"] = (db, DeviceTree.upload(db, 0))
    return _TREES["k16"]


def build_inputs(v, tmp_path):
    if v["set"].startswith("random"):
        fa_b, mp_b = K.random_refs(int(v["set"][len("random"):]))
    else:
        fa_b, mp_b = util.fixture_bytes("build_%s.fa.gz" % v["set"]), util.fixture_bytes("build_%s.map.gz" % v["set"])
    assert (K.sha256(fa_b), K.sha256(mp_b)) == (v["inputs"]["fa"], v["inputs"]["map"])
    fa, mp = tmp_path / "in.fa", tmp_path / "in.map"
    fa.write_bytes(fa_b)
    mp.write_bytes(mp_b)
    return str(fa), str(mp)


@pytest.mark.parametrize("tag", sorted(RUNS["build"]))
def test_build_k16_matches_reference(tag, tmp_path):
    """search.build(W=4) == `utree-build[GG]` -D PACKSIZE=16 [-D IXTYPE=uint32_t]: `.ubt` and `[.gg].log` bytes, node and label counts, or the
    same refusal with no file written."""
    v = RUNS["build"][tag]
    fa, mp = build_inputs(v, tmp_path)
    ubt = str(tmp_path / "o.ubt")
    log = ubt + (".gg.log" if v["gg"] else ".log")
    code, st = build(fa, mp, ubt, W=4, I=v["I"], complevel=v["complevel"], gg=bool(v["gg"]))
    if v["exit"] == 0:
        assert code == lib.OK
        assert (util.sha256_of(ubt), util.sha256_of(log)) == (v["outputs"]["ubt"], v["outputs"]["log"])
        assert ("Total nodes in tree: %d [%d labels]" % (st.n_nodes, st.n_labels)) in v["stdout_tail"]
        assert np.fromfile(ubt, dtype="<u8", count=4)[[0, 2]].tolist() == [4, v["I"]]          # the header: sizeof(WTYPE), sizeof(IXTYPE)
    else:
        assert code in (lib.E_BUILD, lib.E_IO) and EXIT_OF[st.error_kind] == v["exit"]
        assert v["outputs"]["ubt"] is None and not os.path.exists(ubt) and not os.path.exists(log)


@pytest.mark.parametrize("tag", ["rel_I2_gg_c1", "corner_I2_rank_c0", "random161_I4_gg_c2", "err_missing_I2_rank_c1"])
def test_build_cli_k16(tag, tmp_path):
    """`UTREE_PACKSIZE=16 utree-build[GG] in.fa in.map out.ubt 1 complevel`: the reference's stdout tail, exit code and files."""
    v = RUNS["build"][tag]
    fa, mp = build_inputs(v, tmp_path)
    ubt = str(tmp_path / "o.ubt")
    env = dict(os.environ, UTREE_PACKSIZE="16", UTREE_IXTYPE="32" if v["I"] == 4 else "16")
    exe = lib.BUILD_GG_CLI_PATH if v["gg"] else lib.BUILD_CLI_PATH
    r = subprocess.run([exe, fa, mp, ubt, "1", str(v["complevel"])], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == v["exit"], r.stderr.decode()
    assert r.stdout.decode().strip().splitlines()[-3:] == v["stdout_tail"]
    assert util.sha256_of(ubt) == v["outputs"]["ubt"]
    assert util.sha256_of(ubt + (".gg.log" if v["gg"] else ".log")) == v["outputs"]["log"]


@pytest.mark.parametrize("rc", [0, 1])
def test_rank_cli_k16_fixture(torch_cuda, rc, tmp_path):
    """`xtree-search` on the k = 16 fixture: the bytes of the reference's -D SEARCH -D PACKSIZE=16 build."""
    v = RUNS["rank"]["k16_rc%d" % rc]
    out = tmp_path / "o.txt"
    cmd = [lib.RANK_CLI_PATH, util.fixture_ctr("k16"), util.fixture_reads_path("k16"), str(out), "4"] + (["RC"] if rc else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == v["exit"] == 0, r.stderr.decode()
    assert util.sha256_of(str(out)) == v["outputs"]["out"]
    assert ("Good finds: %d" % v["lines"]) in r.stdout.decode()


def rank_case(name, tmp_path):
    if name in ("k16", "k16_random"):
        ctr = util.fixture_ctr("k16")
        data = util.fixture_bytes("k16_reads.fa.gz") if name == "k16" else K.rank_reads(K.db_words(ctrfile.read_ctr(ctr)), 1617)
    else:
        ctr, data = util.k16_table_cases(str(tmp_path))[name[len("table_"):]]
    return ctr, data


@pytest.mark.parametrize("name", sorted({t.rsplit("_rc", 1)[0] for t in RUNS["rank"]}))
def test_rank_k16_matches_reference(torch_cuda, name, tmp_path):
    """utree_rank_search_file == the reference's `xtree-search` -D PACKSIZE=16 on the fixture, seeded reads and the irregular tables, +-RC."""
    ctr, data = rank_case(name, tmp_path)
    fa = tmp_path / "r.fa"
    fa.write_bytes(data)
    db = CtrDB.open(ctr)
    tree = DeviceTree.upload(db, 0)
    try:
        for rc in (0, 1):
            v = RUNS["rank"]["%s_rc%d" % (name, rc)]
            assert (util.sha256_of(ctr), util.sha256_of(data)) == (v["inputs"]["ctr"], v["inputs"]["reads"])
            out = tmp_path / ("o%d.txt" % rc)
            code, st = search_rank(db, tree, str(fa), str(out), rc=bool(rc), threads=4)
            assert code == lib.OK
            assert util.sha256_of(str(out)) == v["outputs"]["out"]
            assert st.good_finds == v["lines"]
    finally:
        tree.close()


def run_batches(torch, db, tree, data, batch, rc, **prm):
    """The batch interface, `batch` reads at a time in file order (the carried hit array crosses the batch boundaries)."""
    fr = frame_fasta(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    n = len(fr["seq_off"])
    tree.rank_reset()
    recs = []
    for a in range(0, n, batch):
        b = min(n, a + batch)
        off = torch.from_numpy(fr["seq_off"][a:b].astype(np.int64)).cuda()
        ln = torch.from_numpy(fr["seq_len"][a:b].astype(np.int32)).cuda()
        recs.append(tree.rank_search(d_buf, off, ln, rc=rc, **prm).cpu().numpy())
    res = np.concatenate(recs) if recs else np.zeros((0, 6), np.int32)
    return db.format(buf, fr["name_off"], fr["name_len"], res, rank=True)


PARAMS = [dict(sparsity=s) for s in (1, 2, 3, 4, 8, 16)] + [dict(slack=1, sparsity=4, tolerance=1), dict(slack=3, sparsity=2, tolerance=3),
                                                           dict(slack=0, sparsity=16, tolerance=0)]


def check_vs_oracle(torch, db, tree, ctr, data, tmp_path, params, batches):
    fa = tmp_path / "r.fa"
    fa.write_bytes(data)
    o = orc.OracleDB.load(ctr)
    n = len(frame_fasta(data)["seq_off"])
    for prm in params:
        for rc in (False, True):
            want = tmp_path / "w.txt"
            code, nr, good, err = orc.rank_search_file(o, str(fa), str(want), rc=rc, **prm)
            assert code == 0 and nr == n, err
            w = want.read_bytes()
            out = tmp_path / "g.txt"
            code, st = search_rank(db, tree, str(fa), str(out), rc=rc, threads=4, **prm)
            assert code == lib.OK and st.n_reads == n
            assert out.read_bytes() == w, (prm, rc)
            for b in batches:
                assert run_batches(torch, db, tree, data, b, rc, **prm) == w, (prm, rc, b)


def test_rank_k16_vs_oracle_fixture(torch_cuda, tmp_path):
    """Seeded reads of 1 bp .. 40 kb (N's, lowercase, CRLF) on the k = 16 fixture, SPARSITY 1, 2, 3, 4, 8, 16 and SLACK / TOLERANCE variants,
    both strands: the file pipeline and the batch interface (batches of 97 and 1000 reads) give the oracle's bytes."""
    db, tree = fixture_tree()
    ctr = util.fixture_ctr("k16")
    data = K.rank_reads(K.db_words(ctrfile.read_ctr(ctr)), 1618)
    check_vs_oracle(torch_cuda, db, tree, ctr, data, tmp_path, PARAMS, (97, 1000))


@pytest.mark.parametrize("case", ["quirk", "dups", "generic", "ix32"])
def test_rank_k16_vs_oracle_irregular_tables(torch_cuda, case, tmp_path):
    """The irregular k = 16 tables (first-bin quirk, repeated and unsorted suffixes, a bin table that is not monotone, 4-byte labels): the
    direct-address table already holds the reference's probe-order answers, so the rank search needs no second path for them."""
    ctr, data = util.k16_table_cases(str(tmp_path))[case]
    db = CtrDB.open(ctr)
    tree = DeviceTree.upload(db, 0)
    try:
        check_vs_oracle(torch_cuda, db, tree, ctr, data, tmp_path, [dict(), dict(sparsity=1), dict(sparsity=16, slack=1, tolerance=1)], (50,))
    finally:
        tree.close()


def test_rank_k16_sparsity_bound(torch_cuda):
    """SPARSITY may be at most PACKSIZE = 16 (one window per step): 17 is refused, 16 runs."""
    import torch
    db, tree = fixture_tree()
    z = torch.full((64,), ord("A"), dtype=torch.uint8, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    ln = torch.full((1,), 40, dtype=torch.int32, device="cuda")
    with pytest.raises(lib.UtreeError):
        tree.rank_search(z, off, ln, sparsity=17)
    tree.rank_search(z, off, ln, sparsity=16)
    torch.cuda.synchronize()


def test_chain_k16_build_compress_search(torch_cuda, tmp_path):
    """Related genomes (300 x 20-100 kb) and 100 000 reads of 150 bp: GPU BUILD_GG -> GPU COMPRESS -> GPU SEARCH_GG and rank-specific
    SEARCH, +-RC; every link's bytes are the reference chain's.  The oracle's rank search on the same `.ctr` is held to it too."""
    ch = RUNS["chain"]
    fa_b, mp_b, seqs = K.chain_refs()
    reads = K.chain_reads(seqs)
    assert (K.sha256(fa_b), K.sha256(mp_b), K.sha256(reads)) == (ch["inputs"]["fa"], ch["inputs"]["map"], ch["inputs"]["reads"])
    fa, mp, rd = tmp_path / "c.fa", tmp_path / "c.map", tmp_path / "c_reads.fa"
    fa.write_bytes(fa_b)
    mp.write_bytes(mp_b)
    rd.write_bytes(reads)
    del fa_b, mp_b, seqs, reads
    ubt, ctr = str(tmp_path / "c.ubt"), str(tmp_path / "c.ctr")
    code, st = build(str(fa), str(mp), ubt, W=4, I=2, complevel=ch["complevel"], gg=True)
    assert code == lib.OK
    assert ("Total nodes in tree: %d [%d labels]" % (st.n_nodes, st.n_labels)) in ch["build"]["stdout_tail"]
    assert (util.sha256_of(ubt), util.sha256_of(ubt + ".gg.log")) == (ch["build"]["outputs"]["ubt"], ch["build"]["outputs"]["log"])
    code, _ = compress(ubt, ctr)
    assert code == lib.OK and util.sha256_of(ctr) == ch["compress"]["outputs"]["ctr"]
    db = CtrDB.open(ctr)
    tree = DeviceTree.upload(db, 0)
    o = orc.OracleDB.load(ctr)
    try:
        for rc in (0, 1):
            out = tmp_path / "gg.txt"
            code, _ = search_gg(db, [tree], str(rd), str(out), rc=bool(rc), threads=4)
            assert code == lib.OK and util.sha256_of(str(out)) == ch["searchGG_rc%d" % rc]["outputs"]["out"]
            out = tmp_path / "rank.txt"
            code, st = search_rank(db, tree, str(rd), str(out), rc=bool(rc), threads=4)
            assert code == lib.OK and util.sha256_of(str(out)) == ch["search_rc%d" % rc]["outputs"]["out"]
            assert st.good_finds == ch["search_rc%d" % rc]["lines"]
            code, _, _, err = orc.rank_search_file(o, str(rd), str(out), rc=bool(rc))
            assert code == 0 and util.sha256_of(str(out)) == ch["search_rc%d" % rc]["outputs"]["out"], err
    finally:
        tree.close()
