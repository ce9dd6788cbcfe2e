"""GPU tests of long queries tile by tile (csrc/tiles_kernels.hip, csrc/tiles.c, csrc/tiles_file.c, `utree-tiles`): plan and views must equal
numpy, the classification of the views the CPU oracle tile by tile, and every file tests/tiles_ref.py -- the contract restated, pinned to the
genuine reference's outputs in tests/test_tiles_cpu.py.  All comparisons are exact: there is no tolerance in this feature.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pairs_ref
import tiles_ref
import util
from test_tiles_cpu import ref
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, frame_fasta, tiles_file


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_TREES = {}


def tree_for(name):
    if name not in _TREES:
        db = CtrDB.open(util.fixture_ctr(name))
        _TREES[name] = (db, DeviceTree.upload(db, 0))
    return _TREES[name]


def device_queries(torch, name):
    """the committed contigs as the file run uploads them: the FASTA's own bytes, the framing's offsets"""
    data = tiles_ref.contigs(name)
    fr = frame_fasta(data)
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    return (torch.from_numpy(buf).cuda(), torch.from_numpy(fr["seq_off"].astype(np.int64)).cuda(),
            torch.from_numpy(fr["seq_len"].astype(np.int32)).cuda(), fr)


def views_np(t):
    return [x.cpu().numpy().view(d) for x, d in zip(t, (np.uint64, np.uint32, np.uint32, np.uint32))]


# ---- a. plan and views against numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("WS", ["k,1", (150, 75), (200, 200), (1000, 1), (5000, 77), (lib.TILE_MAX_BP, lib.TILE_MAX_BP)])
def test_plan_and_views_equal_numpy(torch_cuda, WS):
    """(1000, 1): the 3 kb query has 2 002 tiles beside queries of one; the last two: W larger than every query"""
    db, tree = tree_for("vote")
    W, S = (db.k, 1) if WS == "k,1" else WS
    bases, off, ln, fr = device_queries(torch_cuda, "vote")
    first, toff, tlen, tq, ti = tiles_ref.numpy_views(fr["seq_off"], fr["seq_len"], W, S)
    total = int(first[-1])
    assert total == sum(tiles_ref.n_tiles(int(L), W, S) for L in fr["seq_len"])
    tile_first, meta = tree.tiles_plan(ln, W, S)
    assert meta == dict(total_tiles=total, total_bases=0, max_len=0, error=0)
    assert np.array_equal(tile_first.cpu().numpy().view(np.uint64), first)
    # the whole batch; ranges that begin and end inside a query; one tile; the empty range, in front, inside and at the end
    big = int(np.argmax(fr["seq_len"]))
    a = int(first[big])
    ranges = [(0, total), (0, 1), (total - 1, 1), (0, 0), (total, 0), (a, 0)]
    if first[big + 1] - first[big] > 4:
        ranges += [(a + 1, int(first[big + 1]) - a - 2), (a + 2, 1), (max(a - 3, 0), 7)]
    for f0, n in ranges:
        got = tree.tiles_views(off, ln, W, S, tile_first, f0, n)
        m = got[4]
        want = [x[f0:f0 + n] for x in (toff, tlen, tq, ti)]
        assert m == dict(total_tiles=total, total_bases=int(want[1].astype(np.int64).sum()), max_len=int(want[1].max()) if n else 0, error=0), (f0, n)
        for g, w in zip(views_np(got[:4]), want):
            assert np.array_equal(g, w), (f0, n)
    # a range that ends behind the tiles: error 1, and nothing is written
    for f0, n in ((total, 1), (total - 1, 2), (total + 5, 0)):
        sentinel = torch_cuda.full((4,), -7, dtype=torch_cuda.int64, device=off.device)
        L = lib.load()
        d_meta = torch_cuda.zeros(3, dtype=torch_cuda.int64, device=off.device)
        v32 = [torch_cuda.full((4,), -7, dtype=torch_cuda.int32, device=off.device) for _ in range(3)]
        lib.check(L.utree_tiles_views(tree._h, off.data_ptr(), ln.data_ptr(), ln.numel(), W, S, tile_first.data_ptr(), f0, n, sentinel.data_ptr(),
                                      v32[0].data_ptr(), v32[1].data_ptr(), v32[2].data_ptr(), d_meta.data_ptr(), None), "utree_tiles_views")
        torch_cuda.cuda.synchronize()
        m = lib.TilesMeta.from_buffer_copy(d_meta.cpu().numpy().tobytes())
        assert (m.error, m.total_tiles, m.total_bases, m.max_len) == (1, total, 0, 0)
        assert bool((sentinel == -7).all()) and all(bool((v == -7).all()) for v in v32)


def test_plan_of_an_empty_batch(torch_cuda):
    db, tree = tree_for("vote")
    ln = torch_cuda.zeros(0, dtype=torch_cuda.int32, device="cuda:0")
    tile_first, meta = tree.tiles_plan(ln, 100, 50)
    assert meta["total_tiles"] == 0 and tile_first.cpu().numpy().tolist() == [0]


# ---- b. classify on the views against the oracle, and the views change nothing -----------------------------------------------------------
@pytest.mark.parametrize("name,rc", [(n, r) for n in tiles_ref.FIXTURES for r in (False, True)])
def test_classified_views_equal_the_oracle(torch_cuda, name, rc):
    db, tree = tree_for(name)
    if name == "vote":
        assert tree.info.bucket_bytes == 64 and tree.info.lane_pass == 1          # a bucketed image, the lane-per-read pass
    W, S = tiles_ref.PARAMS[name]
    recs, tl = ref(name, rc)
    bases, off, ln, fr = device_queries(torch_cuda, name)
    whole_before = tree.classify(bases, off, ln, rc=rc).clone()
    tile_first, meta = tree.tiles_plan(ln, W, S)
    assert meta["total_tiles"] == len(tl)
    toff, tlen, tq, ti, m = tree.tiles_views(off, ln, W, S, tile_first, 0, len(tl))
    assert m["error"] == 0 and m["total_bases"] == sum(x.b - x.a for x in tl) and m["max_len"] == max(x.b - x.a for x in tl)
    res = tree.classify(bases, toff, tlen, rc=rc, total_bases=m["total_bases"], max_len=m["max_len"])
    torch_cuda.cuda.synchronize()
    tree.poll()
    got, want = res.cpu().numpy().view(np.uint32), tiles_ref.results_array(tl)
    assert np.array_equal(tq.cpu().numpy(), [x.q for x in tl]) and np.array_equal(ti.cpu().numpy(), [x.t for x in tl])
    assert np.array_equal(got[:, 2], want["found"])
    hit = want["found"] > 0
    multi = hit & (want["uix"] > 1)
    assert np.array_equal(got[hit, 0], want["label"][hit]) and np.array_equal(got[hit, 3], want["uix"][hit])
    assert np.array_equal(got.view(np.int32)[hit, 1], want["cut"][hit])
    assert np.array_equal(got[multi, 4], want["sl"][multi]) and np.array_equal(got[multi, 5], want["ol"][multi])
    # ... and the lines of those results are the reference's
    from utree_amd.search import tiles_format
    text, lines = tiles_format(db, np.frombuffer(tiles_ref.contigs(name), dtype=np.uint8), fr["name_off"], fr["name_len"], fr["seq_len"], W, S,
                               tq.cpu().numpy(), ti.cpu().numpy(), res.cpu().numpy())
    assert text == tiles_ref.golden(name, rc) and lines == int(hit.sum())
    # the whole queries classify as before: the views wrote nothing
    whole_after = tree.classify(bases, off, ln, rc=rc)
    torch_cuda.cuda.synchronize()
    tree.poll()
    assert torch_cuda.equal(whole_before, whole_after)
    assert bytes(bases.cpu().numpy().tobytes()) == tiles_ref.contigs(name)


# ---- c. file to file ---------------------------------------------------------------------------------------------------------------------
STDOUT = re.compile(rb"^Queries: (\d+), tiles (\d+), classified (\d+), segments (\d+)$", re.M)


def cli(tmp_path, name, rc, data=None, env=None, segments=True, fname="contigs.fa"):
    W, S = tiles_ref.PARAMS[name]
    src = tmp_path / fname
    src.write_bytes(tiles_ref.contigs(name) if data is None else data)
    t, s = tmp_path / "tiles.tsv", tmp_path / "segments.tsv"
    for p in (t, s):
        if p.exists():
            p.unlink()
    e = dict(os.environ, UTREE_TILE_BP=str(W), UTREE_TILE_STEP=str(S))
    e.update(env or {})
    r = subprocess.run([lib.TILES_CLI_PATH, util.fixture_ctr(name), str(src), str(t)] + ([str(s)] if segments else []) + (["RC"] if rc else []),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    return r, t, s


def assert_files(r, t, s, name, rc):
    recs, tl = ref(name, rc)
    assert r.returncode == 0, r.stderr[-400:]
    assert t.read_bytes() == tiles_ref.golden(name, rc)
    want = tiles_ref.segments_tsv(recs, tl)
    assert s.read_bytes() == want
    m = tiles_ref.manifest()["fixtures"][name]
    tag = "_rc" if rc else ""
    # the counts on stdout are the reference's own for the pre-split file: "Searched N queries", "Good finds: N"
    assert [int(x) for x in STDOUT.search(r.stdout).groups()] == [m["queries"], m["searched" + tag], m["good_finds" + tag], want.count(b"\n")]


@pytest.mark.parametrize("name,rc", [(n, r) for n in tiles_ref.FIXTURES for r in (False, True)])
def test_cli_writes_the_golden_bytes(torch_cuda, tmp_path, name, rc):
    assert_files(*cli(tmp_path, name, rc), name, rc)


@pytest.mark.parametrize("env", [dict(UTREE_TILES_BATCH="7"), dict(UTREE_CHUNK_BYTES="4000"), dict(UTREE_TILES_BATCH="1", UTREE_CHUNK_BYTES="3100")])
def test_cli_with_small_batches_and_chunks(torch_cuda, tmp_path, env):
    """queries whose tiles straddle sub-batches (the open run is carried), and several chunks (it is not)"""
    for name, rc in (("vote", True), ("ix32", False)):
        assert_files(*cli(tmp_path, name, rc, env=env), name, rc)


def test_cli_reads_fastq_multiline_and_gzip(torch_cuda, tmp_path):
    name, rc = "vote", False
    recs = tiles_ref.parse(tiles_ref.contigs(name))
    fq = b"".join(b"@%s some text\n%s\n+\n%s\n" % (n, s, b"I" * len(s)) for n, s in recs)
    ml = pairs_ref.wrap(tiles_ref.contigs(name), 60)
    assert_files(*cli(tmp_path, name, rc, data=fq, env=dict(UTREE_INPUT="fastq"), fname="contigs.fq"), name, rc)
    assert_files(*cli(tmp_path, name, rc, data=pairs_ref.gz(fq), env=dict(UTREE_INPUT="auto"), fname="contigs.fq.gz"), name, rc)
    assert_files(*cli(tmp_path, name, rc, data=ml, env=dict(UTREE_INPUT="fasta"), fname="contigs.ml.fa"), name, rc)
    assert_files(*cli(tmp_path, name, rc, data=pairs_ref.gz(ml), env=dict(UTREE_INPUT="auto", UTREE_CHUNK_BYTES="4000"), fname="contigs.ml.fa.gz"), name, rc)


def test_cli_without_segments_and_through_the_binding(torch_cuda, tmp_path):
    name, rc = "k64", True
    r, t, s = cli(tmp_path, name, rc, segments=False)
    m = tiles_ref.manifest()["fixtures"][name]
    assert r.returncode == 0 and t.read_bytes() == tiles_ref.golden(name, rc) and not s.exists()
    assert [int(x) for x in STDOUT.search(r.stdout).groups()] == [m["queries"], m["tiles"], m["good_finds_rc"], 0]
    db, tree = tree_for(name)
    W, S = tiles_ref.PARAMS[name]
    code, st = tiles_file(db, tree, str(tmp_path / "contigs.fa"), str(tmp_path / "t2.tsv"), str(tmp_path / "s2.tsv"), tile_bp=W, step_bp=S, rc=rc)
    recs, tl = ref(name, rc)
    assert code == lib.OK and (tmp_path / "t2.tsv").read_bytes() == tiles_ref.golden(name, rc)
    assert (tmp_path / "s2.tsv").read_bytes() == tiles_ref.segments_tsv(recs, tl)
    assert (st.n_queries, st.n_tiles, st.classified, st.segments) == (m["queries"], m["tiles"], m["good_finds_rc"], m["segments_rc"])


def test_cli_framing_error_in_the_third_record(torch_cuda, tmp_path):
    name, rc = "vote", False
    recs, tl = ref(name, rc)
    lines = tiles_ref.contigs(name).split(b"\n")
    bad = b"\n".join(lines[:4] + [b"no_header_here"] + lines[5:])                  # the third record's '>' line
    r, t, s = cli(tmp_path, name, rc, data=bad)
    assert r.returncode == 2 and b"ERROR: no header '>' [L 3]" in r.stderr
    two = [x for x in tl if x.q < 2]
    assert t.read_bytes() == tiles_ref.tiles_tsv(two) and s.read_bytes() == tiles_ref.segments_tsv(recs, two)
    assert [int(x) for x in STDOUT.search(r.stdout).groups()][:2] == [2, len(two)]


def test_cli_unwritable_tiles_and_malformed_variables(torch_cuda, tmp_path):
    name = "vote"
    src = tmp_path / "contigs.fa"
    src.write_bytes(tiles_ref.contigs(name))
    seg = tmp_path / "segments.tsv"
    e = dict(os.environ, UTREE_TILE_BP="150", UTREE_TILE_STEP="75")
    r = subprocess.run([lib.TILES_CLI_PATH, util.fixture_ctr(name), str(src), str(tmp_path / "no_such_dir" / "tiles.tsv"), str(seg)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    assert r.returncode == 1 and not seg.exists()
    r = subprocess.run([lib.TILES_CLI_PATH, util.fixture_ctr(name), str(tmp_path / "no_such.fa"), str(tmp_path / "tiles.tsv"), str(seg)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    assert r.returncode == 1 and not seg.exists() and not (tmp_path / "tiles.tsv").exists()
    for var, val in (("UTREE_TILE_BP", "0"), ("UTREE_TILE_BP", "16777215"), ("UTREE_TILE_BP", "1e3"), ("UTREE_TILE_STEP", "151"), ("UTREE_TILE_STEP", ""),
                     ("UTREE_TILES_BATCH", "0"), ("UTREE_TILES_BATCH", "x"), ("UTREE_INPUT", "bam")):
        r = subprocess.run([lib.TILES_CLI_PATH, util.fixture_ctr(name), str(src), str(tmp_path / "tiles.tsv")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=dict(e, **{var: val}), timeout=120)
        assert r.returncode == 2 and var.encode() in r.stderr and not (tmp_path / "tiles.tsv").exists(), (var, val)
