"""GPU tests of the per-query k-mer hit map (csrc/hitmap_kernels.hip, csrc/hitmap.c, UTREE_HITMAP): run offsets, runs and meta of a batch and
every file must equal tests/hitmap_ref.py -- the contract restated with the CPU oracle, pinned to the genuine reference's outputs in
tests/test_hitmap_cpu.py --, and the per-read results must stay what they were.  All comparisons are exact: there is no tolerance in this
feature.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hitmap_ref
import pairs_ref
import util
from oracle import orc
from profile_ref import fasta_names, profile_ref
from test_coverage_cpu import fixture_seqs
from test_hitmap_cpu import FIXTURES, reference_maps
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree

N_READS = 2000


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_TREES = {}


def tree_for(name):
    if name not in _TREES:
        while len(_TREES) >= 4:
            _TREES.pop(next(iter(_TREES)))[1].close()
        db = CtrDB.open(util.fixture_ctr(name))
        _TREES[name] = (db, DeviceTree.upload(db, 0))
    return _TREES[name]


def device_reads(torch, seqs):
    """(bases, off, len) CUDA tensors of reads laid out one after the other"""
    ln = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln.astype(np.int64))[:-1]]).astype(np.int64)
    buf = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()


def assert_map(got, maps):
    """(run_off, runs, meta) of DeviceTree.hitmap against the reference's maps, everything"""
    run_off, runs, meta = got
    off, want = hitmap_ref.flat(maps)
    windows = int(want[:, 1].astype(np.int64).sum()) if len(want) else 0
    assert meta == dict(total_runs=len(want), total_windows=windows, error=0)
    assert np.array_equal(run_off.cpu().numpy(), off)
    assert np.array_equal(runs.cpu().numpy().view(np.uint32)[:len(want)], want)


# ---- a. every fixture, every image kind ------------------------------------------------------------------------------------------------
def check_fixture(torch, tree, name, rc):
    seqs = fixture_seqs(name)[:N_READS]
    t = device_reads(torch, seqs)
    before = tree.classify(*t, rc=bool(rc)).clone()
    torch.cuda.synchronize()
    got = tree.hitmap(*t, rc=bool(rc))
    assert_map(got, reference_maps(name, rc, N_READS))
    after = tree.classify(*t, rc=bool(rc))
    torch.cuda.synchronize()
    tree.poll()
    assert torch.equal(before, after)
    # ... and the map agrees with the vote's own two figures, read by read
    res, off, runs = after.cpu().numpy(), got[0].cpu().numpy(), got[1].cpu().numpy().view(np.uint32)
    for i in range(0, len(seqs), 7):
        m = [(int(c), int(n)) for c, n in runs[off[i]:off[i + 1]]]
        found, uix = hitmap_ref.found_uix(m)
        assert found == res[i][2] and (uix == res[i][3] or not found)


@pytest.mark.parametrize("name,rc", [(n, r) for n in FIXTURES for r in (0, 1)])
def test_maps_equal_the_reference(torch_cuda, name, rc):
    db, tree = tree_for(name)
    info = tree.info
    if name in ("toy", "vote", "ix32"):
        assert info.lane_pass == 1                                  # the lane-per-read pass's images
    if name == "k64ix32":
        assert info.lane_pass == 0                                  # the wave-per-read kernels'
    if name == "k16":
        assert info.bucket_bytes == 0                               # the direct table
    else:
        assert info.bucket_bytes == 64
    check_fixture(torch_cuda, tree, name, rc)


def test_line_sized_buckets(torch_cuda, monkeypatch):
    monkeypatch.setenv("UTREE_BUCKET_BYTES", "128")
    db = CtrDB.open(util.fixture_ctr("toy"))
    tree = DeviceTree.upload(db, 0)
    try:
        assert tree.info.bucket_bytes == 128
        check_fixture(torch_cuda, tree, "toy", 1)
    finally:
        tree.close()


# ---- b. edges ------------------------------------------------------------------------------------------------------------------------------
_EDGE = {}


def edge_reads(name):
    """one batch of edge reads built from the fixture's reads, so that hits exist"""
    if name not in _EDGE:
        seqs = fixture_seqs(name)
        o = orc.OracleDB.load(util.fixture_ctr(name))
        k = o.k
        base = b"".join(s for s in seqs[:60] if len(s) >= k)                     # no separator: windows across the seams, mostly misses
        assert len(base) > k + 70
        data = util.fixture_bytes(name + "_reads.fa.gz")
        _, off, ln = util.parse_fasta(data)
        res = o.classify_batch(np.frombuffer(data, dtype=np.uint8), off[:800], ln[:800], rc=False, threads=0)
        one = [i for i in range(800) if res["found"][i] > 2 and res["uix"][i] == 1][0]
        mid = seqs[one]
        out = [b"", base[:k - 1], base[:k], base[:k + 1],
               base[5:5 + k // 2], base[5:5 + k // 2 - 1],                      # with RC: 2L+1 = k+1 >= k > L, and 2L+1 = k-1 < k
               b"N" * 50, mid[:len(mid) // 2] + b"N" + mid[len(mid) // 2:], mid.lower(), seqs[one + 1].lower()]
        out += [base[:k - 1 + w] for w in (31, 32, 33, 63, 64, 65)]
        out.append(mid * 20)                                                      # one label's hits over several 32-window items
        rng = np.random.default_rng(5)
        out.append(bytes(b"ACGT"[c] for c in rng.integers(0, 4, 700)))            # runs much longer than a wavefront's 64 windows: misses ...
        out.append(b"N" * 300 + mid + b"N" * 333)                                 # ... and invalid windows
        _EDGE[name + ".mid"] = mid
        short = [s for s in seqs[:40]]
        long1, long2 = b"N".join(seqs[100:400]), b"N".join((seqs * 2)[400:3400])
        assert len(long2) - k + 1 > 2 * 8192                                      # more windows than one workgroup's items hold
        _EDGE[name] = short[:13] + [long1] + short[13:27] + out + [long2] + short[27:] + [b"", base[:k]]
    return _EDGE[name]


def edge_maps(name, rc):
    if (name, rc) not in _EDGE:
        _EDGE[(name, rc)] = hitmap_ref.hitmap(util.fixture_ctr(name), edge_reads(name), rc)
    return _EDGE[(name, rc)]


@pytest.mark.parametrize("name,rc", [(n, r) for n in ("toy", "k64") for r in (0, 1)])
def test_edge_reads(torch_cuda, name, rc):
    torch = torch_cuda
    db, tree = tree_for(name)
    seqs, maps = edge_reads(name), edge_maps(name, rc)
    k = 4 * db.W
    by_len = {len(s): m for s, m in zip(seqs, maps)}
    assert by_len[0] == [] and by_len[k - 1] == ([(hitmap_ref.INVALID, k)] if rc else [])      # (the reference itself, on the edges)
    assert by_len[k // 2] == ([(hitmap_ref.INVALID, 2)] if rc else []) and by_len[k // 2 - 1] == []
    rep = maps[seqs.index(_EDGE[name + ".mid"] * 20)]                              # ONE label, its hits in many different 32-window items
    at, items = 0, set()
    for c, n in rep:
        if c < hitmap_ref.INVALID:
            items.update(range(at // 32, (at + n - 1) // 32 + 1))
        at += n
    assert hitmap_ref.found_uix(rep)[1] == 1 and len(items) >= 10
    assert max(n for m in maps for c, n in m if c == hitmap_ref.MISS) > 192 and sum(1 for m in maps for c, n in m if c == hitmap_ref.INVALID and n > 192) >= 2
    assert_map(tree.hitmap(*device_reads(torch, seqs), rc=bool(rc)), maps)


# ---- c. capacity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short_by", ["one", "all"])
def test_capacity_too_small_is_reported_and_nothing_is_written_beyond_it(torch_cuda, short_by):
    torch = torch_cuda
    db, tree = tree_for("toy")
    seqs, maps = edge_reads("toy"), edge_maps("toy", 1)
    off, want = hitmap_ref.flat(maps)
    cap = len(want) - 1 if short_by == "one" else 0
    guard = 4096
    runs = torch.full((len(want) + guard, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    run_off, _, meta = tree.hitmap(*device_reads(torch, seqs), rc=True, capacity=cap, runs=runs)
    assert meta == dict(total_runs=len(want), total_windows=int(want[:, 1].astype(np.int64).sum()), error=1)
    assert np.array_equal(run_off.cpu().numpy(), off)
    got = runs.cpu().numpy().view(np.uint32)
    assert (got[cap:] == 0x5A5A5A5A).all()                                        # a checked condition: the kernel never writes there
    assert np.array_equal(got[:cap], want[:cap])


# ---- d. pairs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [0, 1])
def test_pairs_are_mapped_as_their_joined_queries(torch_cuda, rc):
    torch = torch_cuda
    db, tree = tree_for("toy")
    P = pairs_ref.Pairs("toy")
    n = 500
    b1, o1, l1 = device_reads(torch, P.seq1[:n])
    b2, o2, l2 = device_reads(torch, P.seq2[:n])
    joined, joff, jlen, meta = tree.join_pairs(b1, o1, l1, b2, o2, l2)
    assert meta["error"] == 0
    assert_map(tree.hitmap(joined, joff, jlen, rc=bool(rc)), hitmap_ref.hitmap(util.fixture_ctr("toy"), P.joined_seqs()[:n], rc))


# ---- f. two streams ------------------------------------------------------------------------------------------------------------------------
def test_two_streams_on_one_tree(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    batches = [fixture_seqs("toy")[:N_READS], edge_reads("toy")]
    want = [reference_maps("toy", 1, N_READS), edge_maps("toy", 1)]
    ts = [device_reads(torch, b) for b in batches]
    totals = [int(t[2].sum().item()) for t in ts]
    ws = [torch.empty(lib.load().utree_hitmap_workspace_bytes(tree._h, len(b), tb, 1), dtype=torch.uint8, device="cuda") for b, tb in zip(batches, totals)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = []
    for rep in range(2):                                                          # (the second round: the same workspaces again)
        got = []
        for s, t, w, tb in zip(streams, ts, ws, totals):
            with torch.cuda.stream(s):
                got.append(tree.hitmap(*t, rc=True, total_bases=tb, workspace=w, sync=False))
        torch.cuda.synchronize()
    for (run_off, runs, d_meta), maps in zip(got, want):
        m = d_meta.cpu().numpy()
        assert_map((run_off, runs, dict(total_runs=int(m[0]), total_windows=int(m[1]), error=int(m[2] & 0xFFFFFFFF))), maps)


# ---- e. the whole-file search and the command line ---------------------------------------------------------------------------------------
VARS = ("UTREE_HITMAP", "UTREE_REDISTRIBUTE", "UTREE_PROFILE", "UTREE_COVERAGE", "UTREE_MATES", "UTREE_INTERLEAVED", "UTREE_INPUT", "UTREE_CHUNK_BYTES",
        "UTREE_HOST_TEXT")


def run_cli(cli, ctr, fa, out, rc, **env):
    base = dict(os.environ, UTREE_GPUS="1")
    for v in VARS:
        base.pop(v, None)
    return subprocess.run([cli, ctr, str(fa), str(out), "4"] + (["RC"] if rc else []), capture_output=True, env=dict(base, **env), timeout=300)


def toy_file(tmp_path):
    data = util.fixture_bytes("toy_reads.fa.gz")
    head = b"\n".join(data.split(b"\n")[:2 * N_READS]) + b"\n"                    # the first N_READS records
    fa = tmp_path / "reads.fa"
    fa.write_bytes(head)
    return fa, head


def test_cli_writes_the_reference_files(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    fa, data = toy_file(tmp_path)
    names = fasta_names(data)
    want = hitmap_ref.file_bytes(names, reference_maps("toy", 1, N_READS))
    plain = run_cli(cli, ctr, fa, tmp_path / "a.txt", 1)
    assert plain.returncode == 0
    hm = tmp_path / "map.tsv"
    r = run_cli(cli, ctr, fa, tmp_path / "b.txt", 1, UTREE_HITMAP=str(hm))
    assert r.returncode == 0 and r.stdout == plain.stdout
    assert hm.read_bytes() == want and (tmp_path / "map.tsv.labels").read_bytes() == hitmap_ref.labels_bytes(ctr)
    out = (tmp_path / "b.txt").read_bytes()
    assert out == (tmp_path / "a.txt").read_bytes()
    golden = util.fixture_bytes("toy_out_rc.txt.gz")
    assert golden.startswith(out) and out.count(b"\n") == sum(1 for l in golden.split(b"\n")[:-1] if int(l.split(b"\t")[0][1:]) < N_READS)
    # several chunks, and a report next to it: the same map, the reference's profile
    prof = tmp_path / "p.tsv"
    r = run_cli(cli, ctr, fa, tmp_path / "c.txt", 1, UTREE_HITMAP=str(hm), UTREE_PROFILE=str(prof), UTREE_CHUNK_BYTES="30000")
    assert r.returncode == 0 and r.stdout == plain.stdout and hm.read_bytes() == want and (tmp_path / "c.txt").read_bytes() == out
    assert prof.read_bytes() == profile_ref(out, names, N_READS)
    # a path that cannot be opened: before the search; a map that cannot be written: the search's output, exit 1, the cause by name
    bad = run_cli(cli, ctr, fa, tmp_path / "d.txt", 1, UTREE_HITMAP=str(tmp_path / "no" / "dir" / "m.tsv"))
    assert bad.returncode == 1 and b"hit map" in bad.stderr and not (tmp_path / "d.txt").exists()


def test_search_gg_two_handles_and_a_map_that_cannot_be_written(torch_cuda, tmp_path):
    from utree_amd.search import search_gg
    db, tree = tree_for("toy")
    fa, data = toy_file(tmp_path)
    want = hitmap_ref.file_bytes(fasta_names(data), reference_maps("toy", 0, N_READS))
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "a.txt"), rc=False, threads=4)
    assert code == lib.OK
    tree2 = DeviceTree.upload(db, 0)
    try:                                                                          # two handles on one card: each maps its share of a slot
        code, st = search_gg(db, [tree, tree2], str(fa), str(tmp_path / "b.txt"), rc=False, threads=4, hitmap=str(tmp_path / "m.tsv"))
    finally:
        tree2.close()
    assert code == lib.OK and st.n_reads == N_READS and st.pipeline == 0
    assert (tmp_path / "m.tsv").read_bytes() == want and (tmp_path / "b.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "c.txt"), rc=False, threads=4, hitmap="/dev/full")
    assert code == lib.E_HITMAP and b"hit map /dev/full" in lib.load().utree_last_hip_error()
    assert (tmp_path / "c.txt").read_bytes() == (tmp_path / "a.txt").read_bytes() and st.n_reads == N_READS


def test_cli_mates(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    P = pairs_ref.Pairs("toy")
    n = 1000
    rp, mp = tmp_path / "r1.fa", tmp_path / "r2.fa"
    rp.write_bytes(P.reads_fasta(n)); mp.write_bytes(P.mates_fasta(n))
    hm = tmp_path / "m.tsv"
    plain = run_cli(cli, ctr, rp, tmp_path / "a.txt", 1, UTREE_MATES=str(mp))
    r = run_cli(cli, ctr, rp, tmp_path / "b.txt", 1, UTREE_MATES=str(mp), UTREE_HITMAP=str(hm), UTREE_CHUNK_BYTES="40000")
    assert r.returncode == plain.returncode == 0 and r.stdout == plain.stdout
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()
    assert hm.read_bytes() == hitmap_ref.file_bytes(P.names1[:n], hitmap_ref.hitmap(ctr, P.joined_seqs()[:n], True))


def test_cli_malformed_third_record(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    seqs = fixture_seqs("toy")
    fa = tmp_path / "bad.fa"
    fa.write_bytes(b">a\n%s\n>b\n%s\nno header here\n%s\n>d\n%s\n" % (seqs[0], seqs[1], seqs[2], seqs[3]))
    plain = run_cli(cli, ctr, fa, tmp_path / "a.txt", 1)
    hm = tmp_path / "m.tsv"
    r = run_cli(cli, ctr, fa, tmp_path / "b.txt", 1, UTREE_HITMAP=str(hm))
    assert r.returncode == plain.returncode == 2 and r.stdout == plain.stdout
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()
    assert hm.read_bytes() == hitmap_ref.file_bytes([b"a", b"b"], hitmap_ref.hitmap(ctr, seqs[:2], True))   # exactly the queries written


def test_rank_specific_cli_ignores_the_variable(torch_cuda, tmp_path):
    ctr, fa = util.fixture_ctr("toy"), util.fixture_reads_path("toy")
    plain = run_cli(lib.RANK_CLI_PATH, ctr, fa, tmp_path / "a.txt", 0)
    withm = run_cli(lib.RANK_CLI_PATH, ctr, fa, tmp_path / "b.txt", 0, UTREE_HITMAP=str(tmp_path / "m.tsv"))
    assert plain.returncode == withm.returncode == 0 and plain.stdout == withm.stdout
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes() and not (tmp_path / "m.tsv").exists()
    assert withm.stderr.count(b"UTREE_HITMAP is ignored") == 1
