"""GPU tests of the redistribution of ambiguous reads (csrc/redist_kernels.hip, csrc/redist.c, UTREE_REDISTRIBUTE): the candidate sets read
back from the device, the passes and every file must equal tests/redist_ref.py -- the contract restated with the CPU oracle, pinned in
tests/test_redist_cpu.py --, and the per-read results must stay what they were.  All comparisons are exact: there is no tolerance in this
feature.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import coverage_ref
import pairs_ref
import redist_ref
from oracle import orc
from profile_ref import fasta_names, profile_ref
from test_coverage_cpu import fixture_seqs
from test_redist_cpu import PINNED, reference_sets
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, search_gg
import util

N_READS = 4000


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


def want_multiset(sets):
    return dict(redist_ref.multiset(sets))


def entries_dict(e, field):
    return {int(l): int(v) for l, v in zip(e["label"], e[field]) if v}


# ---- d. the candidate sets, every classify path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rc", [(n, r) for n in ("toy", "vote", "ix32", "k64", "k64ix32", "k16") for r in (0, 1)])
def test_sets_equal_the_reference(torch_cuda, name, rc):
    torch = torch_cuda
    db, tree = tree_for(name)
    info = tree.info
    if name in ("toy", "vote", "ix32"):
        assert info.lane_pass == 1                                  # the lane-per-read pass
    if name == "k64ix32":
        assert info.lane_pass == 0                                  # the wave-per-read kernels
    if name == "k16":
        assert info.bucket_bytes == 0                               # the direct table
    seqs = fixture_seqs(name)[:N_READS]
    sets, _ = reference_sets(name, rc, N_READS)
    t = device_reads(torch, seqs)
    plain = tree.classify(*t, rc=bool(rc))
    torch.cuda.synchronize()
    rd = tree.redistribution(1 << 14)
    try:
        got = rd.classify(*t, rc=bool(rc))
        torch.cuda.synchronize()
        tree.poll()
        assert torch.equal(got, plain)                              # bit for bit utree_classify_batch's
        ms, n_reads, n_classified = rd.sets()
        want = want_multiset(sets)
        assert n_reads == len(seqs) and n_classified == sum(want.values())
        assert ms == want
        if (name, rc, len(seqs)) in PINNED:
            assert n_classified == PINNED[(name, rc, len(seqs))][0] and sum(1 for s in ms if len(s) > 1) == PINNED[(name, rc, len(seqs))][2]
        rd.reset()
        assert rd.sets() == ({}, 0, 0)
    finally:
        rd.close()


# ---- e. one batch of mixed lengths: the mid, pieces and long-read paths -----------------------------------------------------------------
_MIXED = {}


def mixed_reads():
    """plain toy reads with reads of about 700, about 3000 and more than 2 x 2112 bases among them (runs of toy reads joined with 'N'); some
    long ones repeat ONE read whose hits name a single label: the long-read kernel finishes those records itself"""
    if not _MIXED:
        seqs = fixture_seqs("toy")
        o = orc.OracleDB.load(util.fixture_ctr("toy"))
        data = util.fixture_bytes("toy_reads.fa.gz")
        _, off, ln = util.parse_fasta(data)
        want = o.classify_batch(np.frombuffer(data, dtype=np.uint8), off[:600], ln[:600], rc=False, threads=0)
        one = [i for i in range(600) if want["found"][i] > 2 and want["uix"][i] == 1][:3]
        assert len(one) == 3
        rng = np.random.default_rng(23)
        out = list(seqs[:300])
        for k, run in enumerate((7, 30, 45, 90, 7, 30, 60)):
            a = 300 + 100 * k
            out.insert(int(rng.integers(0, len(out))), b"N".join(seqs[a:a + run]))
        for i in one:
            out.insert(int(rng.integers(0, len(out))), b"N".join([seqs[i]] * 50))
        out.insert(5, b"N".join([b"ACGT" * 30] * 40))                                  # long, and (most likely) no hit at all
        _MIXED["seqs"] = out
        assert sorted(len(s) for s in out)[-1] > 2 * 2112 * 2 and sum(600 < len(s) < 800 for s in out) >= 2
    return _MIXED["seqs"]


def mixed_reference(rc):
    if rc not in _MIXED:
        _MIXED[rc] = redist_ref.candidate_sets(util.fixture_ctr("toy"), mixed_reads(), rc)[0]
    return _MIXED[rc]


@pytest.mark.parametrize("rc,lane_pass", [(0, "1"), (1, "1"), (0, "0"), (1, "0")])
def test_mixed_length_batch(torch_cuda, rc, lane_pass, monkeypatch):
    """lane_pass "0": the wave-per-read kernels take the batch (mid pass, classify_long_k for every long read)"""
    torch = torch_cuda
    monkeypatch.setenv("UTREE_LANE_PASS", lane_pass)
    db, tree = tree_for("toy")
    seqs = mixed_reads()
    t = device_reads(torch, seqs)
    plain = tree.classify(*t, rc=bool(rc))
    torch.cuda.synchronize()
    rd = tree.redistribution(1 << 12)
    try:
        got = rd.classify(*t, rc=bool(rc))
        torch.cuda.synchronize()
        tree.poll()
        assert torch.equal(got, plain)
        ms, n_reads, n_classified = rd.sets()
        want = want_multiset(mixed_reference(rc))
        assert n_reads == len(seqs) and ms == want and n_classified == sum(want.values())
        res = got.cpu().numpy()
        long_single = sum(1 for s, r in zip(seqs, res) if len(s) > 2 * 2112 and r[2] > 0 and r[3] == 1)
        assert long_single >= 3                                      # finished single-label records of long reads were among them
    finally:
        rd.close()


# ---- f. solve, merge, streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "vote"])
def test_solve_equals_the_reference(torch_cuda, name):
    torch = torch_cuda
    db, tree = tree_for(name)
    seqs = fixture_seqs(name)[:N_READS]
    sets, _ = reference_sets(name, 0, N_READS)
    rd = tree.redistribution(1 << 14)
    try:
        rd.classify(*device_reads(torch, seqs), rc=False)
        for mp in (1, 3, 100):
            a, u, p, amb, _ = redist_ref.solve(sets, len(seqs), mp)
            e, passes, ambiguous = rd.solve(mp)
            assert (passes, ambiguous) == (p, amb)
            assert entries_dict(e, "assigned") == dict(a) and entries_dict(e, "unique") == dict(u)
        assert rd.solve(100)[1] == PINNED[(name, 0, N_READS)][4]
        with pytest.raises(lib.UtreeError):
            rd.solve(0)
    finally:
        rd.close()


def test_merge_of_two_handles_equals_one(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    seqs = fixture_seqs("toy")[:N_READS]
    sets, _ = reference_sets("toy", 0, N_READS)
    a, b = tree.redistribution(1 << 12), tree.redistribution(1 << 13)
    try:
        a.classify(*device_reads(torch, seqs[:1700]), rc=False)
        b.classify(*device_reads(torch, seqs[1700:]), rc=False)
        a.merge(b)
        ms, n_reads, n_classified = a.sets()
        assert n_reads == N_READS and ms == want_multiset(sets)
        want_a, want_u, p, amb, _ = redist_ref.solve(sets, N_READS)
        e, passes, ambiguous = a.solve()
        assert (passes, ambiguous) == (p, amb) and entries_dict(e, "assigned") == dict(want_a) and entries_dict(e, "unique") == dict(want_u)
        assert b.sets()[1] == N_READS - 1700                         # the source keeps its own
    finally:
        a.close(); b.close()


def test_four_streams_add_at_once(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    seqs = fixture_seqs("toy")[:N_READS]
    sets, _ = reference_sets("toy", 0, N_READS)
    t = device_reads(torch, seqs)
    total, mx = int(t[2].sum().item()), int(t[2].max().item())
    need = tree.workspace_bytes(len(seqs), total, mx, False)
    streams = [torch.cuda.Stream() for _ in range(4)]
    ws = [torch.empty(need, dtype=torch.uint8, device="cuda") for _ in range(4)]
    outs = [torch.empty((len(seqs), 6), dtype=torch.int32, device="cuda") for _ in range(4)]
    rd = tree.redistribution(1 << 12)
    try:
        torch.cuda.synchronize()
        for s, w, o in zip(streams, ws, outs):
            with torch.cuda.stream(s):
                rd.classify(*t, rc=False, total_bases=total, max_len=mx, out=o, workspace=w)
        torch.cuda.synchronize()
        tree.poll()
        ms, n_reads, _ = rd.sets()
        assert n_reads == 4 * N_READS and ms == {s: 4 * n for s, n in want_multiset(sets).items()}
        assert all(torch.equal(o, outs[0]) for o in outs[1:])
    finally:
        rd.close()


# ---- g. capacity ----------------------------------------------------------------------------------------------------------------------
def test_a_table_too_small_is_an_error_not_a_wrong_table(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    seqs = fixture_seqs("toy")[:N_READS]
    t = device_reads(torch, seqs)
    plain = tree.classify(*t, rc=False)
    rd = tree.redistribution(16)
    try:
        got = rd.classify(*t, rc=False)
        torch.cuda.synchronize()
        tree.poll()
        assert torch.equal(got, plain)                               # the per-read results do not depend on it
        with pytest.raises(lib.UtreeError) as e:
            rd.sets()
        assert e.value.code == lib.E_DEVICE and "UTREE_REDIST_CAPACITY" in str(e.value)
        with pytest.raises(lib.UtreeError) as e:
            rd.solve()
        assert e.value.code == lib.E_DEVICE
        rd.reset()
        rd.classify(*device_reads(torch, seqs[:3]), rc=False)
        assert rd.sets()[1] == 3                                      # usable again after a reset
    finally:
        rd.close()


# ---- h. the whole-file search and the command line ------------------------------------------------------------------------------------
def toy_file(tmp_path):
    data = util.fixture_bytes("toy_reads.fa.gz")
    head = b"\n".join(data.split(b"\n")[:2 * N_READS]) + b"\n"                       # the first N_READS records
    fa = tmp_path / "reads.fa"
    fa.write_bytes(head)
    return fa, head


def toy_reference(rc, max_passes=100):
    sets, texts = reference_sets("toy", rc, N_READS)
    a, u, p, amb, _ = redist_ref.solve(sets, N_READS, max_passes)
    return redist_ref.redist_file(a, u, texts, N_READS, amb, p)


def run_cli(cli, ctr, fa, out, rc, **env):
    base = dict(os.environ, UTREE_GPUS="1")
    for v in ("UTREE_REDISTRIBUTE", "UTREE_REDIST_PASSES", "UTREE_REDIST_CAPACITY", "UTREE_PROFILE", "UTREE_COVERAGE", "UTREE_MATES", "UTREE_INTERLEAVED"):
        base.pop(v, None)
    return subprocess.run([cli, ctr, str(fa), str(out), "4"] + (["RC"] if rc else []), capture_output=True, env=dict(base, **env), timeout=300)


@pytest.mark.parametrize("pipeline", ["device", "host"])
def test_search_gg_writes_the_reference_file(torch_cuda, pipeline, tmp_path, monkeypatch):
    if pipeline == "host":
        monkeypatch.setenv("UTREE_HOST_TEXT", "1")
    db, tree = tree_for("toy")
    fa, data = toy_file(tmp_path)
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "a.txt"), rc=True, threads=4)
    assert code == lib.OK
    red = tmp_path / "r.tsv"
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "b.txt"), rc=True, threads=4, redistribute=str(red))
    assert code == lib.OK and st.n_reads == N_READS and st.pipeline == (1 if pipeline == "device" else 0)
    assert (tmp_path / "b.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    assert red.read_bytes() == toy_reference(1)
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "c.txt"), rc=True, threads=4, redistribute=str(red), redist_passes=1)
    assert code == lib.OK and red.read_bytes() == toy_reference(1, 1) != toy_reference(1)
    # two device handles on one card: their sets are merged before the passes
    tree2 = DeviceTree.upload(db, 0)
    try:
        code, st = search_gg(db, [tree, tree2], str(fa), str(tmp_path / "d.txt"), rc=True, threads=4, redistribute=str(red))
        assert code == lib.OK and red.read_bytes() == toy_reference(1) and (tmp_path / "d.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    finally:
        tree2.close()
    # a file that cannot be written: the search's output, UTREE_E_PROFILE, the cause by name
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "e.txt"), rc=True, threads=4, redistribute="/dev/full")
    assert code == lib.E_PROFILE and b"redistribution /dev/full" in lib.load().utree_last_hip_error()
    assert (tmp_path / "e.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()


def test_cli_file_and_unchanged_output(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    fa, data = toy_file(tmp_path)
    plain = run_cli(cli, ctr, fa, tmp_path / "a.txt", 1)
    assert plain.returncode == 0 and not list(tmp_path.glob("*.tsv"))                  # without the variable: no file
    red = tmp_path / "r.tsv"
    withr = run_cli(cli, ctr, fa, tmp_path / "b.txt", 1, UTREE_REDISTRIBUTE=str(red))
    assert withr.returncode == 0 and withr.stdout == plain.stdout
    assert (tmp_path / "b.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    assert red.read_bytes() == toy_reference(1)
    one = run_cli(cli, ctr, fa, tmp_path / "c.txt", 1, UTREE_REDISTRIBUTE=str(red), UTREE_REDIST_PASSES="1")
    assert one.returncode == 0 and one.stdout == plain.stdout and red.read_bytes() == toy_reference(1, 1)


def test_cli_with_profile_and_coverage(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    fa, data = toy_file(tmp_path)
    red, prof, cov = tmp_path / "r.tsv", tmp_path / "p.tsv", tmp_path / "c.tsv"
    r = run_cli(cli, ctr, fa, tmp_path / "a.txt", 1, UTREE_REDISTRIBUTE=str(red), UTREE_PROFILE=str(prof), UTREE_COVERAGE=str(cov))
    assert r.returncode == 0
    out = (tmp_path / "a.txt").read_bytes()
    assert red.read_bytes() == toy_reference(1)
    assert prof.read_bytes() == profile_ref(out, fasta_names(data), N_READS)
    seqs = fixture_seqs("toy")[:N_READS]
    dbk, covd, hits, texts = coverage_ref.coverage_counts(ctr, seqs, True)
    assert cov.read_bytes() == coverage_ref.coverage_file(dbk, covd, hits, texts, N_READS)
    # the profile's classified and the redistribution's are one figure
    assert prof.read_bytes().split(b"\n")[0].split(b"\t")[:6] == red.read_bytes().split(b"\n")[0].split(b"\t")[:6]


def test_cli_mates_candidates_are_those_of_the_joined_queries(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    P = pairs_ref.Pairs("toy")
    n = 1500
    rp, mp = tmp_path / "r1.fa", tmp_path / "r2.fa"
    rp.write_bytes(P.reads_fasta(n)); mp.write_bytes(P.mates_fasta(n))
    red = tmp_path / "r.tsv"
    r = run_cli(cli, ctr, rp, tmp_path / "a.txt", 1, UTREE_REDISTRIBUTE=str(red), UTREE_MATES=str(mp))
    assert r.returncode == 0
    assert red.read_bytes() == redist_ref.reference_file(ctr, P.joined_seqs()[:n], True)
    plain = run_cli(cli, ctr, rp, tmp_path / "b.txt", 1, UTREE_MATES=str(mp))
    assert plain.stdout == r.stdout and (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()


def test_cli_unwritable_paths_and_bad_passes(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    fa, data = toy_file(tmp_path)
    bad = run_cli(cli, ctr, fa, tmp_path / "c.txt", 1, UTREE_REDISTRIBUTE=str(tmp_path / "no" / "dir" / "r.tsv"))
    assert bad.returncode == 1 and b"redistribution" in bad.stderr and not (tmp_path / "c.txt").exists() and not (tmp_path / "no").exists()
    assert b"Tree read." not in bad.stdout                                             # before the tree is loaded
    bad = run_cli(cli, ctr, fa, tmp_path / "c.txt", 1, UTREE_REDISTRIBUTE=str(tmp_path / "r.tsv"), UTREE_REDIST_PASSES="0")
    assert bad.returncode == 1 and not (tmp_path / "c.txt").exists()
    # a file that cannot be written after the search: the search's stdout and output, the cause on stderr, exit 1
    plain = run_cli(cli, ctr, fa, tmp_path / "a.txt", 1)
    full = run_cli(cli, ctr, fa, tmp_path / "d.txt", 1, UTREE_REDISTRIBUTE="/dev/full")
    assert full.returncode == 1 and full.stdout == plain.stdout and b"redistribution /dev/full" in full.stderr
    assert (tmp_path / "d.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    # a table too small: the same, and the message says what to raise
    red = tmp_path / "r.tsv"
    small = run_cli(cli, ctr, fa, tmp_path / "e.txt", 1, UTREE_REDISTRIBUTE=str(red), UTREE_REDIST_CAPACITY="16")
    assert small.returncode == 1 and small.stdout == plain.stdout and b"UTREE_REDIST_CAPACITY" in small.stderr and not red.exists()


def test_rank_specific_cli_ignores_the_variable(torch_cuda, tmp_path):
    ctr, fa = util.fixture_ctr("toy"), util.fixture_reads_path("toy")
    plain = run_cli(lib.RANK_CLI_PATH, ctr, fa, tmp_path / "a.txt", 0)
    withr = run_cli(lib.RANK_CLI_PATH, ctr, fa, tmp_path / "b.txt", 0, UTREE_REDISTRIBUTE=str(tmp_path / "no" / "dir" / "r.tsv"))
    assert plain.returncode == withr.returncode == 0 and plain.stdout == withr.stdout
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes() == util.fixture_bytes("toy_rank.txt.gz")
    assert not (tmp_path / "no").exists()
