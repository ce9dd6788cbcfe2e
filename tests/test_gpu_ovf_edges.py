"""Overflow runs at their thresholds (tests/ovf_inputs.py: databases whose buckets hold a chosen number of k-mers, and a model of the
image's overflow area), through the lane-per-read pass and the wave-per-read kernels, both strand modes, every record format and both
bucket sizes, and under the A/B switches UTREE_OVF_SCAN, UTREE_OVF_DIR, UTREE_OVF_CHAINS and UTREE_MID_LIMIT.

Every comparison is byte equality with the CPU oracle's search_file output on the same reads.  utree_dev_info.overflow_bytes must equal
the model's figure: that is what shows each designed count landed in its bucket.

The databases "thresholds", "not heavy" and "positions" (and a run of sliding k-mers, which chains link) are the spec groups of ONE
database per record format and bucket size ("edges": distinct slots), so that the file stays at a few dozen uploads of the 2 GiB table
a small database still gets.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, classify_fasta_bytes
import ovf_inputs as ov
import util
from test_gpu_parity import fasta_bytes, random_reads

FORMATS = [(8, 2), (8, 4), (16, 2), (16, 4)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("ovf_edges")


def oracle_text(o, data, workdir, rc):
    fa, out = workdir / "r.fa", workdir / "o.txt"
    fa.write_bytes(data)
    code, nr, good, err = o.search_file(str(fa), str(out), threads=8, rc=rc)
    assert code == 0, err
    return out.read_bytes()


_CASES = {}


def case(workdir, which, W, I, bb, filler=0):
    """(built, path of the .ctr, reads as FASTA, {rc: the oracle's lines}): made once per database, shared by the tests, never changed."""
    key = (which, W, I, bb, filler)
    if key not in _CASES:
        k = 4 * W
        if which == "edges":
            specs = ov.thresholds_specs(W, I, bb) + ov.not_heavy_specs(W, I, bb) + ov.positions_specs(W, I, bb) + ov.stretch_specs(W, I, bb)
            built = ov.build(k, specs, seed=100 + W + I + bb, filler=filler)
            reads = ov.reads_for(built, seed=7)[0]
        elif which == "sixteen":
            built = ov.build(k, ov.sixteen_bits_specs(W, I, bb), seed=16 + W)
            reads = ov.reads_for(built, seed=8, sample=3000)[0]
        else:
            built = ov.build(k, ov.many_runs_specs(W, I, bb), seed=200 + W)
            reads = ov.stitched_reads(built, 2048, seed=9, n_forward=1536) + ov.reads_for(built, seed=10, random_reads=100)[0]
        ctr = built.write(str(workdir / ("%s_%d_%d_%d_%d.ctr" % key)), I)
        data = ov.fasta(reads)
        o = orc.OracleDB.load(ctr)
        want = {rc: oracle_text(o, data, workdir, rc) for rc in (False, True)}
        o.close()
        n_named = sum(1 for n, _ in reads if n[0] == "a")
        assert want[False].count(b"\n") >= n_named                                        # every placed k-mer's read is classified
        _CASES[key] = (built, ctr, data, want)
    return _CASES[key]


def upload(ctr, W, I, bb, monkeypatch, **env):
    monkeypatch.setenv("UTREE_BUCKET_BYTES", str(bb))
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))
    db = CtrDB.open(ctr)
    tree = DeviceTree.upload(db, 0)
    assert tree.info.bucket_bytes == bb and not tree.info.generic_mode and tree.info.irregular_bins == 0
    assert tree.info.lane_pass == (0 if (W, I) == (16, 4) else 1)                        # k = 64 with u32 labels: the wave-per-read kernels alone
    return db, tree


def both_kernel_families_both_strands(db, tree, data, want, monkeypatch):
    for lane_pass in ("1", "0"):
        monkeypatch.setenv("UTREE_LANE_PASS", lane_pass)
        for rc in (False, True):
            got = classify_fasta_bytes(db, tree, data, rc=rc)
            if lane_pass == "1" and tree.info.lane_pass:
                assert tree.kernel_name().startswith("classify_lanes_"), tree.kernel_name()
            else:
                assert "classify_short_k" in tree.kernel_name(), tree.kernel_name()
            assert got == want[rc], (lane_pass, rc)


def check_edges_model(built, m, W, I, bb, cond):
    """The model of the edges database: a bucket that one spec fills alone overflows from CAP+1 records and its run is heavy from 33 -- the
    directory appears exactly between 32 and 33 --; of the two buckets that two hash values share, the run that holds both is not heavy
    and the run that holds one alone is."""
    CAP, D = ov.cap(W, I, bb), ov.dir_slots(W, I)
    by_bucket = {r[0]: r for r in m["runs"]}
    by_name = {s.name: s for s in built.specs}
    assert len(by_name) == len(built.specs)
    shared = {"mix_lo": "mix_hi", "inline_lo": "heavy_hi"}
    extra = lambda heavy: D if heavy and cond != "nodir" else 0
    for s in built.specs:
        if s.name in shared or s.name in shared.values():
            continue
        r = by_bucket.get(ov.bucket_of(s))
        c = s.n - (CAP - 1)
        if s.n <= CAP:
            assert r is None, s.name
        else:
            assert r[1:4] == (s.n, c, c > 32), (s.name, r)
            if not (cond == "chains" and c > 32):                              # (as chains: ovf_inputs.chain_heads decides the size)
                assert r[4] == c + extra(c > 32), (s.name, r)
    for lo, hi, heavy in (("mix_lo", "mix_hi", False), ("inline_lo", "heavy_hi", True)):
        assert ov.bucket_of(by_name[lo]) == ov.bucket_of(by_name[hi]) and by_name[lo].hash < by_name[hi].hash
        r = by_bucket[ov.bucket_of(by_name[lo])]
        assert r[1:4] == (CAP - 1 + 40, 40, heavy) and by_name[lo].n + by_name[hi].n == CAP - 1 + 40, (lo, r)
        if cond != "chains":
            assert r[4] == 40 + extra(heavy), (lo, r)
    assert by_name["c32"].n == 32 + CAP - 1 and by_name["c33"].n == 33 + CAP - 1            # both sides of the threshold are there
    assert m["ovf_scan"] == (32 if cond == "auto32" else 16)


# The sweep: every record format and bucket size under every condition.  UTREE_OVF_SCAN is the lane pass's threshold alone, so it is swept where
# the handle takes the lane pass; chains exist for k = 32.
CONDITIONS = [(W, I, bb, cond) for W, I in FORMATS for bb in (64, 128)
              for cond in ("auto16", "auto32", "scan1", "scan16", "scan32", "scan1024", "nodir", "chains")
              if not (cond.startswith("scan") and (W, I) == (16, 4)) and not (cond == "chains" and W != 8)]


@pytest.mark.parametrize("W,I,bb,cond", CONDITIONS)
def test_runs_at_their_thresholds(torch_cuda, workdir, monkeypatch, W, I, bb, cond):
    """Buckets of CAP-1 .. CAP+2 records, runs of 15, 16, 17, 31, 32, 33, 34 and 100 records, a run of 40 that two hash values share, heavy
    runs with all records at one end of the position range, at every other position, or lumped at one.  As it is the database is
    overflow-heavy (automatic scan threshold 16), with filler it is not (32); then the threshold forced to 1, 16, 32, 1024, the directories
    off, and the heavy runs as chains."""
    built, ctr, data, want = case(workdir, "edges", W, I, bb, filler=6000 if cond == "auto32" else 0)
    m = ov.model(built, I, bb, dir_on=cond != "nodir", chains=cond == "chains")
    env = {}
    if cond.startswith("scan"):
        env["UTREE_OVF_SCAN"] = cond[4:]
    elif cond == "nodir":
        env["UTREE_OVF_DIR"] = "0"
    elif cond == "chains":
        env["UTREE_OVF_CHAINS"] = "1"
    check_edges_model(built, m, W, I, bb, cond)
    db, tree = upload(ctr, W, I, bb, monkeypatch, **env)
    assert tree.info.overflow_chains == (1 if cond == "chains" else 0)
    assert tree.info.overflow_bytes == m["bytes"], (tree.info.overflow_bytes, m["bytes"])
    # (as chains the image is not smaller than behind directories here: k-mers with random flanks link into no chains, each record is a chain
    # of its own -- 16 bytes and a rank against 8 or 16 bytes as a record; only the run of sliding k-mers shrinks)
    if cond == "nodir":
        with_dir = ov.model(built, I, bb)
        n_heavy = sum(1 for r in with_dir["runs"] if r[3])
        assert n_heavy >= 9 and with_dir["bytes"] - m["bytes"] == n_heavy * ov.dir_slots(W, I) * ov.rec_words(W, I) * 8
    both_kernel_families_both_strands(db, tree, data, want, monkeypatch)
    tree.close()
    db.close()


@pytest.mark.parametrize("W", [8, 16])
def test_directory_offsets_end_at_sixteen_bits(torch_cuda, workdir, monkeypatch, W):
    """A run of exactly 65535 records is heavy (its directory's last entry is 65535, the largest a 16-bit offset holds); one of 65536 is not."""
    built, ctr, data, want = case(workdir, "sixteen", W, 2, 64)
    m = ov.model(built, 2, 64)
    assert sorted(r[2:] for r in m["runs"]) == [(65535, True, 65535 + ov.dir_slots(W, 2)), (65536, False, 65536)]
    db, tree = upload(ctr, W, 2, 64, monkeypatch)
    assert tree.info.overflow_bytes == m["bytes"], (tree.info.overflow_bytes, m["bytes"])
    both_kernel_families_both_strands(db, tree, data, want, monkeypatch)
    tree.close()
    db.close()


@pytest.mark.parametrize("bb", [64, 128])
@pytest.mark.parametrize("W,I", FORMATS)
def test_more_overflowing_runs_than_lanes_in_a_wavefront(torch_cuda, workdir, monkeypatch, W, I, bb):
    """200 overflowing buckets, 150-base reads that each cross several of them (ovf_inputs.stitched_reads has the geometry), every record
    format and bucket size: the descriptor a later round prefetches sits at another offset in each.  The database is overflow-heavy, so the
    lane pass reads runs of up to 16 records whole and searches longer ones per window.  The first 1536 of the 2048 stitched reads are
    forward reads: 24 times the 64 consecutive reads a wavefront takes.  Forward strand, one such wavefront:
    k = 32: 5 overflowing runs per read = 320, five rounds of the loop over 64 runs (the later ones on prefetched descriptors).  128 of the runs
            are SHORT (9 .. 16 records): >= 1152 records in five rounds, so some round scans >= 231 > 64 records -- more than one step.  192 are
            LONG with >= 64 * (1 + 17 + 7) = 1600 windows in five rounds: some round searches >= 320 > 256 windows, more than one step of 4 x 64.
    k = 64: 3 to 4 runs per read, 192 .. 256: three or four rounds.  >= 64 SHORT runs of >= 9 records = 576 in at most four rounds: some round
            scans >= 144 > 128 records (two blocks of 64 per step).  LONG: >= 64 * (24 + 13) = 2368 windows: some round searches >= 592 > 256.
    The 512 reads behind them are reverse-complemented (every core names the other bucket of its pair; no count is claimed for them).
    With both strands every run has two overflowing buckets and the list outgrows its room: those reads go to the wave-per-read kernel.
    k = 64 with u32 labels: the wave-per-read kernels alone."""
    built, ctr, data, want = case(workdir, "many", W, I, bb)
    names = [l[1:] for l in data.split(b"\n")[0:2 * 2048:2]]
    assert names == [b"s%d" % i for i in range(2048)]                                     # the stitched reads come first, in order
    m = ov.model(built, I, bb)
    assert len(m["runs"]) == 200 and m["ovf_scan"] == 16 and min(r[2] for r in m["runs"]) == 5 and max(r[2] for r in m["runs"]) == 60
    short = [r[2] for r in m["runs"] if r[0] % 2 == 0 and r[2] != 5]
    assert min(short) == 9 and max(short) == 16 and min(r[2] for r in m["runs"] if r[0] % 2) == 17
    db, tree = upload(ctr, W, I, bb, monkeypatch)
    assert tree.info.overflow_bytes == m["bytes"], (tree.info.overflow_bytes, m["bytes"])
    both_kernel_families_both_strands(db, tree, data, want, monkeypatch)
    tree.close()
    db.close()


_LONG_READS = {}


@pytest.mark.parametrize("lane_pass", ["1", "0"])
@pytest.mark.parametrize("name,rc", [("toy", 0), ("toy", 1), ("k64", 0), ("k64", 1)])
def test_mid_limit_switch(torch_cuda, workdir, name, rc, lane_pass):
    """UTREE_MID_LIMIT moves the boundary between the wave-per-read mid pass and classify_long_k.  Its value is cached per process, so the
    search command line runs in a child process: reads of 600 .. 2200 bases, the oracle's lines with the limit at 640, at 1536 and unset,
    with the lane pass (which takes such reads in pieces, and sizes its workspace by the limit) and with the wave-per-read kernels alone."""
    if name not in _LONG_READS:
        d = util.load_db_fixture(name)
        rng = np.random.default_rng(640)
        data = fasta_bytes(random_reads(rng, d, 300, 600, 2200, hit_frac=0.7))
        o = orc.OracleDB.load(util.fixture_ctr(name))
        _LONG_READS[name] = (data, {r: oracle_text(o, data, workdir, bool(r)) for r in (0, 1)})
        o.close()
    data, want = _LONG_READS[name]
    fa = workdir / ("long_%s.fa" % name)
    fa.write_bytes(data)
    assert want[rc].count(b"\n") > 200
    outs = {}
    for limit in (None, "640", "1536"):
        env = {k: v for k, v in os.environ.items() if k != "UTREE_MID_LIMIT"}
        env["UTREE_LANE_PASS"] = lane_pass
        if limit:
            env["UTREE_MID_LIMIT"] = limit
        out = workdir / ("mid_%s_%d_%s_%s.txt" % (name, rc, lane_pass, limit))
        r = subprocess.run([lib.CLI_PATH, util.fixture_ctr(name), str(fa), str(out), "4"] + (["RC"] if rc else []), env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        outs[limit] = out.read_bytes()
        assert outs[limit] == want[rc], limit
    assert outs["640"] == outs[None] and outs["1536"] == outs[None]
