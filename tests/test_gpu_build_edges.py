"""The database BUILD on the GPU (build_gpu.hip) at its edges: base coding over every 7-bit byte, position -> reference and the ordered
compaction at the wavefront and block boundaries, k-mer range passes, the label numbering clock, the two-pass k = 64 sort, phase 2 in
several launches, and the counts nobody else reads (n_kmers, n_distinct).

Every input comes from tests/build_inputs.py.  `search.build` must write the CPU oracle's `.ubt` and log byte for byte; the oracle is held
to the genuine builders and to the numpy model on the same bytes in tests/test_build_edges_cpu.py.  The counts are checked against the
numpy model, which knows neither the oracle nor the kernels.

Run on the MI355X box:  python -m pytest tests/test_gpu_build_edges.py -m gpu -q
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import lib
from utree_amd.search import build
import build_inputs as B
import util

RUNS = B.runs()
BY_KEY = {r.key: r for r in RUNS}
# the inputs that have k-mers, once each: (name, W, complevel) -> a recorded run of it
CASES = {}
for _r in RUNS:
    if "_none_" not in _r.key:
        CASES.setdefault((_r.key.split("_")[2], _r.W, _r.lv), _r)
_MEMO = {}


def prepared(r, d):
    """The case's files in directory d, and its model (made once per module)."""
    k = (r.key.split("_")[2], r.W, r.lv)
    if k not in _MEMO:
        c = r.make()
        _MEMO[k] = (c, B.model(c.fa, r.W, r.lv))
    c, m = _MEMO[k]
    fa, mp = os.path.join(str(d), "i.fa"), os.path.join(str(d), "i.map")
    open(fa, "wb").write(c.fa)
    open(mp, "wb").write(c.map)
    return c, m, fa, mp


def files(ubt, gg):
    log = ubt + (".gg.log" if gg else ".log")
    return open(ubt, "rb").read(), open(log, "rb").read()


def oracle_files(fa, mp, d, W, I, lv, gg):
    want = os.path.join(str(d), "want_%d_%d.ubt" % (I, gg))
    code, ns, nn, nl, err = orc.build_file(fa, mp, want, W=W, I=I, complevel=lv, gg=bool(gg))
    assert code == 0, err
    return files(want, gg), nn, nl


def gpu_files(fa, mp, d, W, I, lv, gg, tag="got"):
    got = os.path.join(str(d), "%s_%d_%d.ubt" % (tag, I, gg))
    code, st = build(fa, mp, got, W=W, I=I, complevel=lv, gg=bool(gg))
    assert code == lib.OK, code
    return files(got, gg), st


def check_against_oracle_and_model(r, d, I, gg):
    c, m, fa, mp = prepared(r, d)
    want, nn, nl = oracle_files(fa, mp, d, r.W, I, r.lv, gg)
    got, st = gpu_files(fa, mp, d, r.W, I, r.lv, gg)
    assert (st.n_kmers, st.n_distinct) == (m.n_kmers, m.n_distinct)            # label-independent: the model counts them for every case
    if r.one_label:
        assert (st.n_nodes, st.n_labels) == (m.n_distinct, 1)
        assert got == (B.ubt_bytes(m, r.W, I), B.label_lines(B.ONE, m.n_distinct))
    assert (st.n_nodes, st.n_labels) == (nn, nl)
    assert got[0] == want[0]
    assert got[1] == want[1]
    key = r.key.rsplit("_", 1)[0] + ("_gg" if gg else "_plain")
    if I == 2 and key in BY_KEY:                                               # and what the genuine builder wrote on these bytes
        ref = util.reference_run(key, fa=c.fa, map=c.map)
        assert (util.sha256_of(got[0]), util.sha256_of(got[1])) == (ref["outputs"]["ubt"], ref["outputs"]["log"])
    return got


@pytest.mark.parametrize("name,W,lv", sorted(CASES))
def test_build_edge_case(name, W, lv, tmp_path):
    """Every case, BUILD_GG and plain BUILD, 2-byte label indices; the byte and the extremes cases with 4-byte indices too."""
    r = CASES[(name, W, lv)]
    for gg in (1, 0):
        check_against_oracle_and_model(r, tmp_path, 2, gg)
    if name.startswith(("bytes", "extremes")):
        for gg in (1, 0):
            check_against_oracle_and_model(r, tmp_path, 4, gg)


PASS_CASES = [(n, W) for n in ("extremes1", "extremes3", "clock") for W in B.WS] + [("stability", 16)]


@pytest.mark.parametrize("name,W", PASS_CASES)
def test_build_edge_passes(name, W, tmp_path, monkeypatch):
    """UTREE_BUILD_PASS_KMERS at the largest bucket's size, the smallest limit the build accepts: the planted words fall into different
    passes (build_inputs.pass_ranges restates the host's greedy ranges), every range drags empty buckets along, and nothing changes."""
    r = CASES[(name, W, 0)]
    c, m, fa, mp = prepared(r, tmp_path)
    limit = int(m.hist.max())
    ranges = B.pass_ranges(m.hist, limit)
    if name.startswith("extremes"):
        planted = [0, 4095]
    elif name == "clock":
        planted = [int(B.bucket_of(W, *B.positions(c.planted["words"][k], W, 0)[1:])[0]) for k in "XYZ"]
    else:
        planted = sorted({int(B.bucket_of(16, *B.positions(w, 16, 0)[1:])[0]) for w in c.planted["words"]})     # one bucket per high half
    assert len({B.pass_of(ranges, b) for b in planted}) == len(set(planted)) >= 2
    assert sum(e - b for b, e, _ in ranges) == B.N_BUCKETS and int(np.count_nonzero(m.hist)) < B.N_BUCKETS // 2
    for gg in (1, 0):
        single, st1 = gpu_files(fa, mp, tmp_path, W, 2, 0, gg, "single")
        monkeypatch.setenv("UTREE_BUILD_PASS_KMERS", str(limit))
        multi, st2 = gpu_files(fa, mp, tmp_path, W, 2, 0, gg, "multi")
        monkeypatch.delenv("UTREE_BUILD_PASS_KMERS")
        assert multi == single == oracle_files(fa, mp, tmp_path, W, 2, 0, gg)[0]
        assert (st2.n_kmers, st2.n_distinct, st2.n_nodes, st2.n_labels) == (st1.n_kmers, st1.n_distinct, st1.n_nodes, st1.n_labels)
        assert (st2.n_kmers, st2.n_distinct) == (m.n_kmers, m.n_distinct)      # n_distinct is summed over the passes


@pytest.mark.parametrize("W", B.WS)
def test_build_edge_refuses_a_bucket_over_the_limit(W, tmp_path, monkeypatch):
    """One bucket (the all-A word's) larger than the limit: E_NOMEM and no file; the same input then builds in the same process."""
    r = CASES[("extremes3", W, 0)]
    c, m, fa, mp = prepared(r, tmp_path)
    assert B.pass_ranges(m.hist, int(m.hist.max()) - 1) is None
    monkeypatch.setenv("UTREE_BUILD_PASS_KMERS", str(int(m.hist.max()) - 1))
    ubt = str(tmp_path / "refused.ubt")
    code, st = build(fa, mp, ubt, W=W, I=2, complevel=0, gg=True)
    assert code == lib.E_NOMEM
    assert not os.path.exists(ubt) and not os.path.exists(ubt + ".gg.log")
    monkeypatch.delenv("UTREE_BUILD_PASS_KMERS")
    check_against_oracle_and_model(r, tmp_path, 2, 1)


@pytest.mark.parametrize("W", B.WS)
def test_build_edge_phase2_chunks(W, tmp_path, monkeypatch):
    """UTREE_TEST_BUILD_CHUNK: phase 2 in several launches (`first` > 0), one segment and several (pass hook): file, log counts and the
    per-label node counts (the log's second column, summed over the launches) equal the run in one launch.  One label, and a label per
    reference."""
    for name, gg in (("shape513", 1), ("shapemany513", 0)):
        r = CASES[(name, W, 0)]
        c, m, fa, mp = prepared(r, tmp_path)
        N = m.n_distinct
        assert N > 500
        whole, st0 = gpu_files(fa, mp, tmp_path, W, 2, 0, gg, "whole")
        assert st0.n_nodes == N and whole == oracle_files(fa, mp, tmp_path, W, 2, 0, gg)[0]
        seg_limit = 64
        assert len(B.pass_ranges(m.hist, seg_limit)) >= 5
        for limit in (None, seg_limit):
            if limit:
                monkeypatch.setenv("UTREE_BUILD_PASS_KMERS", str(limit))
            for chunk in (1, 255, 256, 257, N - 1, N, N + 1):
                monkeypatch.setenv("UTREE_TEST_BUILD_CHUNK", str(chunk))
                got, st = gpu_files(fa, mp, tmp_path, W, 2, 0, gg, "chunk")
                assert got[1] == whole[1], (name, limit, chunk)                # labels and per-label counts
                assert got[0] == whole[0], (name, limit, chunk)
                assert (st.n_nodes, st.n_labels, st.n_distinct) == (st0.n_nodes, st0.n_labels, st0.n_distinct)
            monkeypatch.delenv("UTREE_TEST_BUILD_CHUNK")
            monkeypatch.delenv("UTREE_BUILD_PASS_KMERS", raising=False)


@pytest.mark.parametrize("W", B.WS)
def test_build_edge_no_kmers(W, tmp_path):
    """No position at all (total_pos == 0), positions but no valid window, and a filter nothing passes: BUILD_E_NO_KMERS, no file."""
    for which, lv in B.NO_KMERS.items():
        r = BY_KEY["build_edges_none_%s_W%d_c%d_gg" % (which, W, lv)]
        c = r.make()
        assert util.reference_run(r.key, fa=c.fa, map=c.map)["exit"] == 2
        fa, mp = tmp_path / (which + ".fa"), tmp_path / (which + ".map")
        fa.write_bytes(c.fa)
        mp.write_bytes(c.map)
        for gg in (1, 0):
            ubt = str(tmp_path / ("%s%d.ubt" % (which, gg)))
            code, st = build(str(fa), str(mp), ubt, W=W, I=2, complevel=lv, gg=bool(gg))
            assert code == lib.E_BUILD and st.error_kind == lib.BUILD_E_NO_KMERS
            assert (st.n_kmers, st.n_nodes) == (0, 0)
            assert not os.path.exists(ubt) and not os.path.exists(ubt + ".gg.log") and not os.path.exists(ubt + ".log")


@pytest.mark.parametrize("key", ["build_edges_extremes3_W8_c0_gg", "build_edges_stability_W16_c0_gg", "build_edges_bytes_W4_c2_gg"])
def test_build_edge_cli_prints_the_reference_lines(key, tmp_path):
    """`utree-buildGG in.fa in.map out.ubt 1 complevel` prints what the genuine builder printed on these bytes, line for line --
    `Done with sequence parse: N k-mers made` (the distinct k-mers) among them -- and writes its files."""
    r = BY_KEY[key]
    c = r.make()
    ref = util.reference_run(key, fa=c.fa, map=c.map)
    fa, mp, ubt = tmp_path / "i.fa", tmp_path / "i.map", str(tmp_path / "o.ubt")
    fa.write_bytes(c.fa)
    mp.write_bytes(c.map)
    env = dict(os.environ, UTREE_PACKSIZE=str(4 * r.W), UTREE_IXTYPE="16")
    p = subprocess.run([lib.BUILD_GG_CLI_PATH, str(fa), str(mp), ubt, "1", str(r.lv)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                       timeout=300)
    assert p.returncode == ref["exit"] == 0, p.stderr.decode()
    lines = p.stdout.decode("latin-1").splitlines()
    assert lines == ref["stdout"]
    m = B.model(c.fa, r.W, r.lv)
    assert "Done with sequence parse: %d k-mers made" % m.n_distinct in lines
    assert (util.sha256_of(ubt), util.sha256_of(ubt + ".gg.log")) == (ref["outputs"]["ubt"], ref["outputs"]["log"])
