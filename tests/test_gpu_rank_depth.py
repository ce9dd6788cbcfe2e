"""The rank-specific search (`xtree-search`) at the batch sizes the file pipeline runs it at, and on the edges of its
kernels (rank_kernels.hip), against the CPU oracle, byte for byte and record for record:

  * batches of more than 2 * 262 144 reads: prev_greater's descent through lvl[1] and lvl[2] of the max tree, and
    rank_state_k's `after` from them, read back by the next batch (tests/rank_inputs.py: depth_case; its layout
    conditions are asserted in tests/test_rank_depth_cpu.py, where the oracle is also held to the genuine binaries);
  * the vote's split between one entry per lane (<= 63 hits) and the label histogram, around planted ties;
  * hits at the 64-window blocks and 960-window LDS segments of rank_hits_k and the register word after them, k = 32, 64;
  * the 'N' between a read and its reverse complement;
  * the hit-list workspace exactly as utree_rank_workspace_bytes sizes it.

Run on the MI355X box:  python -m pytest tests/test_gpu_rank_depth.py -m gpu -q
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import lib
from utree_amd.search import frame_fasta, search_rank
import rank_inputs as ri
from test_gpu_rank import tree_for

P32 = dict(slack=1, sparsity=32, tolerance=1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def same_records(res, want):
    """Field by field, as test_rank_records_match_oracle: hits kept; most, secondMost, printed where there is a hit; the
    label where the line is printed."""
    assert len(res) == len(want)
    assert np.array_equal(res[:, 2], want["found"].astype(np.int32))
    hit = want["found"] > 0
    assert np.array_equal(res[hit, 4], want["most"][hit].astype(np.int32))
    assert np.array_equal(res[hit, 5], want["second"][hit].astype(np.int32))
    assert np.array_equal(res[hit, 1] == -2, want["printed"][hit] != 0)
    pr = hit & (want["printed"] != 0)
    assert np.array_equal(res[pr, 0], want["label"][pr].astype(np.int32))


def oracle_file(name, fa, out, rc=False, **prm):
    code, nr, good, err = orc.rank_search_file(ri.oracle_db(name), str(fa), str(out), rc=rc, **prm)
    assert code == 0, err
    return out.read_bytes(), nr


def run_split(torch, db, tree, data, rc=False, batch=None, cuts=None, **prm):
    """The batch operator over the file's reads in order, `batch` reads at a time (None: all at once) or in batches that
    end at the read indices `cuts`; returns (formatted bytes, records).  test_gpu_rank.run_batches with free cut points."""
    fr = frame_fasta(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    n = len(fr["seq_off"])
    if cuts is None:
        cuts = range(batch, n, batch) if batch else []
    tree.rank_reset()
    recs = []
    for a, b in zip([0] + list(cuts), list(cuts) + [n]):
        off = torch.from_numpy(fr["seq_off"][a:b].astype(np.int64)).cuda()
        ln = torch.from_numpy(fr["seq_len"][a:b].astype(np.int32)).cuda()
        recs.append(tree.rank_search(d_buf, off, ln, rc=rc, **prm).cpu().numpy())
    res = np.concatenate(recs)
    return db.format(buf, fr["name_off"], fr["name_len"], res, rank=True), res


def check_file(torch, name, data, tmp_path, rc=False, **prm):
    """File -> file and the batch operator on the whole file as one batch, both against the oracle; returns its records."""
    db, tree = tree_for(name)
    fa = tmp_path / "r.fa"
    fa.write_bytes(data)
    want, nr = oracle_file(name, fa, tmp_path / "w.txt", rc=rc, **prm)
    out = tmp_path / "g.txt"
    code, st = search_rank(db, tree, str(fa), str(out), rc=rc, threads=4, **prm)
    assert code == lib.OK and st.n_reads == nr
    assert out.read_bytes() == want
    recs = ri.oracle_records(name, data, rc=rc, **prm)
    got, res = run_split(torch, db, tree, data, rc, **prm)
    same_records(res, recs)
    assert got == want
    return recs


# ---- 1, 2: depth ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def depth(tmp_path_factory):
    """The depth file, and the oracle's output on it under the default parameters."""
    c = ri.depth_case(1)
    d = tmp_path_factory.mktemp("depth")
    fa = d / "depth.fa"
    fa.write_bytes(c.data)
    want, nr = oracle_file("rk", fa, d / "want.txt")
    assert nr == c.n and want.count(b"\n") == int(c.records["printed"].sum()) > 50000
    return c, fa, want


@pytest.mark.parametrize("prm", [dict(), P32], ids=["default", "p32s1t1"])
def test_depth_file_to_file(torch_cuda, depth, prm, tmp_path):
    """528 485 reads in one batch of the file pipeline: two full 262 144-read supergroups and a part of a third."""
    c, fa, want = depth
    if prm:
        want, _ = oracle_file("rk", fa, tmp_path / "w.txt", **prm)
    db, tree = tree_for("rk")
    out = tmp_path / "g.txt"
    code, st = search_rank(db, tree, str(fa), str(out), threads=4, **prm)
    assert code == lib.OK and st.n_reads == c.n
    assert out.read_bytes() == want


def test_depth_one_batch_records(torch_cuda, depth):
    c, fa, want = depth
    db, tree = tree_for("rk")
    got, res = run_split(torch_cuda, db, tree, c.data)
    same_records(res, c.records)
    assert got == want


@pytest.mark.parametrize("batch", [300000, 262144, 262145, 4096, 65537])
def test_depth_across_batches(torch_cuda, depth, batch):
    """The same bytes as in one batch -- the oracle's, test_depth_one_batch_records -- whatever the batch size: here
    rank_state_k takes `after` from lvl[1] / lvl[2] and a later batch reads the result back from the carried array."""
    c, fa, want = depth
    db, tree = tree_for("rk")
    got, res = run_split(torch_cuda, db, tree, c.data, batch=batch)
    same_records(res, c.records)
    assert got == want


def test_depth_after_a_batch_without_hits(torch_cuda, depth):
    c, fa, want = depth
    first = int(np.flatnonzero(c.records["found"])[0])
    assert first >= 5
    db, tree = tree_for("rk")
    got, res = run_split(torch_cuda, db, tree, c.data, cuts=[first])
    same_records(res, c.records)
    assert got == want


# ---- 3: the vote's split at 64 entries -------------------------------------------------------------------------------
@pytest.mark.parametrize("prm", [dict(slack=2, sparsity=4, tolerance=2), dict(slack=1, sparsity=4, tolerance=1)], ids=["s2t2", "s1t1"])
def test_vote_split_in_a_full_batch(torch_cuda, prm, tmp_path):
    """Reads keeping 62, 63, 64 and 65 hits after donors whose entry n makes, breaks or leaves a tie, in one batch with more
    label-histogram votes than there are histograms (n_cu * 8): each is used again, so its zeroing after a read is under test."""
    v = ri.vote_split_case(1)
    recs = check_file(torch_cuda, "rk", v.data, tmp_path, **prm)
    assert set(recs["found"][v.targets].tolist()) == {62, 63, 64, 65}
    n_cu = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    assert int(np.sum(recs["found"] >= 64)) > n_cu * 8


@pytest.mark.parametrize("prm", [dict(slack=2, sparsity=4, tolerance=2), dict(slack=1, sparsity=4, tolerance=1)], ids=["s2t2", "s1t1"])
def test_vote_split_one_read_per_batch(torch_cuda, prm):
    """The first 160 reads (every mix, count and donor once), each the only read of its batch: one histogram wavefront."""
    v = ri.vote_split_case(1)
    off, ln = ri.frame(v.data)
    data = v.data[: int(off[159] + ln[159]) + 1]
    recs = ri.oracle_records("rk", data, **prm)
    assert len(recs) == 160 and set(recs["found"][v.targets[:80]].tolist()) == {62, 63, 64, 65}
    db, tree = tree_for("rk")
    _, res = run_split(torch_cuda, db, tree, data, batch=1, **prm)
    same_records(res, recs)


# ---- 4, 5: block and segment edges of rank_hits_k; the N joint ------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("name", ["rk", "k64"])
def test_hits_at_block_and_segment_edges(torch_cuda, name, rc, tmp_path):
    e = ri.edge_case(name)
    recs = check_file(torch_cuda, name, e.data, tmp_path, rc=rc)
    laid = np.concatenate([e.fwd, e.rc]) if rc else e.fwd
    assert recs["found"][laid].min() >= 2


@pytest.mark.parametrize("name", ["rk", "k64"])
def test_n_joint_under_rc(torch_cuda, name, tmp_path):
    j = ri.joint_case(name)
    recs = check_file(torch_cuda, name, j.data, tmp_path, rc=True)
    assert not recs["found"][j.short].any()               # every window holds the separator: no hit, no line
    assert np.all(recs["found"][j.last_fwd] >= 1) and np.all(recs["found"][j.first_rev] == 1)
    fwd = check_file(torch_cuda, name, j.data, tmp_path, rc=False)
    assert np.all(fwd["found"][j.last_fwd] == 1) and not fwd["found"][j.first_rev].any()


# ---- 6: the workspace as sized -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["511", "511_512_513"])
def test_workspace_as_sized(torch_cuda, mixed):
    """utree_rank_batch with exactly utree_rank_workspace_bytes(...) bytes, a 1 MiB tail of 0xA5 behind them: reads that reserve
    511 hit-list entries (one below the direct path; mixed: 512 and 513 too) and fill them.
    What this checks: the records, with every list filled to its last reserved entry next to its neighbours' (an overrun
    changes their votes), on both the chunked (511) and the direct (512, 513) path, and no write behind the sized bytes.
    What it does not: the slack terms of the formula.  A wavefront reserves a new 8 192-entry chunk only after more than
    one grab of 16 reads (16 * 511 = 8 176 entries fit one chunk), and there are n_cu * 32 wavefronts, so the entries
    abandoned at a refill -- the 9/8 in `carve` -- arise only in batches of more than n_cu * 512 such reads (131 072 reads,
    540 MB, on 256 CUs), too large for this suite; and the n_cu * 32 * 8 192 entries for part-used chunks dwarf the
    ~0.6 M entries used here, with the label histograms lying between the lists and the guarded tail."""
    torch = torch_cuda
    db, tree = tree_for("rk")
    data = ri.workspace_case(mixed)
    want = ri.oracle_records("rk", data)
    off, ln = ri.frame(data)
    assert int(want["found"].max()) == (513 if mixed else 511)
    n, total, longest = len(off), int(ln.sum()), int(ln.max())
    L = lib.load()
    prm = lib.RankParams(2, 4, 2)
    need = L.utree_rank_workspace_bytes(tree._h, n, total, longest, 0, C.byref(prm))
    assert need > 0
    tail = 1 << 20
    ws = torch.empty(need + tail, dtype=torch.uint8, device="cuda")
    ws[need:] = 0xA5
    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_len = torch.from_numpy(ln.astype(np.int32)).cuda()
    out = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    tree.rank_reset()
    lib.check(L.utree_rank_batch(tree._h, d_buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, total, longest, 0, C.byref(prm),
                                 out.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "utree_rank_batch")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the batch wrote past the workspace it asked for"
    same_records(out.cpu().numpy(), want)
