"""Tiled classification (csrc/tiles_kernels.hip, csrc/tiles.c, csrc/tiles_file.c, `utree-tiles`) at the tile widths and batch sizes it runs
with: tests/test_gpu_tiles.py classifies eleven queries of up to 3 001 bases at (W, S) = (150, 75), (200, 200) and (100, 33).  Here: the
default (1000, 500); widths on either side of every edge at which the classify path changes its kernels; plans of up to 2^21 queries, more
than 2^32 tiles and ranges of up to 2^21 tiles; the file run with sub-batches that a team formats, with the default split of 2^21 tiles, and
with a malformed record behind the first chunk.

Every comparison is equality: all six record words (assert_records), arrays, or the bytes of a file.  The references -- tiles_ref.views_range,
classify_views, view_files -- are held to numpy_views, to the oracle tile by tile and to the genuine reference's bytes in
tests/test_tiles_scale_cpu.py, which also makes the inputs once for both files.

What reaches what (none of it was reached before):
  tl_count_k's terminator in a block of its own,   test_plan_at_batch_size (n_reads = 256 and 2^21; 65 537 and 2^21 queries: 257 and 8 193 blocks, rocprim's
  the scan over more than one block                multi-block scan, totals beyond 2^32 at (32, 1))
  tl_views_k beyond 2^32: first_tile, g,           test_views_of_a_batch_of_more_than_2_32_tiles
  tile_first[mid] <= g on 64-bit values
  tl_views_k at 1 .. 8 192 blocks, its block       test_ranges_of_every_size (n = 1 .. 2^21; waves and blocks that are part-filled; the zero-length range
  sums and one atomic per block                    that issues no atomic)
  utree_tiles_plan's workspace at any alignment,   test_nothing_is_kept_between_calls
  two views calls in flight on one stream
  a mixed lane-pass batch of overlapping reads of  test_tiles_through_every_classify_pass: (1000, 500) eight lanes; 1063 | 1064 eight | sixteen lanes; with RC
  ONE length above UTREE_LANES_CAP and a shorter   1055 | 1056 the pieces edge; 2095 | 2096 sixteen lanes | pieces; (20000, 7001) every full tile in pieces,
  tail; pieces_k with n_long_cap / n_pieces_cap    total_bases = 2.9 times the buffer; (161, 1) 39 841 two-lane tiles one byte apart; UTREE_LANE_PASS=0:
  carved from W/S times the buffer                 (1000, 500) the wave-per-read mid pass, (2113, 1000) classify_long_k on overlapping reads
  tiles_file.c: format_slice by a team, slices     test_file_run_with_team_formatted_sub_batches (CLI, UTREE_TILES_BATCH = 4096 | 5000 | unset),
  n*k/tm, their in-order write, a slice buffer     test_file_run_through_the_binding_with_every_team (threads = 1: one slice of 6 MB, the buffer doubles three
  grown past 1 MiB, an open run carried out of a   times; 3, 16, 64 -> 16: slices of 23 221 * k / tm)
  team-formatted sub-batch
  the default split at 2^21 tiles                  test_file_run_split_at_the_default_2_21_tiles
  fasta_error.read_index += n_queries - nr         test_framing_error_behind_the_first_chunk[1000]

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tiles_ref
import util
from test_gpu_tally_inline import assert_records
from test_tiles_cpu import ref
from test_tiles_scale_cpu import contig_set, files_ref, giant_batch, oracle, views_ref
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, tiles_file


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_TREE = []


def vote_tree():
    if not _TREE:
        db = CtrDB.open(util.fixture_ctr("vote"))
        _TREE.append((db, DeviceTree.upload(db, 0)))
    return _TREE[0]


def dev(torch, a):
    """a uint32 / uint64 numpy array as the int32 / int64 CUDA tensor the binding takes"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).cuda()


def host(t):
    return [x.cpu().numpy().view(d) for x, d in zip(t, (np.uint64, np.uint32, np.uint32, np.uint32))]


def assert_views(got, want, what):
    for g, w, f in zip(host(got[:4]), want, ("toff", "tlen", "tquery", "tindex")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, f)


def meta_of(total, tlen, error=0):
    return dict(total_tiles=total, total_bases=int(tlen.astype(np.uint64).sum()), max_len=int(tlen.max()) if len(tlen) else 0, error=error)


# ---- A. plan and views at batch size: lengths only, no bases ------------------------------------------------------------------------------

def plan_lengths(n, W, S):
    rng = np.random.default_rng(n + W)
    ln = rng.choice(np.array([0, 1, W - 1, W, W + 1, W + S], dtype=np.int64), n)
    rnd = rng.random(n) < 0.3
    ln[rnd] = rng.integers(0, 20001, int(rnd.sum()))
    ln[rng.integers(0, n, 3)] = 16777183
    ln[-1] = (16777183, W + 1, 0)[n % 3]                                      # what the terminator thread sits next to
    return ln.astype(np.uint32)


@pytest.mark.parametrize("WS", [(32, 1), (1000, 500), (150, 149)])
@pytest.mark.parametrize("n_reads", [255, 256, 257, 65537, 1 << 21])
def test_plan_at_batch_size(torch_cuda, n_reads, WS):
    """tile_first of 255 .. 2^21 queries == numpy's cumulative sum.  Catches: the terminator entry tcnt[n_reads] not written when it falls
    into a block of its own (n_reads % 256 == 0: `i >= n_reads` for `i > n_reads`, or a grid of n_reads / 256 blocks) -- the scan then adds
    whatever the workspace held; a 32-bit tile count or running sum (at (32, 1) one query has 2^24 - 64 tiles and 2^21 of them pass 2^32); a
    count that is wrong at L = 0, W - 1, W, W + 1 or W + S; a scan that is wrong from its second block on."""
    W, S = WS
    db, tree = vote_tree()
    ln = plan_lengths(n_reads, W, S)
    first = tiles_ref.plan_np(ln, W, S)
    assert n_reads < (1 << 21) or W != 32 or int(first[-1]) > 1 << 32
    tile_first, meta = tree.tiles_plan(dev(torch_cuda, ln), W, S)
    assert meta == dict(total_tiles=int(first[-1]), total_bases=0, max_len=0, error=0)
    assert np.array_equal(tile_first.cpu().numpy().view(np.uint64), first)


def test_views_of_a_batch_of_more_than_2_32_tiles(torch_cuda):
    """512 queries of 16 777 183 bases among 3 000 of one tile, (32, 1): 2^33 - 29 768 tiles.  Catches: `g`, `first_tile` or the `total` of the
    range check held in 32 bits (the 1 000 tiles around 2^32 then come from the batch's first queries, or the range is refused), a binary
    search that compares 32-bit halves, `t` or the offset truncated, meta.total_tiles cut to 32 bits."""
    torch = torch_cuda
    db, tree = vote_tree()
    W, S = 32, 1
    off, ln = giant_batch()
    first = tiles_ref.plan_np(ln, W, S)
    total = int(first[-1])
    assert total > 1 << 32 and int(off[-1]) > 1 << 32
    d_off, d_ln = dev(torch, off), dev(torch, ln)
    tile_first, meta = tree.tiles_plan(d_ln, W, S)
    assert meta["total_tiles"] == total and np.array_equal(tile_first.cpu().numpy().view(np.uint64), first)
    last_giant = int(first[-4])                                                       # the tiles in front of the three queries behind the last giant
    for f0, n in (((1 << 32) - 500, 1000), (last_giant - (1 << 23), 4096), (last_giant - 100, 103), (total - 7, 7), (total, 0)):
        want = tiles_ref.views_range(off, ln, W, S, f0, n, first)
        got = tree.tiles_views(d_off, d_ln, W, S, tile_first, f0, n)
        assert got[4] == meta_of(total, want[1]), (f0, n)
        assert_views(got, want, (f0, n))
    got = tree.tiles_views(d_off, d_ln, W, S, tile_first, total - 1, 2)
    assert got[4] == dict(total_tiles=total, total_bases=0, max_len=0, error=1)


RANGE_W, RANGE_S, RANGE_ONES = 1000, 7, 6000


def range_batch():
    """6 000 queries of one tile, one of 2^21 tiles, 4 000 of no bases, 300 of one tile: 2^21 + 10 300 tiles at (1000, 7)"""
    rng = np.random.default_rng(21)
    big = RANGE_W + RANGE_S * ((1 << 21) - 1)
    ln = np.concatenate([rng.integers(0, RANGE_W + 1, RANGE_ONES), [big], np.zeros(4000, dtype=np.int64), rng.integers(1, RANGE_W + 1, 300)]).astype(np.uint32)
    off = np.zeros(len(ln), dtype=np.uint64)
    np.cumsum(ln[:-1].astype(np.uint64) + np.uint64(1), out=off[1:])
    return off, ln


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, (1 << 21) - 1, 1 << 21, "empty tiles"])
def test_ranges_of_every_size(torch_cuda, n):
    """A range that starts among thousands of one-tile queries and runs into the query of 2^21 tiles; total_bases and max_len == numpy's.
    Catches: the block sum starting at wave 2 (n = 65 .. 257: the second wave's tiles are missing from total_bases), `j <= n` or a grid one
    block short at n % 256 == 0 and n % 64 == 0, lanes beyond n adding to the sum or the maximum, `<` for `<=` in the binary search (every
    first tile of a query is then given to the query in front: 300 of them in each range), an atomic lost among 8 192 blocks, a 32-bit
    total_bases (2^21 tiles of 1 000 bases).  "empty tiles": 3 000 tiles of no bases -- no block adds anything, and meta must be zero but
    for total_tiles, which is what a kernel that leaves meta to its atomics gets wrong."""
    torch = torch_cuda
    db, tree = vote_tree()
    W, S = RANGE_W, RANGE_S
    off, ln = range_batch()
    first = tiles_ref.plan_np(ln, W, S)
    total = int(first[-1])
    assert total == (1 << 21) + 10300
    f0, n = (RANGE_ONES + (1 << 21) + 100, 3000) if n == "empty tiles" else (RANGE_ONES - min(n // 2, 300), n)
    d_off, d_ln = dev(torch, off), dev(torch, ln)
    tile_first, meta = tree.tiles_plan(d_ln, W, S)
    want = tiles_ref.views_range(off, ln, W, S, f0, n, first)
    got = tree.tiles_views(d_off, d_ln, W, S, tile_first, f0, n)
    assert got[4] == meta_of(total, want[1]), (f0, n)
    if f0 > RANGE_ONES:
        assert got[4] == dict(total_tiles=total, total_bases=0, max_len=0, error=0) and int(want[3].max()) == 0
    elif n > 1:
        assert int(want[2][0]) < RANGE_ONES == int(want[2][-1]) and got[4]["max_len"] == W
    assert_views(got, want, (f0, n))


def test_nothing_is_kept_between_calls(torch_cuda):
    """d_meta arrives full of 0xFF; two utree_tiles_views calls of different ranges and outputs are in flight on one non-default stream; the
    plan's workspace lies 1 and 255 bytes off its alignment with exactly utree_tiles_workspace_bytes behind it.  Catches: a views kernel
    that adds to what meta held (no memset, or a memset on another stream), state in the handle that the second call overwrites while the
    first runs, a plan that writes behind its workspace's end or assumes an aligned pointer; and a size check that lets a workspace one
    byte short pass when the pointer happens to leave slack."""
    torch = torch_cuda
    db, tree = vote_tree()
    L = lib.load()
    W, S = RANGE_W, RANGE_S
    off, ln = range_batch()
    first = tiles_ref.plan_np(ln, W, S)
    total = int(first[-1])
    d_off, d_ln = dev(torch, off), dev(torch, ln)
    n_reads = len(ln)
    need = L.utree_tiles_workspace_bytes(tree._h, n_reads)
    ws = torch.zeros(need + 512, dtype=torch.uint8, device="cuda:0")
    base = ws.data_ptr() + (-ws.data_ptr() % 256)
    st = torch.cuda.Stream()
    plans = []
    for shift in (1, 255):
        ws.fill_(0xA5)
        tf = torch.full((n_reads + 1,), -1, dtype=torch.int64, device="cuda:0")
        d_meta = torch.full((3,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        assert L.utree_tiles_plan(tree._h, d_ln.data_ptr(), n_reads, W, S, tf.data_ptr(), d_meta.data_ptr(), base + shift, need - 1, st.cuda_stream) == lib.E_ARG
        lib.check(L.utree_tiles_plan(tree._h, d_ln.data_ptr(), n_reads, W, S, tf.data_ptr(), d_meta.data_ptr(), base + shift, need, st.cuda_stream), "utree_tiles_plan")
        st.synchronize()
        m = lib.TilesMeta.from_buffer_copy(d_meta.cpu().numpy().tobytes())
        assert (m.total_tiles, m.total_bases, m.max_len, m.error) == (total, 0, 0, 0)
        assert np.array_equal(tf.cpu().numpy().view(np.uint64), first)
        h = ws.cpu().numpy()
        at = base - ws.data_ptr() + shift
        assert bool((h[:at] == 0xA5).all()) and bool((h[at + need:] == 0xA5).all())       # nothing in front of the pointer, nothing behind its bytes
        plans.append(tf)
    ranges = ((RANGE_ONES - 300, 70000), (RANGE_ONES + (1 << 21) - 5, 4200))
    outs = []
    for f0, n in ranges:
        outs.append([torch.full((n,), -7, dtype=dt, device="cuda:0") for dt in (torch.int64, torch.int32, torch.int32, torch.int32)] +
                    [torch.full((3,), -1, dtype=torch.int64, device="cuda:0")])
    torch.cuda.synchronize()
    for (f0, n), o, tf in zip(ranges, outs, plans):
        lib.check(L.utree_tiles_views(tree._h, d_off.data_ptr(), d_ln.data_ptr(), n_reads, W, S, tf.data_ptr(), f0, n, o[0].data_ptr(), o[1].data_ptr(),
                                      o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), st.cuda_stream), "utree_tiles_views")
    st.synchronize()
    for (f0, n), o in zip(ranges, outs):
        want = tiles_ref.views_range(off, ln, W, S, f0, n, first)
        m = lib.TilesMeta.from_buffer_copy(o[4].cpu().numpy().tobytes())
        assert dict(total_tiles=int(m.total_tiles), total_bases=int(m.total_bases), max_len=int(m.max_len), error=int(m.error)) == meta_of(total, want[1])
        assert_views(o, want, (f0, n))


# ---- B. tiles through every classify pass -------------------------------------------------------------------------------------------------

def pass_cases():
    k = 32                                                                            # (asserted against the database in the test)
    cap3, cap4, both = tiles_ref.lanes_cap(k, 3), tiles_ref.lanes_cap(k, 4), tiles_ref.pieces_min_rc()
    out = []
    for W, S, rcs in (((1000, 500, (False, True)), (cap3, cap3 // 2, (False, True)), (cap3 + 1, (cap3 + 1) // 2, (False, True)), (both, both // 2, (True,)),
                       (both + 1, (both + 1) // 2, (True,)), (cap4, 1000, (False,)), (cap4 + 1, 1000, (False,)), (20000, 7001, (False, True)))):
        out += [(W, S, rc, None, "1") for rc in rcs]
    out.append((tiles_ref.LANES_CAP + 1, 1, False, 4, "1"))
    out += [(W, 500 if W == 1000 else 1000, rc, None, "0") for W in (1000, tiles_ref.MID_CAP + 1) for rc in (False, True)]
    return out


_DEVICE = {}


def pass_queries(torch):
    if "pass" not in _DEVICE:
        recs, buf, names, off, ln = contig_set("pass")
        _DEVICE["pass"] = (torch.from_numpy(buf.copy()).cuda(), dev(torch, off), dev(torch, ln))
    return _DEVICE["pass"]


@pytest.mark.parametrize("W,S,rc,only,lane_pass", pass_cases(), ids=lambda v: str(v))
def test_tiles_through_every_classify_pass(torch_cuda, monkeypatch, W, S, rc, only, lane_pass):
    """Contigs of 120 000, 1, 2 095, 2 096 and 40 000 bases: every batch holds tiles of ONE length above UTREE_LANES_CAP that overlap in
    d_bases, and each query's shorter last tile.  The records == the oracle's on the same views, and == the records of the same tiles
    gathered into a buffer of their own.  The first catches a kernel that disagrees with the oracle at this width: a lane class chosen with
    `<` at its cap (1063 | 1064, 2095 | 2096), a read of 1 056 bases with both strands staged into 2 112 bytes, a pieces pass whose
    n_long_cap or n_pieces_cap -- carved from total_bases = W/S times the buffer -- is short (poll() raises) or whose pieces of
    neighbouring tiles mix.  The second catches a kernel for which a view is not a read like any other: one that reads past a tile's end
    into the next tile's bases, aligns an offset down (at (161, 1) every offset mod 16 occurs), or caches by buffer position.  The last
    line catches one that writes d_bases."""
    torch = torch_cuda
    db, tree = vote_tree()
    assert tree.info.bucket_bytes == 64 and tree.info.lane_pass == 1 and db.k == 32
    recs, buf, names, off, ln = contig_set("pass")
    bases, d_off, d_ln = pass_queries(torch)
    w_toff, w_tlen, w_tq, w_ti, w_res = views_ref("pass", W, S, rc, only)
    first = tiles_ref.plan_np(ln, W, S)
    f0, n = (0, int(first[-1])) if only is None else (int(first[only]), int(first[only + 1] - first[only]))
    tile_first, meta = tree.tiles_plan(d_ln, W, S)
    assert meta["total_tiles"] == int(first[-1])
    toff, tlen, tq, ti, m = tree.tiles_views(d_off, d_ln, W, S, tile_first, f0, n)
    assert m == meta_of(int(first[-1]), w_tlen) and m["max_len"] == W
    assert_views((toff, tlen, tq, ti), (w_toff, w_tlen, w_tq, w_ti), (W, S))
    monkeypatch.setenv("UTREE_LANE_PASS", lane_pass)
    res = tree.classify(bases, toff, tlen, rc=rc, total_bases=m["total_bases"], max_len=m["max_len"])
    torch.cuda.synchronize()
    tree.poll()
    name = tree.kernel_name()
    pieces = (2 * W + 1 if rc else W) > tiles_ref.MID_CAP or W > tiles_ref.lanes_cap(db.k, 4)
    if lane_pass == "1":
        assert name.startswith("classify_lanes_k<8, 2, 16," if pieces else "classify_lanes_mixed_k<"), name
    else:
        assert ("classify_long_k" if pieces else "classify_short_k") in name, name
    assert int((w_res["found"] > 0).sum()) >= n - 3                                   # the tiles do hit (the one-base contig's cannot)
    assert_records(res.cpu().numpy(), w_res, (W, S, rc, "views against the oracle"))
    # the same tiles as reads of their own: contiguous, own offsets
    own_off = np.zeros(n, dtype=np.uint64)
    np.cumsum(w_tlen[:-1].astype(np.uint64), out=own_off[1:])
    idx = np.repeat(w_toff.astype(np.int64) - own_off.astype(np.int64), w_tlen.astype(np.int64)) + np.arange(int(m["total_bases"]), dtype=np.int64)
    own = torch.from_numpy(buf[idx]).cuda()
    res2 = tree.classify(own, dev(torch, own_off), tlen, rc=rc, total_bases=m["total_bases"], max_len=m["max_len"])
    torch.cuda.synchronize()
    tree.poll()
    assert tree.kernel_name() == name
    assert torch.equal(res, res2), (W, S, rc, "views against the gathered tiles")
    assert bases.cpu().numpy().tobytes() == buf.tobytes()


# ---- C. the file run at real sub-batch sizes ------------------------------------------------------------------------------------------------

STDOUT = re.compile(rb"^Queries: (\d+), tiles (\d+), classified (\d+), segments (\d+)$", re.M)
BATCHES = re.compile(rb"(\d+) batches\n")


def written(tmp_path, key):
    p = tmp_path / (key + ".fa")
    if not p.exists():
        p.write_bytes(tiles_ref.fasta(contig_set(key)[0]))
    return p


def cli(tmp_path, src, W, S, rc, env):
    t, s = tmp_path / "tiles.tsv", tmp_path / "segments.tsv"
    e = {k: v for k, v in os.environ.items() if k not in ("UTREE_TILES_BATCH", "UTREE_CHUNK_BYTES")}
    e.update(UTREE_TILE_BP=str(W), UTREE_TILE_STEP=str(S))
    e.update(env)
    r = subprocess.run([lib.TILES_CLI_PATH, util.fixture_ctr("vote"), str(src), str(t), str(s)] + (["RC"] if rc else []), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=e, timeout=120)
    return r, t, s


@pytest.mark.parametrize("batch,rc", [("4096", False), ("5000", True), (None, False)])
def test_file_run_with_team_formatted_sub_batches(torch_cuda, tmp_path, batch, rc):
    """23 221 tiles at (64, 4), one contig's name 300 bytes long: tiles.tsv is 6 MB.  Sub-batches of 4 096 and more are formatted by the
    team.  Catches: slices that overlap or leave a gap (n * k / tm in 32 bits is still right here; an inclusive end or k / tm first is
    not), slices written in the order the threads finish, a thread's buffer reused before it is written, the counts of the slices not
    summed, and the run that a sub-batch leaves open -- classified, tests/test_tiles_scale_cpu.py -- closed at the sub-batch's end or
    dropped."""
    W, S = tiles_ref.FILE_WS
    text, seg, lines, nseg = files_ref("file", W, S, rc)
    r, t, s = cli(tmp_path, written(tmp_path, "file"), W, S, rc, dict(UTREE_TILES_BATCH=batch) if batch else {})
    assert r.returncode == 0, r.stderr[-400:]
    assert t.read_bytes() == text and s.read_bytes() == seg
    assert [int(x) for x in STDOUT.search(r.stdout).groups()] == [3, 23221, lines, nseg]
    assert int(BATCHES.search(r.stderr).group(1)) == -(-23221 // int(batch or lib.TILES_MAX_BATCH))


@pytest.mark.parametrize("threads,batch,rc", [(1, None, True), (3, None, False), (16, None, True), (64, None, False), (3, "5000", True)])
def test_file_run_through_the_binding_with_every_team(torch_cuda, tmp_path, monkeypatch, threads, batch, rc):
    """threads = 1 and the batch unset: ONE slice of 6 MB, so format_slice's buffer doubles from 1 MiB three times; a team of 3 (slices that
    are no multiple of anything), of 16 and of 64, which is cut to 16.  Catches: a buffer that is grown but whose old pointer is written,
    text lost when the first attempt runs out of room, lines[k] counted once per attempt, a team larger than the buffers there are."""
    W, S = tiles_ref.FILE_WS
    db, tree = vote_tree()
    text, seg, lines, nseg = files_ref("file", W, S, rc)
    assert len(text) > (4 << 20)
    monkeypatch.delenv("UTREE_CHUNK_BYTES", raising=False)
    if batch:
        monkeypatch.setenv("UTREE_TILES_BATCH", batch)
    else:
        monkeypatch.delenv("UTREE_TILES_BATCH", raising=False)
    t, s = tmp_path / "t.tsv", tmp_path / "s.tsv"
    code, st = tiles_file(db, tree, str(written(tmp_path, "file")), str(t), str(s), tile_bp=W, step_bp=S, rc=rc, threads=threads)
    assert code == lib.OK
    assert t.read_bytes() == text and s.read_bytes() == seg
    assert (st.n_queries, st.n_tiles, st.classified, st.segments) == (3, 23221, lines, nseg)
    assert st.n_batches == -(-23221 // int(batch or lib.TILES_MAX_BATCH))


def test_file_run_split_at_the_default_2_21_tiles(torch_cuda, tmp_path, monkeypatch):
    """One contig of 2^21 + 5 000 tiles at (32, 1), random but for three fixture reads, UTREE_TILES_BATCH unset: two sub-batches, the first
    of exactly 2^21 tiles.  The vote database has no two k-mers 31 bases apart, so at S = 1 the run that the split cuts is the
    unclassified one between two k-mers of the island laid across tile 2^21 (32 tiles; tests/test_tiles_scale_cpu.py): it must be ONE
    line.  Catches: a second sub-batch that starts at `batch` instead of `first + batch`, its views taken from tile 0, the open run closed
    or lost at the split, `first + n >= total` wrong at the last sub-batch (the run that ends the contig is then never written)."""
    W, S = tiles_ref.SPLIT_WS
    db, tree = vote_tree()
    text, seg, lines, nseg = files_ref("split", W, S, False)
    monkeypatch.delenv("UTREE_TILES_BATCH", raising=False)
    monkeypatch.delenv("UTREE_CHUNK_BYTES", raising=False)
    t, s = tmp_path / "t.tsv", tmp_path / "s.tsv"
    code, st = tiles_file(db, tree, str(written(tmp_path, "split")), str(t), str(s), tile_bp=W, step_bp=S, rc=False)
    assert code == lib.OK and st.n_batches == 2
    assert (st.n_queries, st.n_tiles, st.classified, st.segments) == (1, tiles_ref.SPLIT_TILES, lines, nseg)
    assert t.read_bytes() == text and s.read_bytes() == seg


@pytest.mark.parametrize("chunk", ["4000", "1000"])
def test_framing_error_behind_the_first_chunk(torch_cuda, tmp_path, monkeypatch, chunk):
    """The committed vote contigs with the '>' of record 9 broken.  With chunks of 4 000 bytes records 1 to 10 are framed together; with
    1 000 the first chunk ends inside record 8 and the broken record is the second of the second chunk
    (tests/test_tiles_scale_cpu.py).  The message carries the reference's index for this file (tiles_manifest.json: [L 9]).  Catches:
    read_index reported as the framing counts it, from the chunk's first record ([L 2] with 1 000); the tiles of the second chunk's good
    record, or its open run, lost when the error ends the run."""
    m = tiles_ref.manifest()["scale"]["framing"]
    W, S = tiles_ref.PARAMS["vote"]
    recs, tl = ref("vote", False)
    bad = tiles_ref.broken_header(tiles_ref.contigs("vote"), m["record"])
    src = tmp_path / "broken.fa"
    src.write_bytes(bad)
    front = [x for x in tl if x.q < m["record"] - 1]
    r, t, s = cli(tmp_path, src, W, S, False, dict(UTREE_CHUNK_BYTES=chunk))
    assert r.returncode == m["exit"] == 2 and (m["message"] + "\n").encode() in r.stderr, r.stderr[-400:]
    assert t.read_bytes() == tiles_ref.tiles_tsv(front) and s.read_bytes() == tiles_ref.segments_tsv(recs, front)
    assert [int(x) for x in STDOUT.search(r.stdout).groups()] == [8, len(front), sum(1 for x in front if x.line), tiles_ref.segments_tsv(recs, front).count(b"\n")]
    # the same through the binding: the index itself, and the chunks the run took
    db, tree = vote_tree()
    monkeypatch.setenv("UTREE_CHUNK_BYTES", chunk)
    monkeypatch.delenv("UTREE_TILES_BATCH", raising=False)
    code, st = tiles_file(db, tree, str(src), str(tmp_path / "t2.tsv"), str(tmp_path / "s2.tsv"), tile_bp=W, step_bp=S, rc=False)
    assert code == lib.E_FASTA and (st.fasta_error.code, st.fasta_error.read_index) == (2, m["index"])
    assert (st.n_queries, st.n_tiles, st.n_batches) == (8, len(front), 1 if chunk == "4000" else 2)
    assert (tmp_path / "t2.tsv").read_bytes() == tiles_ref.tiles_tsv(front)
