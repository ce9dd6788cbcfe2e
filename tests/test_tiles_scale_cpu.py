"""CPU-only: the references that tests/test_gpu_tiles_scale.py compares the device with are themselves held here.

  views_range          == numpy_views, tile for tile, for every W and S up to 12 and lengths 0 to 40; and past 2^32 == Python integers
  classify_views       == classify (tile by tile through classify_read) on the committed fixtures, records, lines and segments
  view_files           over classify_views hashes to what the genuine reference wrote for the pre-split FASTA of the generated contigs at
                       (1000, 500), (2096, 1000), (20000, 7001) and (64, 4) (tests/golden/make_golden_tiles.py: scale; hashes and counts in
                       tiles_manifest.json -- the contigs are generated again here and must hash to the recorded ones)
  the inputs           have the shapes the GPU tests rely on: a classified run across a sub-batch boundary of 4096 and of 5000 tiles, all but
                       a few thousand of 2^21 + 5000 tiles unclassified and one run across tile 2^21, record 9 in a later chunk of 1000 bytes

The module also keeps what both files need, computed once: the contig sets, their views and the oracle's records."""
import numpy as np
import pytest

import tiles_ref
import util
from oracle import orc
from test_tiles_cpu import ref

_O, _SETS, _VIEWS, _FILES = [], {}, {}, {}


def oracle():
    if not _O:
        _O.append(orc.OracleDB.load(util.fixture_ctr("vote")))
    return _O[0]


def contig_set(key):
    """(recs, FASTA bytes as uint8, names, seq_off, seq_len) of "pass", "file" or "split": generated once, never changed"""
    if key not in _SETS:
        recs = {"pass": tiles_ref.pass_contigs, "file": tiles_ref.file_contigs, "split": tiles_ref.split_contig}[key]()
        buf, names, off, ln = tiles_ref.framed_arrays(recs)
        buf.flags.writeable = False
        _SETS[key] = (recs, buf, names, off, ln)
    return _SETS[key]


def views_ref(key, W, S, rc, only=None):
    """(toff, tlen, tquery, tindex, records) of all tiles of a set (only: of that one contig), the oracle's records on the views"""
    k = (key, W, S, rc, only)
    if k not in _VIEWS:
        recs, buf, names, off, ln = contig_set(key)
        first = tiles_ref.plan_np(ln, W, S)
        f0, n = (0, int(first[-1])) if only is None else (int(first[only]), int(first[only + 1] - first[only]))
        v = tiles_ref.views_range(off, ln, W, S, f0, n, first)
        _VIEWS[k] = v + (tiles_ref.classify_views(oracle(), buf, v[0], v[1], rc),)
    return _VIEWS[k]


def files_ref(key, W, S, rc):
    """(tiles.tsv, segments.tsv, lines, segments) of a set: the restatement over classify_views"""
    k = (key, W, S, rc)
    if k not in _FILES:
        recs, buf, names, off, ln = contig_set(key)
        toff, tlen, tq, ti, res = views_ref(key, W, S, rc)
        _FILES[k] = tiles_ref.view_files(oracle(), names, ln, W, S, tq, ti, res)
    return _FILES[k]


# ---- views_range ------------------------------------------------------------------------------------------------------------------------

def test_views_range_equals_numpy_views():
    """every W and S up to 12, lengths 0 to 40 (0: one tile of length 0), the whole batch and ranges that begin and end inside queries"""
    rng = np.random.default_rng(7)
    ln = np.concatenate([np.arange(41), rng.integers(0, 41, 30)]).astype(np.uint32)
    ln = ln[rng.permutation(len(ln))]
    off = (np.cumsum(ln.astype(np.uint64) + np.uint64(3)) + np.uint64(1000)).astype(np.uint64)
    for W in range(1, 13):
        for S in range(1, W + 1):
            first, toff, tlen, tq, ti = tiles_ref.numpy_views(off, ln, W, S)
            total = int(first[-1])
            assert np.array_equal(tiles_ref.plan_np(ln, W, S), first)
            assert int(tlen[ln[tq] == 0].sum()) == 0 and int((ln == 0).sum()) == int(((ln[tq] == 0) & (ti == 0)).sum())
            for f0, n in [(0, total), (0, 0), (total, 0), (total - 1, 1)] + [(int(a), int(rng.integers(0, total - a + 1))) for a in rng.integers(0, total, 6)]:
                got = tiles_ref.views_range(off, ln, W, S, f0, n)
                for g, w in zip(got, (toff, tlen, tq, ti)):
                    assert g.dtype == w.dtype and np.array_equal(g, w[f0:f0 + n]), (W, S, f0, n)


def giant_batch():
    """(off, ln) of test A's batch whose tiles pass 2^32 at (32, 1): 512 queries of 16 777 183 bases -- 2^24 - 64 tiles each -- among 3 000 of
    one tile (0 to 32 bases): 300, 256 giants, 1 000, 255 giants, 1 697, the last giant, 3.  Tile 2^32 lies inside giant 257 (3 000 queries
    of one tile cannot fill the 16 384 tiles that 256 giants leave below 2^32)."""
    rng = np.random.default_rng(33)
    G = 16777183
    small = lambda n: rng.integers(0, 33, n)
    ln = np.concatenate([small(300), np.full(256, G), small(1000), np.full(255, G), small(1697), [G], small(3)]).astype(np.uint32)
    off = np.zeros(len(ln), dtype=np.uint64)
    np.cumsum(ln[:-1].astype(np.uint64) + np.uint64(1), out=off[1:])
    return off + np.uint64(12), ln


def test_views_range_past_2_32_equals_python_integers():
    off, ln = giant_batch()
    W, S = 32, 1
    cnt = [tiles_ref.n_tiles(int(L), W, S) for L in ln]
    first = [0]
    for c in cnt:
        first.append(first[-1] + c)
    total = first[-1]
    assert total == 512 * ((1 << 24) - 64) + 3000 > 1 << 32 and [int(x) for x in tiles_ref.plan_np(ln, W, S)] == first
    import bisect
    for f0, n in (((1 << 32) - 500, 1000), (total - 7, 7), (first[-4] - 100, 103), (0, 400)):
        toff, tlen, tq, ti = tiles_ref.views_range(off, ln, W, S, f0, n)
        assert (len({int(q) for q in tq}) > 1) == (f0 != (1 << 32) - 500)                 # all but the one inside giant 257 cross queries
        for j in range(n):
            g = f0 + j
            q = bisect.bisect_right(first, g) - 1
            t = g - first[q]
            assert (int(toff[j]), int(tlen[j]), int(tq[j]), int(ti[j])) == (int(off[q]) + t * S, min(int(ln[q]) - t * S, W), q, t)
    assert int(tiles_ref.views_range(off, ln, W, S, (1 << 32) - 500, 1000)[0].max()) > 1 << 32      # offsets past 2^32 too


# ---- classify_views against classify ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rc", (False, True))
@pytest.mark.parametrize("name", tiles_ref.FIXTURES)
def test_classify_views_equals_classify_tile_by_tile(name, rc):
    """the oracle on overlapping views of one buffer == the oracle on every tile cut out as a read of its own: records, lines, segments"""
    recs, tl = ref(name, rc)
    W, S = tiles_ref.PARAMS[name]
    o = orc.OracleDB.load(util.fixture_ctr(name))
    buf, names, off, ln = tiles_ref.framed_arrays(recs)
    assert names == [n for n, _ in recs]
    toff, tlen, tq, ti = tiles_ref.views_range(off, ln, W, S, 0, len(tl))
    res = tiles_ref.classify_views(o, buf, toff, tlen, rc)
    want = tiles_ref.results_array(tl)
    for f in want.dtype.names:
        assert np.array_equal(res[f], want[f]), f
    vt = tiles_ref.view_tiles(o, names, ln, W, S, tq, ti, res)
    assert [(x.q, x.t, x.a, x.b, x.line, x.taxon) for x in vt] == [(x.q, x.t, x.a, x.b, x.line, x.taxon) for x in tl]
    text, seg, lines, nseg = tiles_ref.view_files(o, names, ln, W, S, tq, ti, res)
    assert text == tiles_ref.tiles_tsv(tl) == tiles_ref.golden(name, rc) and lines == text.count(b"\n")
    assert seg == tiles_ref.segments_tsv(recs, tl) and nseg == seg.count(b"\n")


# ---- the generated contigs against the genuine reference ------------------------------------------------------------------------------------

def test_the_generated_contigs_are_the_recorded_ones():
    m = tiles_ref.manifest()["scale"]
    for key, lengths in (("pass", tiles_ref.PASS_LENGTHS), ("file", tiles_ref.FILE_LENGTHS)):
        recs = contig_set(key)[0]
        assert [len(s) for _, s in recs] == lengths == m[key]["lengths"]
        assert tiles_ref.sha256(tiles_ref.fasta(recs)) == m[key]["contigs_sha256"]
    assert len(contig_set("file")[0][0][0]) == 300
    k = oracle().k
    assert {p: [r["W"], r["S"]] for p, r in m["pass"]["runs"].items()} == {p: list(ws) for p, ws in tiles_ref.pass_params(k).items()}
    assert [m["file"]["runs"]["file"][x] for x in ("W", "S")] == list(tiles_ref.FILE_WS)
    assert tiles_ref.pass_params(k)["pieces"][0] == 2096 and tiles_ref.lanes_cap(k, 3) == 1063 and tiles_ref.pieces_min_rc() == 1055


SCALE_RUNS = [("pass", "default"), ("pass", "pieces"), ("pass", "wide"), ("file", "file")]


@pytest.mark.parametrize("rc", (False, True))
@pytest.mark.parametrize("key,run", SCALE_RUNS)
def test_the_restatement_over_views_hashes_to_the_reference(key, run, rc):
    """view_files over classify_views == the bytes xtree-searchGG wrote for the pre-split FASTA; "Searched" and "Good finds" are its own"""
    m = tiles_ref.manifest()["scale"][key]["runs"][run]
    W, S = m["W"], m["S"]
    recs, buf, names, off, ln = contig_set(key)
    tag = "_rc" if rc else ""
    text, seg, lines, nseg = files_ref(key, W, S, rc)
    assert tiles_ref.sha256(text) == m["out%s_sha256" % tag]
    assert len(views_ref(key, W, S, rc)[4]) == m["tiles"] == m["searched" + tag] and lines == m["good_finds" + tag] and nseg == m["segments" + tag]
    if run != "file":
        assert tiles_ref.sha256(tiles_ref.fasta(tiles_ref.split_records(recs, W, S))) == m["split_sha256"]


# ---- the shapes the GPU tests rely on -----------------------------------------------------------------------------------------------------

def runs_of(seg):
    """[(query name, first base, last base, tiles, class)] of a segments.tsv"""
    return [(r[0], int(r[1]), int(r[2]), int(r[3]), r[4]) for r in (l.split(b"\t") for l in seg.split(b"\n")[:-1])]


def test_a_classified_run_straddles_the_team_formatted_sub_batches():
    """at (64, 4) a k-mer lies in about eight tiles in a row: with UTREE_TILES_BATCH = 4096 and with 5000, at least one sub-batch of the
    file set ends inside a classified run (and at least one inside an unclassified one), which the next sub-batch has to continue"""
    W, S = tiles_ref.FILE_WS
    for rc in (False, True):
        text, seg, lines, nseg = files_ref("file", W, S, rc)
        assert len(text) > (4 << 20)                                                     # one thread's buffer of 1 MiB has to grow twice
        at, inside = 0, set()
        for name, a, b, n, c in runs_of(seg):
            for batch in (4096, 5000):
                if any(at < edge < at + n for edge in range(batch, 23221, batch)):
                    inside.add((batch, c))
            at += n
        assert at == 23221 and {(4096, b"C"), (5000, b"C")} <= inside, inside


def test_the_split_contig_is_unclassified_but_for_its_islands():
    """2^21 + 5000 tiles at (32, 1), of which the oracle classifies a few dozen: Python formats only those.  The vote database holds no two
    k-mers that overlap by 31 bases, so no two tiles in a row are classified at S = 1: the run that the default split of 2^21 tiles cuts is
    the unclassified one between two k-mers of the island laid across it, 32 tiles from 2^21 - 6 on."""
    W, S = tiles_ref.SPLIT_WS
    recs, buf, names, off, ln = contig_set("split")
    toff, tlen, tq, ti, res = views_ref("split", W, S, False)
    assert len(res) == tiles_ref.SPLIT_TILES == (1 << 21) + 5000 and len(recs) == 1
    hit = np.flatnonzero(res["found"] > 0)
    assert 10 <= len(hit) < 5000
    assert hit[0] == 0 and hit[-1] == len(res) - 1                                        # islands at the very start and the very end
    before, after = hit[hit < (1 << 21)].max(), hit[hit >= (1 << 21)].min()
    assert (1 << 21) - 40 <= before < (1 << 21) - 1 and (1 << 21) < after <= (1 << 21) + 40
    text, seg, lines, nseg = files_ref("split", W, S, False)
    assert lines == len(hit)
    cut = [r for r in runs_of(seg) if r[1] - 1 <= (1 << 21) < r[1] - 1 + r[3]]            # (S = 1: tile t starts at base t + 1)
    assert cut == [(names[0], int(before) + 2, int(after) + 31, int(after - before - 1), b"U")]


def test_record_9_lies_in_a_later_chunk_of_1000_bytes():
    """With 4000-byte chunks the first chunk of the committed vote contigs holds records 1 to 10; with 1000-byte chunks it ends inside
    record 8, so the broken record 9 is the second one framed in the second chunk.  The reference's index for the file is the manifest's."""
    m = tiles_ref.manifest()["scale"]["framing"]
    data = tiles_ref.contigs("vote")
    bad = tiles_ref.broken_header(data, tiles_ref.FRAMING_RECORD)
    assert tiles_ref.sha256(bad) == m["input_sha256"] and (m["record"], m["index"], m["exit"]) == (9, 9, 2)
    assert m["message"] == "ERROR: no header '>' [L 9]"
    starts = [i for i in range(len(data)) if data[i:i + 1] == b">"]
    assert len(starts) == 11 and starts[10] < 4000                                        # records 1 .. 10 begin (and end) within 4000 bytes
    assert starts[7] < 1000 < starts[8]                                                   # 1000 bytes end inside record 8
    assert starts[9] - starts[7] < 1000                                                   # records 8 and 9 are in the second chunk
