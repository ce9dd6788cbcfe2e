"""GPU tests of utree_search_run (include/utree_amd.h): every older entry point is a fixed-argument form of it, so the same small search
through either writes the same bytes; and the host pipeline's one shard path (csrc/search.c: stage, then run) at its edges -- an empty, a full
and a half second shard, single reads and pairs, with the reports that ride the uploaded span; and a slot formatted in three pieces across a shard edge.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree
from profile_ref import fasta_names
import pairs_ref
import samples_ref as sr
import util

T = 4                                                    # host threads
REPORTS = ("profile_path", "coverage_path", "redistribute_path", "hitmap_path", "samples_path", "sample_redistribute_path")


@pytest.fixture(scope="module")
def toy():
    """the toy database on two handles of one card (the second a copy of the first's image), and the inputs, their reads named
    <sample>_<n>: single reads and the pairs made of them, with the genuine reference's output under those names"""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    db = CtrDB.open(util.fixture_ctr("toy"))
    tree = DeviceTree.upload(db, 0)
    ptr, used = tree.image_ptr()

    class _Raw:
        __cuda_array_interface__ = {"shape": (used,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    c = torch.empty(used + 4096, dtype=torch.uint8, device="cuda:0")[4096:]
    c.copy_(torch.as_tensor(_Raw(), device="cuda:0"))
    torch.cuda.synchronize()
    second = DeviceTree.attach(db, c, 0)
    data = util.fixture_bytes("toy_reads.fa.gz")
    old = fasta_names(data)
    new = sr.round_robin_names(len(old), sr.SEVEN)
    single, rank = {}, {}
    for rc, tag in ((0, ""), (1, "_rc")):
        reads, single[rc] = sr.rename_reads(data, util.fixture_bytes("toy_out%s.txt.gz" % tag), old, new)
        rank[rc] = sr.rename_reads(data, util.fixture_bytes("toy_rank%s.txt.gz" % tag), old, new)[1]
    P = pairs_ref.Pairs("toy")
    p_old, p_new = list(P.names1), sr.round_robin_names(P.n, sr.SEVEN)
    pairs = {rc: sr.rename_reads(b"".join(b">" + o + b"\n\n" for o in p_old), pairs_ref.golden("toy", rc), p_old, p_new)[1] for rc in (0, 1)}
    P.names1 = p_new
    yield {"db": db, "trees": [tree, second], "reads": reads, "P": P, "want_single": single, "want_pairs": pairs, "want_rank": rank}
    second.close()
    tree.close()


def write_inputs(toy, d, kind, n=None):
    """the reads (and mates) of `kind` in directory d, the first n records / pairs of them: (reads path, mates path or None, interleaved)"""
    P = toy["P"]
    rp, mp = d / "r.fa", d / "m.fa"
    if kind == "single":
        rp.write_bytes(toy["reads"] if n is None else b"".join(b">" + r for r in toy["reads"].split(b">")[1:n + 1]))
        return str(rp), None, 0
    if kind == "two":
        rp.write_bytes(P.reads_fasta(n)); mp.write_bytes(P.mates_fasta(n))
        return str(rp), str(mp), 0
    rp.write_bytes(P.interleaved_fasta(None if n is None else 2 * n))
    return str(rp), None, 1


def request(d, reads, mates, interleaved, rc, fmt=lib.INPUT_REFERENCE, reports=(), max_passes=0, delim=0, rank=None):
    """(SearchRequest, the files it writes) with the output and the named reports in directory d"""
    d.mkdir(exist_ok=True)
    files = {"out_path": d / "out.txt"}
    files.update({k: d / (k + ".txt") for k in reports})
    req = lib.SearchRequest(do_rc=rc, host_threads=T, input_format=fmt, reads_path=reads.encode(), mates_path=mates.encode() if mates else None,
                            interleaved=interleaved, max_passes=max_passes, sample_delim=delim, **{k: str(p).encode() for k, p in files.items()})
    if rank is not None:
        req.rank = C.pointer(rank)
    if "hitmap_path" in files:
        files["labels"] = d / "hitmap_path.txt.labels"
    return req, files


def run(toy, req, n_handles=1):
    arr = (C.c_void_p * n_handles)(*[t._h for t in toy["trees"][:n_handles]])
    st = lib.SearchStats()
    code = lib.load().utree_search_run(toy["db"]._h, arr, n_handles, C.byref(req), C.byref(st))
    assert code == lib.OK, lib.UtreeError(code, "utree_search_run")
    return st


def same_files(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].read_bytes() == b[k].read_bytes(), k
        assert k == "labels" or a[k].stat().st_size > 0, k


# ---- 1. old and new give the same bytes --------------------------------------------------------------------------------------------------
# legacy name -> (input kind, rc, input format, reports it can name, in its argument order); every GG entry point takes a prefix of
# [profile, coverage, redistribute, max_passes, hitmap, samples, delim, sample_redistribute]
GG = {
    "utree_search_file": ("single", 0, None, ()),
    "utree_search_file_opts": ("single", 1, lib.INPUT_FASTA_MULTILINE, ()),
    "utree_search_file_profile": ("single", 0, lib.INPUT_REFERENCE, REPORTS[:1]),
    "utree_search_file_coverage": ("single", 1, lib.INPUT_REFERENCE, REPORTS[:2]),
    "utree_search_pairs_file": ("two", 1, lib.INPUT_REFERENCE, REPORTS[:2]),
    "utree_search_file_redistribute": ("inter", 0, lib.INPUT_REFERENCE, REPORTS[:3]),
    "utree_search_file_hitmap": ("single", 1, lib.INPUT_AUTO, REPORTS[:4]),
    "utree_search_file_samples": ("single", 0, lib.INPUT_REFERENCE, REPORTS[:5]),
    "utree_search_file_sample_redistribute": ("two", 1, lib.INPUT_FASTA_MULTILINE, REPORTS[:6]),
}
PASSES = 7


@pytest.mark.parametrize("name", sorted(GG))
def test_gg_entry_point_and_its_request_write_the_same_bytes(toy, name, tmp_path):
    kind, rc, fmt, reports = GG[name]
    reads, mates, interleaved = write_inputs(toy, tmp_path, kind)
    passes = PASSES if "redistribute_path" in reports else 0
    old, old_files = request(tmp_path / "old", reads, mates, interleaved, rc, fmt or 0, reports, passes, ord("_"))
    p = lambda k: getattr(old, k)
    tail = [p("profile_path"), p("coverage_path"), p("redistribute_path"), passes, p("hitmap_path"), p("samples_path"), ord("_"),
            p("sample_redistribute_path")]
    n_tail = {0: 0, 1: 1, 2: 2, 3: 4, 4: 5, 5: 7, 6: 8}[len(reports)]
    if name == "utree_search_pairs_file":
        head = [old.reads_path, mates.encode(), old.out_path, rc, T, fmt]
    elif len(reports) >= 3:
        head = [old.reads_path, old.mates_path, interleaved, old.out_path, rc, T, fmt]
    else:
        head = [old.reads_path, old.out_path, rc, T] + ([] if fmt is None else [fmt])
    arr = (C.c_void_p * 1)(toy["trees"][0]._h)
    st_old = lib.SearchStats()
    lib.check(getattr(lib.load(), name)(toy["db"]._h, arr, 1, *head, *tail[:n_tail], C.byref(st_old)), name)
    # the equivalent request; a delimiter of 0 still means '_'
    new, new_files = request(tmp_path / "new", reads, mates, interleaved, rc, fmt or 0, reports, passes, 0)
    st_new = run(toy, new)
    same_files(old_files, new_files)
    assert (st_old.n_reads, st_old.good_finds, st_old.pipeline) == (st_new.n_reads, st_new.good_finds, st_new.pipeline)
    want = toy["want_single"][rc] if kind == "single" else toy["want_pairs"][rc]
    assert new_files["out_path"].read_bytes() == want == old_files["out_path"].read_bytes()


RANK = {
    "utree_rank_search_file": (0, None, ()),
    "utree_rank_search_file_opts": (1, lib.INPUT_AUTO, ()),
    "utree_rank_search_file_profile": (0, lib.INPUT_REFERENCE, ("profile_path",)),
    "utree_rank_search_file_samples": (1, lib.INPUT_REFERENCE, ("profile_path", "samples_path")),
}


@pytest.mark.parametrize("name", sorted(RANK))
def test_rank_entry_point_and_its_request_write_the_same_bytes(toy, name, tmp_path):
    rc, fmt, reports = RANK[name]
    prm = lib.RankParams(2, 4, 2)
    reads = write_inputs(toy, tmp_path, "single")[0]
    old, old_files = request(tmp_path / "old", reads, None, 0, rc, fmt or 0, reports)
    tail = [old.profile_path] * (len(reports) >= 1) + [old.samples_path, ord("_")] * (len(reports) >= 2)
    st_old = lib.SearchStats()
    lib.check(getattr(lib.load(), name)(toy["db"]._h, toy["trees"][0]._h, old.reads_path, old.out_path, rc, C.byref(prm), T,
                                        *([] if fmt is None else [fmt]), *tail, C.byref(st_old)), name)
    new, new_files = request(tmp_path / "new", reads, None, 0, rc, fmt or 0, reports, rank=prm)
    st_new = run(toy, new)
    same_files(old_files, new_files)
    assert (st_old.n_reads, st_old.good_finds) == (st_new.n_reads, st_new.good_finds)
    assert new_files["out_path"].read_bytes() == toy["want_rank"][rc]


# ---- 2. the one shard path at its edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "two", "inter"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_second_shard_empty_full_and_half(toy, kind, n, tmp_path, monkeypatch):
    """two handles, per = ceil(n / 2) records each: the second shard of 1, 2, 3 records is empty, full, half.  With a hit map and a sample
    table the names ride the uploaded span and the map's shard offsets are in play."""
    monkeypatch.setenv("UTREE_HOST_TEXT", "1")
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "65536")             # (one slot holds the input; the buffers and the map's worst case stay small)
    reads, mates, interleaved = write_inputs(toy, tmp_path, kind, n)
    one, one_files = request(tmp_path / "one", reads, mates, interleaved, 1, reports=("hitmap_path", "samples_path"))
    two, two_files = request(tmp_path / "two", reads, mates, interleaved, 1, reports=("hitmap_path", "samples_path"))
    st1, st2 = run(toy, one, 1), run(toy, two, 2)
    assert st1.n_reads == st2.n_reads == n and st1.pipeline == st2.pipeline == 0
    same_files(one_files, two_files)
    assert one_files["hitmap_path"].read_bytes().count(b"\n") == n


# ---- 3. everything at once ---------------------------------------------------------------------------------------------------------------
def test_every_report_over_several_slots_on_two_handles(toy, tmp_path, monkeypatch):
    reads, mates, interleaved = write_inputs(toy, tmp_path, "two")
    one, one_files = request(tmp_path / "one", reads, mates, interleaved, 1, reports=REPORTS, max_passes=PASSES)
    st1 = run(toy, one, 1)
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "30000")             # several slots, and a carry in each file
    two, two_files = request(tmp_path / "two", reads, mates, interleaved, 1, reports=REPORTS, max_passes=PASSES)
    st2 = run(toy, two, 2)
    assert st1.n_reads == st2.n_reads == toy["P"].n and len(toy["P"].reads_fasta()) > 8 * 30000
    same_files(one_files, two_files)
    assert two_files["out_path"].read_bytes() == toy["want_pairs"][1]


# ---- 4. more than one formatting piece per slot -------------------------------------------------------------------------------------------
def test_three_formatting_pieces_across_a_shard_edge(toy, tmp_path, monkeypatch):
    """8193 reads in one slot, three host threads, two handles: the formatter cuts the slot into min(threads, reads / 4096 + 1) = 3 pieces at
    reads 2731 and 5462, the handles' shards meet at read 4097 -- inside piece 1 --, and piece 2 is all of handle 1's.  The output, the map,
    the sample table and each read's redistributed label (the spool's records carry the handle) equal those of one handle and one piece."""
    n = 8193
    monkeypatch.setenv("UTREE_HOST_TEXT", "1")
    monkeypatch.delenv("UTREE_CHUNK_BYTES", raising=False)
    reads = write_inputs(toy, tmp_path, "single", n)[0]
    reports = ("hitmap_path", "samples_path", "redistribute_reads_path")
    one, one_files = request(tmp_path / "one", reads, None, 0, 1, reports=reports, max_passes=PASSES)
    two, two_files = request(tmp_path / "two", reads, None, 0, 1, reports=reports, max_passes=PASSES)
    one.host_threads, two.host_threads = 1, 3
    st1, st2 = run(toy, one, 1), run(toy, two, 2)
    assert st1.n_reads == st2.n_reads == n and st1.pipeline == st2.pipeline == 0
    same_files(one_files, two_files)
    assert two_files["hitmap_path"].read_bytes().count(b"\n") == n
    names = set(fasta_names(open(reads, "rb").read()))
    assert len(names) == n
    want = b"".join(l for l in toy["want_single"][1].splitlines(True) if l.split(b"\t", 1)[0] in names)
    assert two_files["out_path"].read_bytes() == want
