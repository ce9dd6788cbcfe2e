"""GPU tests of the per-sample redistribution (csrc/sredist_kernels.hip, csrc/sredist.c, UTREE_SAMPLE_REDISTRIBUTE): the per-sample multisets of
candidate sets read back from the device, every sample's passes and every file must equal tests/sample_redist_ref.py -- the contract restated
with the CPU oracle, pinned in tests/test_sample_redist_cpu.py --, and the per-read results must stay what they were.  All comparisons are
exact: there is no tolerance in this feature.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import json
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pairs_ref
import redist_ref
import sample_redist_ref as srr
import samples_ref as sr
from test_coverage_cpu import fixture_seqs
from test_gpu_redist import mixed_reads, mixed_reference
from test_redist_cpu import reference_sets
from test_sample_redist_cpu import PAD, PINNED, dealt
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, SredistReadback, search_gg
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


def fasta(names, seqs):
    return b"".join(b">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs))


def device_batch(torch, names, seqs):
    """(bases, off, len, text, name_off, name_len): one device text of '>name\\nseq\\n' records, the bases read in place"""
    off, ln, noff, nlen, pos = [], [], [], [], 0
    for nm, s in zip(names, seqs):
        noff.append(pos + 1); nlen.append(len(nm)); off.append(pos + len(nm) + 2); ln.append(len(s))
        pos += len(nm) + len(s) + 3
    buf = torch.from_numpy(np.frombuffer(fasta(names, seqs) + b"\0", dtype=np.uint8).copy()).cuda()
    return (buf, torch.from_numpy(np.array(off, dtype=np.int64)).cuda(), torch.from_numpy(np.array(ln, dtype=np.int32)).cuda(), buf,
            torch.from_numpy(np.array(noff, dtype=np.int32)).cuda(), torch.from_numpy(np.array(nlen, dtype=np.int32)).cuda())


def check_readback(rb, sets, ids, times=1):
    """the read-back is the reference's: ids, per-sample reads and unclassified reads, per-sample multisets of sets"""
    n = Counter(ids)
    assert rb.n_reads == times * len(ids) and sorted(rb.ids) == sorted(n) and len(set(rb.ids)) == len(rb.ids)
    assert dict(zip(rb.ids, rb.reads.tolist())) == {i: times * c for i, c in n.items()}
    uncl = Counter(i for s, i in zip(sets, ids) if not s)
    assert dict(zip(rb.ids, rb.unclassified.tolist())) == {i: times * uncl.get(i, 0) for i in n}
    want = {i: {s: times * c for s, c in ms.items()} for i, ms in srr.multisets(sets, ids).items()}
    assert rb.multisets() == want


def solved_of(rb, e, passes, ambiguous):
    """{id: (assigned, unique, passes, ambiguous)} of a solve, zeros dropped"""
    out = {i: ({}, {}, int(passes[k]), int(ambiguous[k])) for k, i in enumerate(rb.ids)}
    for s, l, a, u in e.tolist():
        if a:
            out[rb.ids[s]][0][l] = a
        if u:
            out[rb.ids[s]][1][l] = u
    return out


def want_solved(sets, ids, mp=100):
    return {i: ({l: c for l, c in v[0].items() if c}, {l: c for l, c in v[1].items() if c}, v[2], v[3]) for i, v in srr.solve(sets, ids, mp).items()}


# ---- 1. per-sample multisets of sets, every classify path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("deal", ["block", "rr"])
@pytest.mark.parametrize("name,rc", [(n, r) for n in ("toy", "vote", "k64", "ix32", "k64ix32", "k16") for r in (0, 1)])
def test_multisets_equal_the_reference(torch_cuda, name, rc, deal):
    torch = torch_cuda
    db, tree = tree_for(name)
    seqs = fixture_seqs(name)[:N_READS]
    sets, texts, names, ids = dealt(name, rc, N_READS, deal)
    t = device_batch(torch, names, seqs)
    plain = tree.classify(*t[:3], rc=bool(rc))
    torch.cuda.synchronize()
    h = tree.sample_redistribution(64, 1 << 14, 1 << 14)
    try:
        got = h.classify(*t, rc=bool(rc))
        torch.cuda.synchronize()
        tree.poll()
        assert torch.equal(got, plain)                              # bit for bit utree_classify_batch's
        rb = h.read()
        check_readback(rb, sets, ids)
        h.reset()
        rb = h.read()
        assert rb.n_reads == 0 and rb.ids == [] and len(rb.cells) == 0
    finally:
        h.close()


def test_several_workgroups_and_rounds(torch_cuda):
    """20 000 reads in one batch: two workgroups, three rounds each, the queue of ambiguous reads carried over a round"""
    torch = torch_cuda
    db, tree = tree_for("toy")
    sets, _ = reference_sets("toy", 0, N_READS)
    seqs = fixture_seqs("toy")[:N_READS] * 5
    sets = list(sets) * 5
    for deal in ("block", "rr"):
        names = srr.deal_names(len(seqs), deal, [b"S%d" % k for k in range(7)])
        ids = [sr.sample_id(nm) for nm in names]
        h = tree.sample_redistribution(64, 1 << 14, 1 << 15)
        try:
            h.classify(*device_batch(torch, names, seqs), rc=False)
            check_readback(h.read(), sets, ids)
        finally:
            h.close()


# ---- 2. solve -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,deal", [("toy", "rr"), ("vote", "rr"), ("vote", "block")])
def test_solve_equals_the_reference(torch_cuda, name, deal):
    torch = torch_cuda
    db, tree = tree_for(name)
    sets, texts, names, ids = dealt(name, 0, N_READS, deal)
    h = tree.sample_redistribution(64, 1 << 14, 1 << 14)
    try:
        h.classify(*device_batch(torch, names, fixture_seqs(name)[:N_READS]), rc=False)
        rb = h.read()
        for mp in (1, 3, 100):
            assert solved_of(rb, *h.solve(mp)) == want_solved(sets, ids, mp)
        passes = dict(zip(rb.ids, h.solve(100)[1].tolist()))
        assert tuple(passes[s] for s in srr.THREE) == PINNED[(name, 0, N_READS, deal)]      # the samples stop on their own
        assert len(set(passes.values())) > 1
        with pytest.raises(lib.UtreeError):
            h.solve(0)
        with pytest.raises(lib.UtreeError):
            h.solve(1001)
    finally:
        h.close()


def test_stopping_threshold_above_zero(torch_cuda):
    """the read-back inserted with every count times 1000 (N_s >= 100 000), and with PAD unclassified reads added to every sample instead
    (N_s grows alone: some sample stops earlier): both against solve_multiset on the same multiset"""
    torch = torch_cuda
    db, tree = tree_for("vote")
    sets, texts, names, ids = dealt("vote", 0, N_READS, "rr")
    h = tree.sample_redistribution(64, 1 << 14, 1 << 14)
    big, pad = tree.sample_redistribution(64, 1 << 14, 1 << 14), tree.sample_redistribution(64, 1 << 14, 1 << 14)
    try:
        h.classify(*device_batch(torch, names, fixture_seqs("vote")[:N_READS]), rc=False)
        rb = h.read()
        base = dict(zip(rb.ids, h.solve(100)[1].tolist()))
        cells = rb.cells.copy()
        cells["reads"] *= 1000
        big.insert(SredistReadback(rb.ids, rb.reads * 1000, rb.unclassified * 1000, cells, rb.labels, rb.n_reads * 1000))
        pad.insert(SredistReadback(rb.ids, rb.reads + PAD, rb.unclassified + PAD, rb.cells, rb.labels, rb.n_reads + PAD * len(rb.ids)))
        earlier = 0
        for hh, mul, add in ((big, 1000, 0), (pad, 1, PAD)):
            r2 = hh.read()
            assert r2.n_reads == rb.n_reads * mul + add * len(rb.ids)
            got = solved_of(r2, *hh.solve(100))
            for i, ms in srr.multisets(sets, ids).items():
                n = int(rb.reads[rb.ids.index(i)]) * mul + add
                assert n >= 100000
                a, u, p, amb = srr.solve_multiset({s: c * mul for s, c in ms.items()}, n)
                assert got[i] == ({l: c for l, c in a.items() if c}, {l: c for l, c in u.items() if c}, p, amb), (i, mul)
                earlier += p < base[i]
        assert earlier > 0
    finally:
        h.close(); big.close(); pad.close()


# ---- 3. a batch made by hand --------------------------------------------------------------------------------------------------------------
_HAND = {}


def hand_made():
    """(names, seqs, sets) -- reads of the toy fixture chosen by their candidate sets (RC off)"""
    if not _HAND:
        sets, _ = reference_sets("toy", 0, N_READS)
        seqs = fixture_seqs("toy")[:N_READS]
        first = {}
        for r, s in enumerate(sets):
            first.setdefault(s, r)
        a, b = next((s for s in sorted(first) if len(s) == 2 and (s[0],) in first and (s[1],) in first))
        r_ab, r_a, r_b, r_none = first[(a, b)], first[(a,)], first[(b,)], first[()]
        multi = first[Counter(s for s in sets if len(s) > 2).most_common(1)[0][0]]
        rows = [(b"w%02d_1" % k, multi) for k in range(64)]                                  # 64 samples, one multi-label set: one set slot, 64 cells
        rows += [(b"runA_%d" % r, r) for r in range(70)] + [(b"runB_%d" % r, r) for r in range(70, 140)]
        rows += [(b"runA_%d" % r, r) for r in range(140, 210)]                               # the same id in non-adjacent runs
        rows += [(b"_7", 300), (b"_8", multi), (b"", 301)]                                   # the empty id
        rows += [(b"nodelim", 302), (b"nodelim", r_ab), (b"x.y_z.1", 303), (b"x.y_z.2", multi), (b"x.y_q.1", 304)]
        rows += [(b"void_%d" % k, r_none) for k in range(5)]                                 # a sample of unclassified reads only
        rows += [(b"tieA_%d" % k, r) for k, r in enumerate([r_ab] * 3 + [r_b, r_a, r_none, r_none])]      # T0: a 4, b 4 -- the tie goes to a
        rows += [(b"tieB_%d" % k, r) for k, r in enumerate([r_ab] * 3 + [r_b] * 3 + [r_a])]               # the other majority: b
        _HAND["v"] = ([nm for nm, _ in rows], [seqs[r] for _, r in rows], [sets[r] for _, r in rows], (a, b))
    return _HAND["v"]


@pytest.mark.parametrize("delim", [b"_", b"."])
def test_batch_made_by_hand(torch_cuda, delim, tmp_path):
    torch = torch_cuda
    db, tree = tree_for("toy")
    names, seqs, sets, (a, b) = hand_made()
    ids = [sr.sample_id(nm, delim) for nm in names]
    assert (b"" in ids) and (b"nodelim" in ids) and ((b"x.y" in ids) == (delim == b"_")) and ((b"x.y_z" in ids) == (delim == b"."))
    h = tree.sample_redistribution(1024, 1 << 10, 1 << 12, delim)         # (with '.' most names are ids of their own)
    try:
        h.classify(*device_batch(torch, names, seqs), rc=False)
        rb = h.read()
        check_readback(rb, sets, ids)
        got = solved_of(rb, *h.solve(100))
        assert got == want_solved(sets, ids)
        if delim == b"_":
            assert len({tuple(sorted(rb.labels[f:f + n].tolist())) for s, n, f, r in rb.cells.tolist() if rb.ids[s].startswith(b"w")}) == 1
            assert got[b"tieA"][0] == {a: 4, b: 1} and got[b"tieB"][0] == {a: 1, b: 6} and got[b"void"] == ({}, {}, 1, 0)
        path = tmp_path / "t.tsv"
        h.write(str(path))
        assert path.read_bytes() == srr.file_from_sets(sets, [db.label(i) for i in range(db.info.n_labels)], names, delim)
        srr.check_invariants(path.read_bytes())
    finally:
        h.close()


# ---- 4. one batch of mixed lengths: the mid, pieces and long-read paths ---------------------------------------------------------------------
@pytest.mark.parametrize("rc,lane_pass", [(0, "1"), (1, "1"), (0, "0"), (1, "0")])
def test_mixed_length_batch(torch_cuda, rc, lane_pass, monkeypatch):
    torch = torch_cuda
    monkeypatch.setenv("UTREE_LANE_PASS", lane_pass)
    db, tree = tree_for("toy")
    seqs = mixed_reads()
    sets = mixed_reference(rc)
    names = srr.deal_names(len(seqs), "rr")
    ids = [sr.sample_id(nm) for nm in names]
    t = device_batch(torch, names, seqs)
    plain = tree.classify(*t[:3], rc=bool(rc))
    torch.cuda.synchronize()
    h = tree.sample_redistribution(64, 1 << 12, 1 << 12)
    try:
        got = h.classify(*t, rc=bool(rc))
        torch.cuda.synchronize()
        tree.poll()
        assert torch.equal(got, plain)
        check_readback(h.read(), sets, ids)
        res = got.cpu().numpy()
        assert sum(1 for s, r in zip(seqs, res) if len(s) > 2 * 2112 and r[2] > 0 and r[3] == 1) >= 3     # finished single-label records of long reads
    finally:
        h.close()


# ---- 5. streams, merge, two handles ---------------------------------------------------------------------------------------------------------
def test_four_streams_add_at_once(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    sets, texts, names, ids = dealt("toy", 0, N_READS, "rr")
    t = device_batch(torch, names, fixture_seqs("toy")[:N_READS])
    total, mx = int(t[2].sum().item()), int(t[2].max().item())
    need = tree.workspace_bytes(N_READS, total, mx, False)
    streams = [torch.cuda.Stream() for _ in range(4)]
    ws = [torch.empty(need, dtype=torch.uint8, device="cuda") for _ in range(4)]
    outs = [torch.empty((N_READS, 6), dtype=torch.int32, device="cuda") for _ in range(4)]
    h = tree.sample_redistribution(64, 1 << 12, 1 << 13)
    try:
        torch.cuda.synchronize()
        for s, w, o in zip(streams, ws, outs):
            with torch.cuda.stream(s):
                h.classify(*t, rc=False, total_bases=total, max_len=mx, out=o, workspace=w)
        torch.cuda.synchronize()
        tree.poll()
        check_readback(h.read(), sets, ids, times=4)
        assert all(torch.equal(o, outs[0]) for o in outs[1:])
    finally:
        h.close()


def test_merge_of_two_handles_equals_one(torch_cuda):
    """two handles side by side on one card, fed different halves (the samples numbered otherwise in each), merged"""
    torch = torch_cuda
    db, tree = tree_for("toy")
    sets, texts, names, ids = dealt("toy", 0, N_READS, "rr")
    seqs = fixture_seqs("toy")[:N_READS]
    a, b = tree.sample_redistribution(16, 1 << 12, 1 << 12), tree.sample_redistribution(64, 1 << 13, 1 << 13)
    try:
        cut = 1700
        a.classify(*device_batch(torch, names[:cut], seqs[:cut]), rc=False)
        b.classify(*device_batch(torch, names[cut:][::-1], seqs[cut:][::-1]), rc=False)
        check_readback(b.read(), sets[cut:], ids[cut:])
        a.merge(b)
        rb = a.read()
        check_readback(rb, sets, ids)
        assert solved_of(rb, *a.solve()) == want_solved(sets, ids)
        assert b.read().n_reads == N_READS - cut                     # the source keeps its own
    finally:
        a.close(); b.close()


# ---- 6. capacities ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("caps,knob", [((2, 1 << 12, 1 << 12), "UTREE_SAMPLE_CAPACITY"), ((64, 16, 1 << 12), "UTREE_REDIST_CAPACITY"),
                                       ((64, 1 << 12, 16), "UTREE_SAMPLE_CELLS")])
def test_a_table_too_small_is_an_error_not_a_wrong_table(torch_cuda, caps, knob):
    torch = torch_cuda
    db, tree = tree_for("toy")
    sets, texts, names, ids = dealt("toy", 0, N_READS, "rr")
    t = device_batch(torch, names, fixture_seqs("toy")[:N_READS])
    plain = tree.classify(*t[:3], rc=False)
    h = tree.sample_redistribution(*caps)
    try:
        got = h.classify(*t, rc=False)
        torch.cuda.synchronize()
        tree.poll()
        assert torch.equal(got, plain)                               # the per-read results do not depend on it
        for call in (h.read, h.solve):
            with pytest.raises(lib.UtreeError) as e:
                call()
            assert e.value.code == lib.E_DEVICE and knob in str(e.value)
        h.reset()
        h.classify(*device_batch(torch, names[:2], fixture_seqs("toy")[:2]), rc=False)
        assert h.read().n_reads == 2                                  # usable again after a reset
    finally:
        h.close()


def test_create_refuses_what_it_cannot_hold(torch_cuda):
    db, tree = tree_for("toy")
    for args in ((0, 16, 16), ((1 << 19) + 1, 16, 16), (16, 0, 16), (16, (1 << 28) + 1, 16), (16, 16, 0), (16, 16, (1 << 30) + 1), (16, 16, 16, b"\t")):
        with pytest.raises(lib.UtreeError) as e:
            tree.sample_redistribution(*args)
        assert e.value.code == lib.E_ARG
    t = device_batch(torch_cuda, [b"a_1"], [b"ACGT" * 10])
    h = tree.sample_redistribution(16, 16, 16)
    try:
        with pytest.raises(ValueError):
            h.classify(*t[:3], t[3], t[4].long(), t[5])
        # a name that leaves the text: refused and flagged, never read
        h.classify(*t[:4], t[4] + 1000, t[5])
        with pytest.raises(lib.UtreeError) as e:
            h.read()
        assert e.value.code == lib.E_DEVICE and "name" in str(e.value)
    finally:
        h.close()


# ---- 7. the whole-file search -------------------------------------------------------------------------------------------------------------------
def toy_case(tmp_path, deal="rr", rc=1):
    sets, texts, names, ids = dealt("toy", rc, N_READS, deal)
    fa = tmp_path / ("reads_%s.fa" % deal)
    fa.write_bytes(fasta(names, fixture_seqs("toy")[:N_READS]))
    return fa, names, sets, texts


def test_device_host_and_small_chunks_write_the_reference_file(torch_cuda, tmp_path, monkeypatch):
    db, tree = tree_for("toy")
    fa, names, sets, texts = toy_case(tmp_path)
    want = srr.file_from_sets(sets, texts, names)
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "a.txt"), rc=True, threads=4)
    assert code == lib.OK and st.pipeline == 1
    plain = (tmp_path / "a.txt").read_bytes()
    tab = tmp_path / "s.tsv"
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "b.txt"), rc=True, threads=4, sample_redistribute=str(tab))
    assert code == lib.OK and st.pipeline == 1 and st.n_reads == N_READS and (tmp_path / "b.txt").read_bytes() == plain
    assert tab.read_bytes() == want
    srr.check_invariants(want)
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "c.txt"), rc=True, threads=4, sample_redistribute=str(tab), redist_passes=1)
    assert code == lib.OK and tab.read_bytes() == srr.file_from_sets(sets, texts, names, max_passes=1) != want
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "d.txt"), rc=True, threads=4, sample_redistribute=str(tab), sample_delim=b".")
    assert code == lib.OK and tab.read_bytes() == srr.file_from_sets(sets, texts, names, b".")
    monkeypatch.setenv("UTREE_HOST_TEXT", "1")
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "e.txt"), rc=True, threads=4, sample_redistribute=str(tab))
    assert code == lib.OK and st.pipeline == 0 and (tmp_path / "e.txt").read_bytes() == plain and tab.read_bytes() == want
    # two device handles on one card: the host pipeline's shards, merged before the passes
    tree2 = DeviceTree.upload(db, 0)
    try:
        code, st = search_gg(db, [tree, tree2], str(fa), str(tmp_path / "f.txt"), rc=True, threads=4, sample_redistribute=str(tab))
        assert code == lib.OK and (tmp_path / "f.txt").read_bytes() == plain and tab.read_bytes() == want
        monkeypatch.delenv("UTREE_HOST_TEXT")
        monkeypatch.setenv("UTREE_CHUNK_BYTES", "20000")
        code, st = search_gg(db, [tree, tree2], str(fa), str(tmp_path / "g.txt"), rc=True, threads=4, sample_redistribute=str(tab))
        assert code == lib.OK and st.pipeline == 1 and (tmp_path / "g.txt").read_bytes() == plain and tab.read_bytes() == want
    finally:
        tree2.close()
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "4000")
    fb, names_b, _, _ = toy_case(tmp_path, "block")
    code, st = search_gg(db, [tree], str(fb), str(tmp_path / "h.txt"), rc=True, threads=4, sample_redistribute=str(tab))
    assert code == lib.OK and st.pipeline == 1 and tab.read_bytes() == srr.file_from_sets(sets, texts, names_b)
    # a file that cannot be written: the search's output, UTREE_E_PROFILE, the cause by name
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "i.txt"), rc=True, threads=4, sample_redistribute="/dev/full")
    assert code == lib.E_PROFILE and b"sample redistribution /dev/full" in lib.load().utree_last_hip_error()
    assert (tmp_path / "i.txt").read_bytes() == plain


_PAIRS = {}


def pairs_case(n=1500):
    if not _PAIRS:
        P = pairs_ref.Pairs("toy")
        ctr = util.fixture_ctr("toy")
        sets, texts = redist_ref.candidate_sets(ctr, P.joined_seqs()[:n], True)
        _PAIRS["v"] = (P, sets, texts)
    return _PAIRS["v"]


@pytest.mark.parametrize("interleaved", [False, True])
def test_pairs_count_once_under_mate_ones_name(torch_cuda, interleaved, tmp_path, monkeypatch):
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "30000")
    db, tree = tree_for("toy")
    n = 1500
    P, sets, texts = pairs_case(n)
    names = srr.deal_names(n, "rr")
    old = P.names1
    P.names1 = names + list(old[n:])
    try:
        reads, mates = (P.interleaved_fasta(2 * n), None) if interleaved else (P.reads_fasta(n), P.mates_fasta(n))
    finally:
        P.names1 = old
    rp, mp, tab = tmp_path / "r.fa", tmp_path / "m.fa", tmp_path / "s.tsv"
    rp.write_bytes(reads)
    if mates is not None:
        mp.write_bytes(mates)
    kw = dict(rc=True, threads=4, mates=str(mp) if mates is not None else None, interleaved=interleaved)
    code, st = search_gg(db, [tree], str(rp), str(tmp_path / "a.txt"), **kw)
    assert code == lib.OK
    code, st = search_gg(db, [tree], str(rp), str(tmp_path / "b.txt"), sample_redistribute=str(tab), **kw)
    assert code == lib.OK and st.n_reads == n and (tmp_path / "b.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    assert tab.read_bytes() == srr.file_from_sets(sets, texts, names)


def test_fastq_and_gzip(torch_cuda, tmp_path):
    db, tree = tree_for("toy")
    fa, names, sets, texts = toy_case(tmp_path)
    seqs = fixture_seqs("toy")[:N_READS]
    fq = b"".join(b"@%s\n%s\n+\n%s\n" % (nm, s, b"I" * len(s)) for nm, s in zip(names, seqs))
    tab = tmp_path / "s.tsv"
    for tag, blob, fmt in (("q", fq, lib.INPUT_FASTQ), ("z", pairs_ref.gz(fq), lib.INPUT_AUTO)):
        p = tmp_path / (tag + ".in")
        p.write_bytes(blob)
        code, st = search_gg(db, [tree], str(p), str(tmp_path / (tag + ".txt")), rc=True, threads=4, input_format=fmt, sample_redistribute=str(tab))
        assert code == lib.OK and st.pipeline == 0 and st.n_reads == N_READS
        assert tab.read_bytes() == srr.file_from_sets(sets, texts, names)
        tab.unlink()


def test_with_every_other_report_nothing_else_changes(torch_cuda, tmp_path):
    db, tree = tree_for("toy")
    fa, names, sets, texts = toy_case(tmp_path, rc=0)
    files = {}
    for tag in ("a", "b"):
        p = lambda x: str(tmp_path / (tag + "." + x))
        kw = {"sample_redistribute": p("sr")} if tag == "b" else {}
        code, st = search_gg(db, [tree], str(fa), p("txt"), threads=4, profile=p("prof"), coverage=p("cov"), redistribute=p("rd"), hitmap=p("hm"),
                             samples=p("smp"), **kw)
        assert code == lib.OK
        files[tag] = [open(p(x), "rb").read() for x in ("txt", "prof", "cov", "rd", "hm", "hm.labels", "smp")]
    assert files["a"] == files["b"] and not (tmp_path / "a.sr").exists()
    got = (tmp_path / "b.sr").read_bytes()
    assert got == srr.file_from_sets(sets, texts, names)
    # the `# reads` and `# unclassified` rows are the sample table's rows for the same run
    N, G, A, S, ids, n, u, a, P, rows = srr.check_invariants(got)
    tN, tG, tS, tids, tn, tu, _ = sr.parse_table(files["b"][6])
    assert (N, S, ids, n, u) == (tN, tS, tids, tn, tu)
    # the pooled file is what it is without the new report, and another statistic
    pa, pu, pp, pamb, _ = redist_ref.solve(sets, N_READS)
    assert files["b"][3] == redist_ref.redist_file(pa, pu, texts, N_READS, pamb, pp)


def test_one_sample_is_the_redistributions_column(torch_cuda, tmp_path):
    db, tree = tree_for("vote")
    seqs = fixture_seqs("vote")[:N_READS]
    fa, tab, red = tmp_path / "in.fa", tmp_path / "s.tsv", tmp_path / "r.tsv"
    fa.write_bytes(fasta([b"only_%d" % i for i in range(N_READS)], seqs))
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "o.txt"), threads=4, redistribute=str(red), sample_redistribute=str(tab))
    assert code == lib.OK and st.pipeline == 1
    N, G, A, S, ids, n, u, a, P, rows = srr.check_invariants(tab.read_bytes())
    lines = red.read_bytes().split(b"\n")
    head = lines[0].split(b"\t")
    assert (N, G, A, S, ids, P) == (N_READS, int(head[3]), int(head[7]), 1, [b"only"], [int(head[9])])
    want = {}
    for ln in lines[2:-1]:
        f = ln.rsplit(b"\t", 4)
        if int(f[1]):
            want[f[0]] = [int(f[1])]
    assert rows == want


def test_a_failed_search_leaves_the_path_as_it_was(torch_cuda, tmp_path):
    cases = json.load(open(os.path.join(util.GOLD, "edge_cases.json")))
    db, tree = tree_for("toy")
    bad = 0
    for nm, c in sorted(cases.items()):
        if c["exit"] == 0:
            continue
        fa, tab = tmp_path / "in.fa", tmp_path / "s.tsv"
        fa.write_bytes(bytes.fromhex(c["input_hex"]))
        tab.write_bytes(b"what was here before\n")
        code, st = search_gg(db, [tree], str(fa), str(tmp_path / "o.txt"), rc=bool(c["rc"]), threads=4, sample_redistribute=str(tab))
        assert code != lib.OK and (tmp_path / "o.txt").read_bytes() == bytes.fromhex(c["output_hex"]), nm
        assert tab.read_bytes() == b"what was here before\n", nm
        bad += 1
    assert bad > 0


# ---- 8. the command line --------------------------------------------------------------------------------------------------------------------------
VARS = ("UTREE_SAMPLE_REDISTRIBUTE", "UTREE_SAMPLE_TABLE", "UTREE_SAMPLE_DELIM", "UTREE_SAMPLE_CAPACITY", "UTREE_SAMPLE_CELLS", "UTREE_REDISTRIBUTE",
        "UTREE_REDIST_PASSES", "UTREE_REDIST_CAPACITY", "UTREE_PROFILE", "UTREE_COVERAGE", "UTREE_HITMAP", "UTREE_MATES", "UTREE_INTERLEAVED")


def run_cli(cli, ctr, fa, out, rc, **env):
    base = dict(os.environ, UTREE_GPUS="1")
    for v in VARS:
        base.pop(v, None)
    return subprocess.run([cli, ctr, str(fa), str(out), "4"] + (["RC"] if rc else []), capture_output=True, env=dict(base, **env), timeout=300)


def test_cli(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    fa, names, sets, texts = toy_case(tmp_path)
    want = srr.file_from_sets(sets, texts, names)
    plain = run_cli(cli, ctr, fa, tmp_path / "a.txt", 1)
    assert plain.returncode == 0 and sorted(p.name for p in tmp_path.iterdir()) == ["a.txt", fa.name]      # without the variable: no file
    out = (tmp_path / "a.txt").read_bytes()
    tab = tmp_path / "s.tsv"
    r = run_cli(cli, ctr, fa, tmp_path / "b.txt", 1, UTREE_SAMPLE_REDISTRIBUTE=str(tab))
    assert r.returncode == 0 and r.stdout == plain.stdout and (tmp_path / "b.txt").read_bytes() == out and tab.read_bytes() == want
    r = run_cli(cli, ctr, fa, tmp_path / "c.txt", 1, UTREE_SAMPLE_REDISTRIBUTE=str(tab), UTREE_REDIST_PASSES="1", UTREE_SAMPLE_DELIM=".")
    assert r.returncode == 0 and tab.read_bytes() == srr.file_from_sets(sets, texts, names, b".", 1)
    # paths and knobs
    bad = run_cli(cli, ctr, fa, tmp_path / "f.txt", 1, UTREE_SAMPLE_REDISTRIBUTE=str(tmp_path / "no" / "dir" / "s.tsv"))
    assert bad.returncode == 1 and b"sample redistribution" in bad.stderr and b"Tree read." not in bad.stdout and not (tmp_path / "f.txt").exists()
    tab.unlink()
    for var, value in (("UTREE_SAMPLE_CAPACITY", "2"),):              # (a file named without the convention ends like this)
        small = run_cli(cli, ctr, fa, tmp_path / "g.txt", 1, UTREE_SAMPLE_REDISTRIBUTE=str(tab), **{var: value})
        assert small.returncode == 1 and small.stdout == plain.stdout and (tmp_path / "g.txt").read_bytes() == out and not tab.exists(), var
        err = [ln for ln in small.stderr.split(b"\n") if ln.startswith(b"ERROR")]
        assert len(err) == 1 and var.encode() in err[0] and str(tab).encode() in err[0], var


def test_rank_specific_cli_ignores_the_variable(torch_cuda, tmp_path):
    ctr, fa = util.fixture_ctr("toy"), util.fixture_reads_path("toy")
    plain = run_cli(lib.RANK_CLI_PATH, ctr, fa, tmp_path / "a.txt", 0)
    withr = run_cli(lib.RANK_CLI_PATH, ctr, fa, tmp_path / "b.txt", 0, UTREE_SAMPLE_REDISTRIBUTE=str(tmp_path / "no" / "dir" / "s.tsv"))
    assert plain.returncode == withr.returncode == 0 and plain.stdout == withr.stdout
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes() == util.fixture_bytes("toy_rank.txt.gz")
    assert not (tmp_path / "no").exists()
