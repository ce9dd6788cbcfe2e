"""GPU tests of the per-sample taxon table (csrc/samples_kernels.hip, csrc/samples.c, UTREE_SAMPLE_TABLE).  The golden fixtures name their
reads q0, q1, ...: the tests rewrite the names to <sample>_<n>.  A name only reaches column 1 of the output, so the expected per-read output
is the genuine reference's golden output with the names substituted, and the expected table is tests/samples_ref.py of that.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, search_gg, write_samples
from profile_ref import fasta_names
import pairs_ref
import samples_ref as sr
import util

RANK = util.manifest().get("rank_outputs", {})


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_TREES = {}


def tree_for(name):
    if name not in _TREES:
        while len(_TREES) >= 4:                         # (a handle that has searched a file keeps its lanes' buffers: the oldest go)
            _TREES.pop(next(iter(_TREES)))[1].close()
        db = CtrDB.open(util.fixture_ctr(name))
        _TREES[name] = (db, DeviceTree.upload(db, 0))
    return _TREES[name]


_RENAMED = {}


def renamed(name, rc, deal):
    """(reads bytes, expected output, new names, expected table) of fixture `name` under 7 samples dealt round-robin or in blocks"""
    key = (name, rc, deal)
    if key not in _RENAMED:
        data = util.fixture_bytes(util.READS_OF.get(name, name) + "_reads.fa.gz")
        out = util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
        old = fasta_names(data)
        new = (sr.round_robin_names if deal == "round_robin" else sr.block_names)(len(old), sr.SEVEN)
        data2, out2 = sr.rename_reads(data, out, old, new)
        _RENAMED[key] = (data2, out2, new, sr.samples_ref(out2, new, len(new)))
    return _RENAMED[key]


def run(db, trees, data, tmp_path, rc, tag="t", **kw):
    fa, out, tab = tmp_path / (tag + ".fa"), tmp_path / (tag + ".txt"), tmp_path / (tag + ".samples.tsv")
    fa.write_bytes(data)
    for p in (out, tab):
        if p.exists():
            p.unlink()
    code, st = search_gg(db, trees, str(fa), str(out), rc=bool(rc), threads=4, samples=str(tab), **kw)
    return code, st, out, tab


# ---- 1. the goldens ------------------------------------------------------------------------------------------------------------------
GG = [("toy", 0), ("toy", 1), ("k64", 0), ("k64", 1), ("ix32", 0), ("ix32", 1), ("k16", 0), ("k16", 1), ("vote", 0), ("generic", 0)]


@pytest.mark.parametrize("name,rc", GG)
@pytest.mark.parametrize("deal", ["round_robin", "blocks"])
def test_gg_golden_tables(torch_cuda, name, rc, deal, tmp_path):
    db, tree = tree_for(name)
    data, want, names, table = renamed(name, rc, deal)
    code, st, out, tab = run(db, [tree], data, tmp_path, rc)
    assert code == lib.OK and st.pipeline == 1 and st.n_reads == len(names)
    assert out.read_bytes() == want
    assert tab.read_bytes() == table
    sr.check_invariants(table)


# ---- 2. names, through utree_samples_add on hand-made records ---------------------------------------------------------------------------
LONG = b"L" * 299
NAMES = [b"a_b_3", b"a_", b"_7", b"", b"nodelim", b"abcx_1", b"abcy_1", b"ab_1", b"abc_1", LONG + b"1_5", LONG + b"2_5", b"t\tab_1", b"back\\slash_2",
         b"a.b.3", b"a.", b".7", b"x.y_z.1", b"a_b_4", b"_", b"__"]


def hand_made(db, delim, seed, repeats=3):
    """(text, name_off, name_len, records, ids per record, [(record, taxon)] of those with a line)"""
    rng = np.random.default_rng(seed)
    n_lab = db.info.n_labels
    l0, l1 = 0, n_lab - 1
    kinds = [(l0, -2, 3), (l0, -1, 2), (l1, -1, 1), (l0, 5, 1), (l0, 0, 1), (l1, -2, 7), (l0, -2, 0), (l1, -4, 2), (l0, -3, 1), (l1, 1, 4)]
    recs = [(nm, k) for nm in NAMES for k in kinds] * repeats
    order = rng.permutation(len(recs))
    text, off, ln, res, ids, cls = bytearray(b"##"), [], [], [], [], []
    for i in order:
        nm, (lab, cut, found) = recs[i]
        text += b">"
        off.append(len(text)); ln.append(len(nm))
        text += nm + b"\nACGT\n"
        res.append((lab, cut, found, 1, 0, 0))
        ids.append(sr.sample_id(nm, delim))
        if found and cut != -4:
            t = db.label(lab)
            cls.append((len(ids) - 1, b"" if cut == -1 else t if cut < 0 else t[:cut]))
    return bytes(text), np.array(off, dtype=np.int32), np.array(ln, dtype=np.int32), np.array(res, dtype=np.int32), ids, cls


def to_dev(torch, text, off, ln, res):
    return (torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda(),
            torch.from_numpy(res).cuda())


@pytest.mark.parametrize("delim", [b"_", b"."])
def test_names_and_records_by_hand(torch_cuda, delim, tmp_path):
    torch = torch_cuda
    db, tree = tree_for("toy")
    text, off, ln, res, ids, cls = hand_made(db, delim, 5)
    assert 300 <= len(ids) <= 1000
    smp = tree.samples(64, 1 << 10, delim)
    d = to_dev(torch, text, off, ln, res)
    smp.add(*d)
    half = len(ids) // 2
    smp.add(d[0], d[1][half:], d[2][half:], d[3][half:])             # the second half once more: ids that are there already
    rb = smp.read()
    ids2 = ids + ids[half:]
    cls2 = cls + [(r - half + len(ids), t) for r, t in cls if r >= half]
    assert rb.n_reads == len(ids2) and sorted(rb.ids) == sorted(set(ids2)) and len(rb.ids) == len(set(rb.ids))
    assert b"" in rb.ids and LONG + (b"1" if delim == b"_" else b"1_5") in rb.ids and (b"a_b" in rb.ids) == (delim == b"_") and (b"a.b" in rb.ids) == (delim == b".")
    assert set(rb.cells["cut"].tolist()) == {-2, -1, 0, 1, 5}
    path = tmp_path / "t.tsv"
    write_samples(db, [rb], str(path))
    assert path.read_bytes() == sr.table_from(ids2, cls2, len(ids2))
    smp.reset()
    rb = smp.read()
    assert rb.n_reads == 0 and rb.ids == [] and len(rb.cells) == 0
    smp.add(*d, n=10)                                                # after a reset the handle counts again
    rb = smp.read()
    assert rb.n_reads == 10 and sorted(rb.ids) == sorted(set(ids[:10]))
    smp.close()


def test_add_refuses_what_it_cannot_count(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    with pytest.raises(lib.UtreeError):
        tree.samples(64, 64, b"\t")
    with pytest.raises(lib.UtreeError):
        tree.samples(0, 64, b"_")
    smp = tree.samples(64, 1 << 10)
    text, off, ln, res, ids, cls = hand_made(db, b"_", 6, repeats=1)
    d = to_dev(torch, text, off, ln, res)
    for bad in ((d[0].cpu(), d[1], d[2], d[3]), (d[0], d[1].long(), d[2], d[3]), (d[0], d[1], d[2], d[3][:, :5].contiguous())):
        with pytest.raises(ValueError):
            smp.add(*bad)
    with pytest.raises(ValueError):
        smp.add(*d, n=len(ids) + 1)
    # a name that leaves the text, and a label the database lacks: refused, flagged, never read or counted as something else
    for spoil in ("name", "label"):
        off2, ln2, res2 = off.copy(), ln.copy(), res.copy()
        if spoil == "name":
            off2[7] = len(text) - 1; ln2[7] = 5
        else:
            res2[7] = (db.info.n_labels, -2, 1, 1, 0, 0)
        smp.reset()
        smp.add(d[0], torch.from_numpy(off2).cuda(), torch.from_numpy(ln2).cuda(), torch.from_numpy(res2).cuda())
        with pytest.raises(lib.UtreeError) as ei:
            smp.read()
        assert ei.value.code == lib.E_DEVICE and spoil.encode() in lib.load().utree_last_hip_error()
    smp.reset()
    smp.add(*d)
    assert smp.read().n_reads == len(ids)                            # the same records unspoiled: a table
    smp.close()


# ---- 3. races ----------------------------------------------------------------------------------------------------------------------------
def test_four_streams_meet_2000_new_ids_at_once(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    n, n_ids, n_lab = 200_000, 2000, db.info.n_labels
    rng = np.random.default_rng(21)
    idt = [b"S%d%s" % (i * 7919 % 100003, b"x" * (i % 5)) for i in range(n_ids)]
    assert len(set(idt)) == n_ids
    which = rng.integers(0, n_ids, n)
    which[:n_ids] = rng.permutation(n_ids)                           # every id occurs
    lab = rng.integers(0, min(n_lab, 12), n)
    found = (rng.random(n) < 0.8).astype(np.int32)
    names = [idt[w] + b"_%d" % r for r, w in enumerate(which.tolist())]
    ln = np.array([len(x) for x in names], dtype=np.int32)
    off = (np.concatenate([[0], np.cumsum(ln[:-1] + 1)]) + 1).astype(np.int32)
    text = b">" + b">".join(names)
    res = np.zeros((n, 6), dtype=np.int32)
    res[:, 0], res[:, 1], res[:, 2] = lab, -2, found
    d = to_dev(torch, text, off, ln, res)
    smp = tree.samples(4096, 1 << 16)
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    q = n // 4
    for k, s in enumerate(streams):
        with torch.cuda.stream(s):
            smp.add(d[0], d[1][k * q:(k + 1) * q], d[2][k * q:(k + 1) * q], d[3][k * q:(k + 1) * q])
    torch.cuda.synchronize()
    rb = smp.read()
    assert rb.n_reads == n and len(rb.ids) == n_ids and sorted(rb.ids) == sorted(idt)          # every id once
    col = {s: j for j, s in enumerate(rb.ids)}
    pos = np.array([col[s] for s in idt])[which]
    assert np.array_equal(rb.reads, np.bincount(pos, minlength=n_ids).astype(np.uint64))
    assert np.array_equal(rb.unclassified, np.bincount(pos[found == 0], minlength=n_ids).astype(np.uint64))
    want = np.bincount(pos[found == 1] * 16 + lab[found == 1], minlength=16 * n_ids)
    got = np.zeros(16 * n_ids, dtype=np.int64)
    np.add.at(got, rb.cells["sample"].astype(np.int64) * 16 + rb.cells["label"], rb.cells["reads"].astype(np.int64))
    assert np.array_equal(got, want) and (rb.cells["cut"] == -2).all() and len(rb.cells) == int((want > 0).sum())
    smp.close()


@pytest.mark.parametrize("deal", ["sevenths", "runs_1024", "runs_64", "round_robin"])
def test_several_workgroups_and_rounds(torch_cuda, deal):
    """20 011 records: two workgroups of 10 006 (the second starts in the middle of a run, not on a multiple of 64), three rounds of 4096 each, a
    partial last wavefront.  Long runs of one id: a run's boundary inside a wavefront, and the id a thread had 1024 records before is its id again (sevenths);
    that id is always another sample's (runs_1024); every boundary at lane 0 (runs_64); every lane begins a run (round_robin)."""
    torch = torch_cuda
    db, tree = tree_for("toy")
    n, n_ids = 20_011, 7
    r = np.arange(n)
    which = {"sevenths": r * n_ids // n, "runs_1024": r // 1024 % n_ids, "runs_64": r // 64 % n_ids, "round_robin": r % n_ids}[deal]
    idt = [b"smp%d%s" % (i, b"x" * (i % 3)) for i in range(n_ids)]
    rng = np.random.default_rng(33)
    cut = rng.integers(0, 10, n)
    found = (rng.random(n) < 0.8).astype(np.int32)
    names = [idt[w] + b"_%d" % k for k, w in enumerate(which.tolist())]
    ln = np.array([len(x) for x in names], dtype=np.int32)
    off = (np.concatenate([[0], np.cumsum(ln[:-1] + 1)]) + 1).astype(np.int32)
    res = np.zeros((n, 6), dtype=np.int32)
    res[:, 0], res[:, 1], res[:, 2] = 0, cut, found
    smp = tree.samples(16, 256)
    smp.add(*to_dev(torch, b">" + b">".join(names), off, ln, res))
    rb = smp.read()
    assert rb.n_reads == n and sorted(rb.ids) == sorted(idt)                                   # every id once
    col = {s: j for j, s in enumerate(rb.ids)}
    pos = np.array([col[s] for s in idt])[which]
    assert np.array_equal(rb.reads, np.bincount(pos, minlength=n_ids).astype(np.uint64))
    assert np.array_equal(rb.unclassified, np.bincount(pos[found == 0], minlength=n_ids).astype(np.uint64))
    want = np.bincount(pos[found == 1] * 16 + cut[found == 1], minlength=16 * n_ids)
    got = np.zeros(16 * n_ids, dtype=np.int64)
    np.add.at(got, rb.cells["sample"].astype(np.int64) * 16 + rb.cells["cut"], rb.cells["reads"].astype(np.int64))
    assert np.array_equal(got, want) and (rb.cells["label"] == 0).all() and len(rb.cells) == int((want > 0).sum())
    smp.close()


# ---- 4. capacities -----------------------------------------------------------------------------------------------------------------------
def test_capacities_by_hand(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    names = [b"s%d_%d" % (i % 5, i) for i in range(400)]
    ln = np.array([len(x) for x in names], dtype=np.int32)
    off = (np.concatenate([[0], np.cumsum(ln[:-1] + 1)]) + 1).astype(np.int32)
    res = np.zeros((400, 6), dtype=np.int32)
    res[:, 0], res[:, 1], res[:, 2] = 0, np.arange(400) // 5 % 10, 1 # 5 samples x 10 cuts: 50 distinct cells
    d = to_dev(torch, b">" + b">".join(names), off, ln, res)
    for scap, ccap, word in ((4, 256, b"UTREE_SAMPLE_CAPACITY"), (8, 16, b"UTREE_SAMPLE_CELLS")):
        smp = tree.samples(scap, ccap)
        smp.add(*d)
        with pytest.raises(lib.UtreeError) as ei:
            smp.read()
        assert ei.value.code == lib.E_DEVICE and word in lib.load().utree_last_hip_error()
        smp.close()
    smp = tree.samples(5, 64)                                         # exactly enough ids
    smp.add(*d)
    rb = smp.read()
    assert sorted(rb.ids) == [b"s%d" % i for i in range(5)] and (rb.reads == 80).all() and len(rb.cells) == 50
    smp.close()


@pytest.mark.parametrize("var,value,word", [("UTREE_SAMPLE_CAPACITY", "4", b"UTREE_SAMPLE_CAPACITY"), ("UTREE_SAMPLE_CELLS", "1", b"UTREE_SAMPLE_CELLS")])
def test_file_search_with_a_table_too_small(torch_cuda, var, value, word, tmp_path, monkeypatch):
    db, tree = tree_for("toy")
    data, want, names, table = renamed("toy", 1, "round_robin")
    assert table.count(b"\n") - 4 > 16                                # more taxa than 16 cell slots
    monkeypatch.setenv(var, value)
    code, st, out, tab = run(db, [tree], data, tmp_path, 1)
    assert code == lib.E_PROFILE and not tab.exists() and out.read_bytes() == want
    msg = lib.load().utree_last_hip_error()
    assert word in msg and str(tab).encode() in msg
    monkeypatch.delenv(var)
    code, st, out, tab = run(db, [tree], data, tmp_path, 1)
    assert code == lib.OK and tab.read_bytes() == table


# ---- 5. the pipelines agree --------------------------------------------------------------------------------------------------------------
def test_device_host_and_small_chunks_agree(torch_cuda, tmp_path, monkeypatch):
    db, tree = tree_for("toy")
    data, want, names, table = renamed("toy", 1, "round_robin")
    code, st, out, tab = run(db, [tree], data, tmp_path, 1, tag="host", input_format=lib.INPUT_FASTA_MULTILINE)
    assert code == lib.OK and st.pipeline == 0 and out.read_bytes() == want and tab.read_bytes() == table
    monkeypatch.setenv("UTREE_HOST_TEXT", "1")
    code, st, out, tab = run(db, [tree], data, tmp_path, 1, tag="host2")
    assert code == lib.OK and st.pipeline == 0 and out.read_bytes() == want and tab.read_bytes() == table
    monkeypatch.delenv("UTREE_HOST_TEXT")
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "4000")
    assert len(data) > 200 * 4000
    code, st, out, tab = run(db, [tree], data, tmp_path, 1, tag="small")
    assert code == lib.OK and st.pipeline == 1 and out.read_bytes() == want and tab.read_bytes() == table
    data, want, names, table = renamed("toy", 1, "blocks")
    code, st, out, tab = run(db, [tree], data, tmp_path, 1, tag="smallb")
    assert code == lib.OK and st.pipeline == 1 and out.read_bytes() == want and tab.read_bytes() == table


def test_two_handles_on_one_card(torch_cuda, tmp_path, monkeypatch):
    torch = torch_cuda
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "20000")
    db, tree = tree_for("toy")
    ptr, used = tree.image_ptr()

    class _Raw:
        __cuda_array_interface__ = {"shape": (used,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    c = torch.empty(used + 4096, dtype=torch.uint8, device="cuda:0")[4096:]
    c.copy_(torch.as_tensor(_Raw(), device="cuda:0"))
    torch.cuda.synchronize()
    trees = [tree, DeviceTree.attach(db, c, 0)]
    data, want, names, table = renamed("toy", 1, "round_robin")
    try:
        for host in ("", "1"):                                    # the device pipeline, then the host pipeline's sharding
            if host:
                monkeypatch.setenv("UTREE_HOST_TEXT", host)
            code, st, out, tab = run(db, trees, data, tmp_path, 1)
            assert code == lib.OK and out.read_bytes() == want and tab.read_bytes() == table
    finally:
        trees[1].close()


@pytest.mark.parametrize("interleaved", [False, True])
def test_pairs_take_mate_ones_name(torch_cuda, interleaved, tmp_path, monkeypatch):
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "30000")
    db, tree = tree_for("toy")
    P = pairs_ref.Pairs("toy")
    old = list(P.names1)
    new = sr.round_robin_names(P.n, sr.SEVEN)
    gold = pairs_ref.golden("toy", 1)
    _, want = sr.rename_reads(b"\n".join(b">" + o + b"\n" for o in old), gold, old, new)
    P.names1 = new
    reads, mates = (P.interleaved_fasta(), None) if interleaved else (P.reads_fasta(), P.mates_fasta())
    rp, mp, out, tab = tmp_path / "r.fa", tmp_path / "m.fa", tmp_path / "o.txt", tmp_path / "s.tsv"
    rp.write_bytes(reads)
    if mates is not None:
        mp.write_bytes(mates)
    code, st = search_gg(db, [tree], str(rp), str(out), rc=True, threads=4, mates=str(mp) if mates is not None else None, interleaved=interleaved,
                         samples=str(tab))
    assert code == lib.OK and st.n_reads == P.n and out.read_bytes() == want
    assert tab.read_bytes() == sr.samples_ref(want, new, P.n)          # counts are per pair, ids mate 1's


# ---- 6. with the other reports -----------------------------------------------------------------------------------------------------------
def test_rows_sum_to_the_profiles_assigned(torch_cuda, tmp_path):
    db, tree = tree_for("vote")
    data, want, names, table = renamed("vote", 0, "round_robin")
    prof = tmp_path / "p.tsv"
    code, st, out, tab = run(db, [tree], data, tmp_path, 0, profile=str(prof))
    assert code == lib.OK and tab.read_bytes() == table
    rows = sr.parse_table(table)[6]
    assigned = {}
    for ln in prof.read_bytes().split(b"\n")[2:-1]:
        f = ln.rsplit(b"\t", 2)
        if int(f[1]):
            assigned[f[0]] = int(f[1])
    assert {t: sum(r) for t, r in rows.items()} == assigned


def test_hitmap_and_redistribution_are_what_they_were(torch_cuda, tmp_path):
    db, tree = tree_for("toy")
    data, want, names, table = renamed("toy", 0, "blocks")
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    files = {}
    for tag, kw in (("a", {}), ("b", {"samples": str(tmp_path / "b.samples")})):
        hm, rd = tmp_path / (tag + ".hm"), tmp_path / (tag + ".rd")
        code, st = search_gg(db, [tree], str(fa), str(tmp_path / (tag + ".txt")), threads=4, hitmap=str(hm), redistribute=str(rd), **kw)
        assert code == lib.OK and st.pipeline == 0
        files[tag] = ((tmp_path / (tag + ".txt")).read_bytes(), hm.read_bytes(), (tmp_path / (tag + ".hm.labels")).read_bytes(), rd.read_bytes())
    assert files["a"] == files["b"] and files["a"][0] == want
    assert (tmp_path / "b.samples").read_bytes() == table


# ---- 7. failures -------------------------------------------------------------------------------------------------------------------------
def test_a_failed_search_leaves_no_table(torch_cuda, tmp_path):
    cases = json.load(open(os.path.join(util.GOLD, "edge_cases.json")))
    db, tree = tree_for("toy")
    bad = 0
    for nm, c in sorted(cases.items()):
        data = bytes.fromhex(c["input_hex"])
        code, st, out, tab = run(db, [tree], data, tmp_path, c["rc"])
        want = bytes.fromhex(c["output_hex"])
        assert out.read_bytes() == want, nm
        if c["exit"] == 0:
            assert code == lib.OK, nm
            assert tab.read_bytes() == sr.samples_ref(want, fasta_names(data), st.n_reads), nm
        else:
            bad += 1
            assert code != lib.OK and not tab.exists(), nm
    assert bad > 0


# ---- 8. the command line -----------------------------------------------------------------------------------------------------------------
def test_cli(torch_cuda, tmp_path):
    ctr = util.fixture_ctr("toy")
    data, want, names, table = renamed("toy", 1, "round_robin")
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    env = dict(os.environ, UTREE_GPUS="1")
    for v in ("UTREE_SAMPLE_TABLE", "UTREE_SAMPLE_DELIM", "UTREE_SAMPLE_CAPACITY", "UTREE_SAMPLE_CELLS"):
        env.pop(v, None)
    cmd = lambda o: [lib.CLI_PATH, ctr, str(fa), str(tmp_path / o), "4", "RC"]
    plain = subprocess.run(cmd("a.txt"), capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0 and (tmp_path / "a.txt").read_bytes() == want
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.txt", "in.fa"]                  # without the variable: no file
    tab = tmp_path / "s.tsv"
    withs = subprocess.run(cmd("b.txt"), capture_output=True, env=dict(env, UTREE_SAMPLE_TABLE=str(tab)), timeout=300)
    assert withs.returncode == 0 and withs.stdout == plain.stdout and (tmp_path / "b.txt").read_bytes() == want
    assert tab.read_bytes() == table
    dot = subprocess.run(cmd("c.txt"), capture_output=True, env=dict(env, UTREE_SAMPLE_TABLE=str(tab), UTREE_SAMPLE_DELIM="."), timeout=300)
    assert dot.returncode == 0 and tab.read_bytes() == sr.samples_ref(want, names, len(names), b".")
    bad = subprocess.run(cmd("d.txt"), capture_output=True, env=dict(env, UTREE_SAMPLE_TABLE=str(tmp_path / "no" / "dir" / "s.tsv")), timeout=300)
    assert bad.returncode == 1 and b"sample table" in bad.stderr and b"Tree read." not in bad.stdout and not (tmp_path / "d.txt").exists()
    for d in ("\t", " ", "ab", ""):
        r = subprocess.run(cmd("e.txt"), capture_output=True, env=dict(env, UTREE_SAMPLE_TABLE=str(tab), UTREE_SAMPLE_DELIM=d), timeout=300)
        assert r.returncode == 1 and b"UTREE_SAMPLE_DELIM" in r.stderr and b"Tree read." not in r.stdout, d
    tab.unlink()
    small = subprocess.run(cmd("f.txt"), capture_output=True, env=dict(env, UTREE_SAMPLE_TABLE=str(tab), UTREE_SAMPLE_CAPACITY="4"), timeout=300)
    assert small.returncode == 1 and small.stdout == plain.stdout and (tmp_path / "f.txt").read_bytes() == want and not tab.exists()
    err = [ln for ln in small.stderr.split(b"\n") if ln.startswith(b"ERROR")]
    assert len(err) == 1 and b"UTREE_SAMPLE_CAPACITY" in err[0] and b"delimiter" in err[0]


def test_cli_rank_specific(torch_cuda, tmp_path):
    tag = "toy_rank" if "toy_rank" in RANK else sorted(RANK)[0]
    v = RANK[tag]
    data = util.fixture_bytes(v["reads"] + "_reads.fa.gz")
    gold = util.fixture_bytes(tag + ".txt.gz")
    old = fasta_names(data)
    new = sr.round_robin_names(len(old), sr.SEVEN)
    data2, want = sr.rename_reads(data, gold, old, new)
    fa, tab = tmp_path / "in.fa", tmp_path / "s.tsv"
    fa.write_bytes(data2)
    sl, sp, tol = v["params"]
    env = dict(os.environ, UTREE_GPUS="1", UTREE_SLACK=str(sl), UTREE_SPARSITY=str(sp), UTREE_TOLERANCE=str(tol), UTREE_SAMPLE_TABLE=str(tab))
    r = subprocess.run([lib.RANK_CLI_PATH, util.fixture_ctr(v["db"]), str(fa), str(tmp_path / "o.txt"), "4"] + (["RC"] if v["rc"] else []),
                       capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes() == want
    assert tab.read_bytes() == sr.samples_ref(want, new, len(new))
