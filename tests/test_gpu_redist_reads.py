"""GPU tests of each read's redistributed label (csrc/redist_kernels.hip: redist_add_k<true>, redist_winner_k, redist_assign_k; csrc/redist.c;
UTREE_REDISTRIBUTE_READS): every read's key, assigned after a solve, must give the label and the number of candidates that
tests/redist_reads_ref.py gives -- the contract restated with the CPU oracle, pinned in tests/test_redist_reads_cpu.py --, the candidate sets and
the per-read results must stay what they were, and the whole-file report must be the reference's bytes.  All comparisons are exact.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import gzip
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pairs_ref
import redist_ref
import redist_reads_ref
from test_coverage_cpu import fixture_seqs
from test_gpu_redist import device_reads, mixed_reads, mixed_reference, tree_for, want_multiset
from test_redist_cpu import reference_sets
from test_redist_reads_cpu import reference_assign
from utree_amd import lib
from utree_amd.search import DeviceTree, search_gg
import util

N_READS = 4000
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def u32(t):
    """a device int32 tensor's bit patterns as a host uint32 array"""
    return t.cpu().numpy().view(np.uint32)


def want_arrays(labels, ncand):
    return np.array([NONE if l is None else l for l in labels], dtype=np.uint32), np.array(ncand, dtype=np.uint32)


def entries_dict(e, field):
    return {int(l): int(v) for l, v in zip(e["label"], e[field]) if v}


def check_against_solve(rd, keys, sets, n_reads, passes=(1, 3, 100), solved=None):
    """for every pass cap: solve, assign, and each read has the reference's label and candidates; the histograms are the solve's own figures"""
    for mp in passes:
        labels, ncand, _ = redist_reads_ref.assign(sets, n_reads, mp)
        wl, wc = want_arrays(labels, ncand)
        e, _, _ = (solved or rd).solve(mp)
        label, nc = rd.assign(keys, solved=solved)
        gl, gc = u32(label), u32(nc)
        assert np.array_equal(gl, wl) and np.array_equal(gc, wc), mp
        hit = gl != NONE
        assert dict(Counter(gl[hit].tolist())) == entries_dict(e, "assigned")
        assert dict(Counter(gl[gc == 1].tolist())) == entries_dict(e, "unique")
        assert (gc[~hit] == 0).all()


# ---- 1. keys through every record form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rc", [(n, r) for n in ("toy", "vote", "ix32", "k64", "k64ix32", "k16") for r in (0, 1)])
def test_keys_assign_the_reference_labels(torch_cuda, name, rc):
    torch = torch_cuda
    db, tree = tree_for(name)
    seqs = fixture_seqs(name)[:N_READS]
    sets, _ = reference_sets(name, rc, N_READS)
    t = device_reads(torch, seqs)
    plain = tree.classify(*t, rc=bool(rc))
    torch.cuda.synchronize()
    rd = tree.redistribution(1 << 14)
    try:
        keys = torch.full((len(seqs),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        got = rd.classify(*t, rc=bool(rc), keys=keys)
        torch.cuda.synchronize()
        tree.poll()
        assert torch.equal(got, plain)                              # bit for bit DeviceTree.classify's
        ms, n_reads, _ = rd.sets()
        assert n_reads == len(seqs) and ms == want_multiset(sets)    # the sets are those of the pass without keys
        k = u32(keys)
        single = np.array([len(s) == 1 for s in sets])
        assert (k[np.array([len(s) == 0 for s in sets])] == NONE).all()
        assert np.array_equal(k[single], np.array([s[0] for s in sets if len(s) == 1], dtype=np.uint32))
        assert (k[np.array([len(s) > 1 for s in sets])] >= 0x80000000).all()
        check_against_solve(rd, keys, sets, len(seqs))
    finally:
        rd.close()


@pytest.mark.parametrize("rc,lane_pass", [(0, "1"), (1, "1"), (0, "0"), (1, "0")])
def test_mixed_length_batch(torch_cuda, rc, lane_pass, monkeypatch):
    """test_gpu_redist.py's batch: lengths that finish in classify_long_k (records that are finished when the pass sees them)"""
    torch = torch_cuda
    monkeypatch.setenv("UTREE_LANE_PASS", lane_pass)
    db, tree = tree_for("toy")
    seqs = mixed_reads()
    sets = mixed_reference(rc)
    t = device_reads(torch, seqs)
    plain = tree.classify(*t, rc=bool(rc))
    torch.cuda.synchronize()
    rd = tree.redistribution(1 << 12)
    try:
        keys = torch.empty(len(seqs), dtype=torch.int32, device="cuda")
        got = rd.classify(*t, rc=bool(rc), keys=keys)
        torch.cuda.synchronize()
        tree.poll()
        assert torch.equal(got, plain)
        assert rd.sets()[0] == want_multiset(sets)
        check_against_solve(rd, keys, sets, len(seqs), passes=(1, 100))
    finally:
        rd.close()


# ---- 2. rounds of a workgroup and its second queue --------------------------------------------------------------------------------------
def repeated_reads(torch, seqs, n):
    """n reads on the device: `seqs` over and over (built there from one copy)"""
    bases, off, ln = device_reads(torch, seqs)
    m, total = len(seqs), int(ln.sum().item())
    reps = (n + m - 1) // m
    big = bases[:total].repeat(reps)
    big = torch.cat([big, torch.zeros(1, dtype=torch.uint8, device="cuda")])
    offs = (off[None, :] + (torch.arange(reps, device="cuda", dtype=torch.int64) * total)[:, None]).reshape(-1)[:n].contiguous()
    lens = ln.repeat(reps)[:n].contiguous()
    return big, offs, lens, total * (n // m) + int(ln[:n % m].sum().item())


@pytest.mark.parametrize("case", ["all reads, two rounds", "ambiguous reads, three rounds"])
def test_rounds_and_the_second_queue(torch_cuda, case):
    torch = torch_cuda
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    db, tree = tree_for("toy")
    seqs = fixture_seqs("toy")[:N_READS]
    sets, _ = reference_sets("toy", 0, N_READS)
    if case.startswith("ambiguous"):
        keep = [i for i, s in enumerate(sets) if len(s) > 1]          # every read goes through rd_multi
        seqs, sets = [seqs[i] for i in keep], [sets[i] for i in keep]
        n = 2 * 4096 * n_cu + 3        # 8193 reads a workgroup: the second queue fills in two rounds, is emptied mid-way and again at the end
    else:
        n = 4096 * n_cu + 37           # 4097 reads a workgroup: a second round, and the second queue carries over into it
    m = len(seqs)
    assert m > 1000
    bases, off, ln, total = repeated_reads(torch, seqs, n)
    # (the default capacity: every lane that meets a free slot reserves arena space for its set before it claims the slot, and hundreds of
    # copies of each set arrive at once here)
    rd = tree.redistribution(1 << 22)
    try:
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        rd.classify(bases, off, ln, rc=False, total_bases=total, max_len=int(ln.max().item()), keys=keys)
        torch.cuda.synchronize()
        tree.poll()
        full, part = redist_ref.multiset(sets), redist_ref.multiset(sets[:n % m])
        want = {s: (n // m) * c + part.get(s, 0) for s, c in full.items()}
        ms, n_reads, _ = rd.sets()
        assert n_reads == n and ms == want
        rep_sets = [sets[i % m] for i in range(n)]
        labels, ncand, _ = redist_reads_ref.assign(rep_sets, n, 100)
        wl, wc = want_arrays(labels[:m], ncand[:m])
        # (a read's label depends on its set alone, so the first m reads' labels repeat; that they do is asserted, not assumed)
        assert all(labels[i] == labels[i % m] for i in range(m, n, 997))
        idx = torch.arange(n, device="cuda") % m
        e, _, _ = rd.solve(100)
        label, nc = rd.assign(keys)
        assert torch.equal(label, torch.from_numpy(wl.view(np.int32)).cuda()[idx]) and torch.equal(nc, torch.from_numpy(wc.view(np.int32)).cuda()[idx])
        hist = torch.bincount(label[label != -1].long(), minlength=db.info.n_labels).cpu().numpy()
        assert {int(l): int(v) for l, v in enumerate(hist) if v} == entries_dict(e, "assigned")
    finally:
        rd.close()


@pytest.mark.parametrize("n", [1, 4097])
def test_small_batches(torch_cuda, n):
    torch = torch_cuda
    db, tree = tree_for("toy")
    seqs = fixture_seqs("toy")[:N_READS]
    sets, _ = reference_sets("toy", 0, N_READS)
    if n == 1:
        first = next(i for i, s in enumerate(sets) if len(s) > 1)    # the one read is an ambiguous one
        seqs, sets = [seqs[first]], [sets[first]]
    else:
        seqs, sets = (seqs + seqs)[:n], (sets + sets)[:n]
    rd = tree.redistribution(1 << 12)
    try:
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        rd.classify(*device_reads(torch, seqs), rc=False, keys=keys)
        torch.cuda.synchronize()
        tree.poll()
        assert rd.sets()[0] == want_multiset(sets)
        check_against_solve(rd, keys, sets, n, passes=(1, 100))
    finally:
        rd.close()


# ---- 3. two handles on one card ---------------------------------------------------------------------------------------------------------
def second_tree(torch, db, tree):
    ptr, used = tree.image_ptr()

    class _Raw:
        __cuda_array_interface__ = {"shape": (used,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    c = torch.empty(used + 4096, dtype=torch.uint8, device="cuda:0")[4096:]
    c.copy_(torch.as_tensor(_Raw(), device="cuda:0"))
    torch.cuda.synchronize()
    return DeviceTree.attach(db, c, 0)


def test_two_handles_merge_and_assign(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    tree2 = second_tree(torch, db, tree)
    seqs = fixture_seqs("toy")[:N_READS]
    sets, _ = reference_sets("toy", 0, N_READS)
    half = 1700
    a, b = tree.redistribution(1 << 12), tree2.redistribution(1 << 13)
    try:
        ka = torch.empty(half, dtype=torch.int32, device="cuda")
        kb = torch.empty(N_READS - half, dtype=torch.int32, device="cuda")
        a.classify(*device_reads(torch, seqs[:half]), rc=False, keys=ka)
        b.classify(*device_reads(torch, seqs[half:]), rc=False, keys=kb)
        torch.cuda.synchronize()
        tree.poll(); tree2.poll()
        # A alone, before the merge: its own reads under its own tally
        check_against_solve(a, ka, sets[:half], half, passes=(100,))
        a.merge(b)
        assert a.sets()[0] == want_multiset(sets)
        with pytest.raises(lib.UtreeError) as err:                  # the merge ended A's solved state
            a.assign(ka)
        assert err.value.code == lib.E_ARG
        for mp in (1, 100):
            labels, ncand, _ = redist_reads_ref.assign(sets, N_READS, mp)
            wl, wc = want_arrays(labels, ncand)
            a.solve(mp)
            la, ca = a.assign(ka)                                   # A's keys, taken before the merge, are still right after it
            lb, cb = b.assign(kb, solved=a)                         # B's keys meet B's table under A's tally
            assert np.array_equal(np.concatenate([u32(la), u32(lb)]), wl) and np.array_equal(np.concatenate([u32(ca), u32(cb)]), wc)
            lb2, _ = b.assign(kb, solved=a)                         # (the second call of a solve computes no winners again)
            assert torch.equal(lb, lb2)
        with pytest.raises(lib.UtreeError) as err:                  # B itself was never solved
            b.assign(kb)
        assert err.value.code == lib.E_ARG
    finally:
        a.close(); b.close(); tree2.close()


# ---- 4. four streams add with keys at once ----------------------------------------------------------------------------------------------
def test_four_streams_add_with_keys_at_once(torch_cuda):
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
    keys = [torch.empty(len(seqs), dtype=torch.int32, device="cuda") for _ in range(4)]
    rd = tree.redistribution(1 << 12)
    try:
        torch.cuda.synchronize()
        for s, w, o, k in zip(streams, ws, outs, keys):
            with torch.cuda.stream(s):
                rd.classify(*t, rc=False, total_bases=total, max_len=mx, out=o, workspace=w, keys=k)
        torch.cuda.synchronize()
        tree.poll()
        ms, n_reads, _ = rd.sets()
        assert n_reads == 4 * N_READS and ms == {s: 4 * n for s, n in want_multiset(sets).items()}
        assert all(torch.equal(k, keys[0]) for k in keys[1:])        # equal sets share a slot, whichever stream claimed it
        labels, ncand, _ = redist_reads_ref.assign(sets * 4, 4 * N_READS, 100)
        wl, wc = want_arrays(labels[:N_READS], ncand[:N_READS])
        assert labels[N_READS:] == labels[:N_READS] * 3
        rd.solve(100)
        for k in keys:
            label, nc = rd.assign(k)
            assert np.array_equal(u32(label), wl) and np.array_equal(u32(nc), wc)
    finally:
        rd.close()


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------------
def test_assign_needs_a_solve_that_still_stands(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    seqs = fixture_seqs("toy")[:N_READS]
    sets, _ = reference_sets("toy", 0, N_READS)
    t = device_reads(torch, seqs[:1000])
    rd = tree.redistribution(1 << 12)
    try:
        keys = torch.empty(1000, dtype=torch.int32, device="cuda")
        rd.classify(*t, rc=False, keys=keys)
        with pytest.raises(lib.UtreeError) as err:                  # before any solve
            rd.assign(keys)
        assert err.value.code == lib.E_ARG
        rd.solve(100)
        rd.assign(keys)
        keys2 = torch.empty(1000, dtype=torch.int32, device="cuda")
        rd.classify(*device_reads(torch, seqs[1000:2000]), rc=False, keys=keys2)
        with pytest.raises(lib.UtreeError) as err:                  # after a further classify
            rd.assign(keys)
        assert err.value.code == lib.E_ARG
        torch.cuda.synchronize()
        rd.solve(100)                                               # a new solve: both batches' keys, under the tally of both
        labels, ncand, _ = redist_reads_ref.assign(sets[:2000], 2000, 100)
        wl, wc = want_arrays(labels, ncand)
        l1, c1 = rd.assign(keys)
        l2, c2 = rd.assign(keys2)
        assert np.array_equal(np.concatenate([u32(l1), u32(l2)]), wl) and np.array_equal(np.concatenate([u32(c1), u32(c2)]), wc)
        l0, c0 = rd.assign(keys[:0])                                # no keys: nothing
        assert l0.numel() == 0
        rd.reset()
        with pytest.raises(lib.UtreeError):
            rd.assign(keys)
    finally:
        rd.close()


# ---- 6. keys that name nothing ------------------------------------------------------------------------------------------------------------
def test_refused_keys(torch_cuda):
    """KEY_NONE, a label equal to n_labels and a free slot of a table of 16 slots.  (A slot index beyond the table is refused by the same
    comparison in front of the same load; it is not exercised here.)"""
    torch = torch_cuda
    db, tree = tree_for("toy")
    seqs = fixture_seqs("toy")[:N_READS]
    sets, _ = reference_sets("toy", 0, N_READS)
    amb = [i for i, s in enumerate(sets) if len(s) > 1][:3]
    few = [seqs[i] for i in amb]
    rd = tree.redistribution(16)
    try:
        keys = torch.empty(len(few), dtype=torch.int32, device="cuda")
        rd.classify(*device_reads(torch, few), rc=False, keys=keys)
        torch.cuda.synchronize()
        tree.poll()
        assert len(rd.sets()[0]) <= 3
        used = {int(k) & 0x7FFFFFFF for k in u32(keys)}
        assert all(int(k) >= 0x80000000 for k in u32(keys)) and all(s < 16 for s in used)
        free = next(s for s in range(16) if s not in used)          # the complement of the occupied slots
        nl = db.info.n_labels
        probe = np.array([NONE, nl, 0x80000000 | free, int(u32(keys)[0]), 0], dtype=np.uint32)
        rd.solve(100)
        label, nc = rd.assign(torch.from_numpy(probe.view(np.int32)).cuda())
        gl, gc = u32(label), u32(nc)
        assert (gl[0], gc[0]) == (NONE, 0)
        assert (gl[1], gc[1]) == (NONE, NONE)
        assert (gl[2], gc[2]) == (NONE, NONE)
        assert gl[3] in sets[amb[0]] and gc[3] == len(sets[amb[0]])
        assert (gl[4], gc[4]) == (0, 1)
    finally:
        rd.close()


# ---- 7. the whole-file search and the command line ----------------------------------------------------------------------------------------
ENV_VARS = ("UTREE_REDISTRIBUTE", "UTREE_REDISTRIBUTE_READS", "UTREE_REDIST_PASSES", "UTREE_REDIST_CAPACITY", "UTREE_PROFILE", "UTREE_COVERAGE",
            "UTREE_MATES", "UTREE_INTERLEAVED", "UTREE_HITMAP", "UTREE_INPUT", "UTREE_CHUNK_BYTES", "UTREE_HOST_TEXT")


def run_cli(cli, ctr, fa, out, rc, **env):
    base = dict(os.environ, UTREE_GPUS="1")
    for v in ENV_VARS:
        base.pop(v, None)
    return subprocess.run([cli, ctr, str(fa), str(out), "4"] + (["RC"] if rc else []), capture_output=True, env=dict(base, **env), timeout=300)


def toy_file(tmp_path):
    data = util.fixture_bytes("toy_reads.fa.gz")
    head = b"\n".join(data.split(b"\n")[:2 * N_READS]) + b"\n"                       # the first N_READS records
    fa = tmp_path / "reads.fa"
    fa.write_bytes(head)
    return fa, head


def toy_reference(max_passes=100):
    """(reads file, redistribution file) of toy's first reads, RC"""
    labels, ncand, texts = reference_assign("toy", 1, N_READS, max_passes)
    names = util.parse_fasta(util.fixture_bytes("toy_reads.fa.gz"))[0][:N_READS]
    sets, _ = reference_sets("toy", 1, N_READS)
    a, u, p, amb, _ = redist_ref.solve(sets, N_READS, max_passes)
    return redist_reads_ref.reads_file(names, labels, ncand, texts), redist_ref.redist_file(a, u, texts, N_READS, amb, p)


def check_files(reads_bytes, out_bytes, table_bytes=None):
    """cut -f1 of both files is the same; the reads file's histogram by label text is the table's `assigned`, its rows with 1 candidate `unique`"""
    rows = [l.split(b"\t") for l in reads_bytes.split(b"\n") if l]
    assert all(len(r) == 3 for r in rows)
    assert [r[0] for r in rows] == [l.split(b"\t")[0] for l in out_bytes.split(b"\n") if l]
    if table_bytes is not None:
        table = [l.split(b"\t") for l in table_bytes.split(b"\n") if l and not l.startswith(b"#")]
        assert dict(Counter(r[1] for r in rows)) == {t[0]: int(t[1]) for t in table if int(t[1])}
        assert dict(Counter(r[1] for r in rows if r[2] == b"1")) == {t[0]: int(t[2]) for t in table if int(t[2])}


def no_spool(tmp_path):
    return not list(tmp_path.glob("*.spool"))


def test_search_gg_writes_the_reference_file(torch_cuda, tmp_path, monkeypatch):
    torch = torch_cuda
    db, tree = tree_for("toy")
    fa, data = toy_file(tmp_path)
    want_reads, want_table = toy_reference()
    plain_out, q, red = tmp_path / "a.txt", tmp_path / "q.tsv", tmp_path / "r.tsv"
    code, st = search_gg(db, [tree], str(fa), str(plain_out), rc=True, threads=4, redistribute=str(red))
    assert code == lib.OK and st.pipeline == 1 and red.read_bytes() == want_table
    # with the table: one solve serves both files
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "b.txt"), rc=True, threads=4, redistribute=str(red), redistribute_reads=str(q))
    assert code == lib.OK and st.n_reads == N_READS and st.pipeline == 0
    assert (tmp_path / "b.txt").read_bytes() == plain_out.read_bytes() and red.read_bytes() == want_table
    assert q.read_bytes() == want_reads and no_spool(tmp_path)
    check_files(q.read_bytes(), plain_out.read_bytes(), red.read_bytes())
    # alone, one pass, small chunks (several batches)
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "40000")
    red.unlink()
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "c.txt"), rc=True, threads=4, redistribute_reads=str(q), redist_passes=1)
    assert code == lib.OK and st.pipeline == 0 and not red.exists() and no_spool(tmp_path)
    assert q.read_bytes() == toy_reference(1)[0] != want_reads and (tmp_path / "c.txt").read_bytes() == plain_out.read_bytes()
    # two device handles on one card: each key meets its own handle's table, under the merged tally
    tree2 = second_tree(torch, db, tree)
    try:
        code, st = search_gg(db, [tree, tree2], str(fa), str(tmp_path / "d.txt"), rc=True, threads=4, redistribute=str(red), redistribute_reads=str(q))
        assert code == lib.OK and q.read_bytes() == want_reads and red.read_bytes() == want_table and no_spool(tmp_path)
        assert (tmp_path / "d.txt").read_bytes() == plain_out.read_bytes()
    finally:
        tree2.close()
    # a file that cannot be written: the search's output, UTREE_E_PROFILE, the cause by name
    code, st = search_gg(db, [tree], str(fa), str(tmp_path / "e.txt"), rc=True, threads=4, redistribute_reads="/dev/full")
    assert code == lib.E_PROFILE and b"redistributed reads /dev/full" in lib.load().utree_last_hip_error()
    assert (tmp_path / "e.txt").read_bytes() == plain_out.read_bytes() and not os.path.exists("/dev/full.spool")


def test_cli_file_and_unchanged_output(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    fa, data = toy_file(tmp_path)
    want_reads, want_table = toy_reference()
    red, prof, hm, q = tmp_path / "r.tsv", tmp_path / "p.tsv", tmp_path / "h.txt", tmp_path / "q.tsv"
    plain = run_cli(cli, ctr, fa, tmp_path / "a.txt", 1, UTREE_REDISTRIBUTE=str(red), UTREE_PROFILE=str(prof), UTREE_HITMAP=str(hm))
    assert plain.returncode == 0 and not q.exists()
    keep = {p.name: p.read_bytes() for p in (red, prof, hm, tmp_path / "h.txt.labels")}
    withq = run_cli(cli, ctr, fa, tmp_path / "b.txt", 1, UTREE_REDISTRIBUTE=str(red), UTREE_PROFILE=str(prof), UTREE_HITMAP=str(hm),
                    UTREE_REDISTRIBUTE_READS=str(q))
    assert withq.returncode == 0 and withq.stdout == plain.stdout
    assert (tmp_path / "b.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    assert {p.name: p.read_bytes() for p in (red, prof, hm, tmp_path / "h.txt.labels")} == keep      # the other reports, byte for byte
    assert q.read_bytes() == want_reads and red.read_bytes() == want_table and no_spool(tmp_path)
    check_files(q.read_bytes(), (tmp_path / "b.txt").read_bytes(), red.read_bytes())
    # the variable alone, one pass
    red.unlink()
    one = run_cli(cli, ctr, fa, tmp_path / "c.txt", 1, UTREE_REDISTRIBUTE_READS=str(q), UTREE_REDIST_PASSES="1")
    assert one.returncode == 0 and q.read_bytes() == toy_reference(1)[0] and not red.exists() and no_spool(tmp_path)
    assert (tmp_path / "c.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()


def test_cli_mates_lines_are_those_of_the_joined_queries(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    P = pairs_ref.Pairs("toy")
    n = 1500
    rp, mp = tmp_path / "r1.fa", tmp_path / "r2.fa"
    rp.write_bytes(P.reads_fasta(n)); mp.write_bytes(P.mates_fasta(n))
    red, q = tmp_path / "r.tsv", tmp_path / "q.tsv"
    r = run_cli(cli, ctr, rp, tmp_path / "a.txt", 1, UTREE_REDISTRIBUTE=str(red), UTREE_REDISTRIBUTE_READS=str(q), UTREE_MATES=str(mp))
    assert r.returncode == 0 and no_spool(tmp_path)
    sets, texts = redist_ref.candidate_sets(ctr, P.joined_seqs()[:n], True)
    labels, ncand, _ = redist_reads_ref.assign(sets, n, 100)
    assert q.read_bytes() == redist_reads_ref.reads_file(P.names1[:n], labels, ncand, texts)      # one line per pair, under mate 1's name
    plain = run_cli(cli, ctr, rp, tmp_path / "b.txt", 1, UTREE_REDISTRIBUTE=str(red), UTREE_MATES=str(mp))
    assert plain.stdout == r.stdout and (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()
    check_files(q.read_bytes(), (tmp_path / "a.txt").read_bytes(), red.read_bytes())


def test_cli_gzipped_fastq(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    fa, data = toy_file(tmp_path)
    names, off, ln = util.parse_fasta(data)
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(gzip.compress(b"".join(b"@%s\n%s\n+\n%s\n" % (nm, data[int(o):int(o) + int(l)], b"I" * int(l)) for nm, o, l in zip(names, off, ln)), 1))
    q = tmp_path / "q.tsv"
    r = run_cli(cli, ctr, fq, tmp_path / "a.txt", 1, UTREE_REDISTRIBUTE_READS=str(q), UTREE_INPUT="fastq", UTREE_CHUNK_BYTES="60000")
    assert r.returncode == 0 and q.read_bytes() == toy_reference()[0] and no_spool(tmp_path)
    check_files(q.read_bytes(), (tmp_path / "a.txt").read_bytes())


# ---- 8. failures --------------------------------------------------------------------------------------------------------------------------
def test_cli_failures(torch_cuda, tmp_path):
    cli, ctr = lib.CLI_PATH, util.fixture_ctr("toy")
    fa, data = toy_file(tmp_path)
    q = tmp_path / "q.tsv"
    plain = run_cli(cli, ctr, fa, tmp_path / "a.txt", 1)
    # a table too small: the usual stdout, exit 1, the knob by name, no file, no spool
    small = run_cli(cli, ctr, fa, tmp_path / "b.txt", 1, UTREE_REDISTRIBUTE_READS=str(q), UTREE_REDIST_CAPACITY="16")
    assert small.returncode == 1 and small.stdout == plain.stdout and b"UTREE_REDIST_CAPACITY" in small.stderr
    assert not q.exists() and no_spool(tmp_path) and (tmp_path / "b.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    # a malformed record mid-file: exit 2, the path as it was, no spool
    lines = data.split(b"\n")
    lines[2 * 2500] = b"no header here"
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b"\n".join(lines))
    q.write_bytes(b"as it was\n")
    broken = run_cli(cli, ctr, bad, tmp_path / "c.txt", 1, UTREE_REDISTRIBUTE_READS=str(q))
    assert broken.returncode == 2 and q.read_bytes() == b"as it was\n" and no_spool(tmp_path)
    q.unlink()
    # an unwritable path: exit 1 before the search
    nowhere = run_cli(cli, ctr, fa, tmp_path / "d.txt", 1, UTREE_REDISTRIBUTE_READS=str(tmp_path / "no" / "dir" / "q.tsv"))
    assert nowhere.returncode == 1 and b"redistributed reads" in nowhere.stderr and not (tmp_path / "d.txt").exists() and not (tmp_path / "no").exists()
    assert b"Tree read." not in nowhere.stdout


def test_rank_specific_cli_ignores_the_variable(torch_cuda, tmp_path):
    ctr, fa = util.fixture_ctr("toy"), util.fixture_reads_path("toy")
    plain = run_cli(lib.RANK_CLI_PATH, ctr, fa, tmp_path / "a.txt", 0)
    withq = run_cli(lib.RANK_CLI_PATH, ctr, fa, tmp_path / "b.txt", 0, UTREE_REDISTRIBUTE_READS=str(tmp_path / "no" / "dir" / "q.tsv"))
    assert plain.returncode == withq.returncode == 0 and plain.stdout == withq.stdout
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes() == util.fixture_bytes("toy_rank.txt.gz")
    assert not (tmp_path / "no").exists() and no_spool(tmp_path)
