"""GPU tests of the per-taxon read-count profile (csrc/profile_kernels.hip, csrc/profile.c, UTREE_PROFILE): every profile must equal
tests/profile_ref.py applied to the per-read output the reference writes, and the per-read output must stay what it was.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import gzip
import json
import os
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, PROFILE_ENTRY_DTYPE, frame_fasta, search_gg, search_rank, write_profile
from profile_ref import fasta_names, profile_from_taxa, profile_ref
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


def gg_profile_run(db, trees, data, tmp_path, rc, **kw):
    fa, out, prof = tmp_path / "in.fa", tmp_path / "out.txt", tmp_path / "profile.tsv"
    fa.write_bytes(data)
    for p in (out, prof):
        if p.exists():
            p.unlink()
    code, st = search_gg(db, trees, str(fa), str(out), rc=rc, threads=4, profile=str(prof), **kw)
    return code, st, out, prof


GG = [("toy", 0), ("toy", 1), ("k64", 0), ("k64", 1), ("ix32", 0), ("ix32", 1), ("k64ix32", 0), ("k64ix32", 1), ("k16", 0), ("k16", 1),
      ("vote", 0), ("kat", 0), ("katq", 0), ("katq2", 0), ("generic", 0)]


@pytest.mark.parametrize("name,rc", GG)
def test_gg_golden_profiles(torch_cuda, name, rc, tmp_path):
    db, tree = tree_for(name)
    data = util.fixture_bytes(util.READS_OF.get(name, name) + "_reads.fa.gz")
    code, st, out, prof = gg_profile_run(db, [tree], data, tmp_path, bool(rc))
    want = util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
    assert code == lib.OK
    assert out.read_bytes() == want
    assert prof.read_bytes() == profile_ref(want, fasta_names(data), st.n_reads)


def test_gg_edge_case_profiles(torch_cuda, tmp_path):
    cases = json.load(open(os.path.join(util.GOLD, "edge_cases.json")))
    db, tree = tree_for("toy")
    for nm, c in sorted(cases.items()):
        data = bytes.fromhex(c["input_hex"])
        code, st, out, prof = gg_profile_run(db, [tree], data, tmp_path, bool(c["rc"]))
        want = bytes.fromhex(c["output_hex"])
        assert out.read_bytes() == want, nm
        if c["exit"] == 0:
            assert code == lib.OK, nm
            assert prof.read_bytes() == profile_ref(want, fasta_names(data), st.n_reads), nm
        else:
            assert code != lib.OK and not prof.exists(), nm           # a failed search writes no profile


@pytest.mark.parametrize("tag", sorted(RANK))
def test_rank_golden_profiles(torch_cuda, tag, tmp_path):
    v = RANK[tag]
    db, tree = tree_for(v["db"])
    out, prof = tmp_path / "o.txt", tmp_path / "p.tsv"
    sl, sp, tol = v["params"]
    code, st = search_rank(db, tree, util.fixture_reads_path(v["reads"]), str(out), rc=bool(v["rc"]), slack=sl, sparsity=sp,
                           tolerance=tol, threads=4, profile=str(prof))
    want = util.fixture_bytes(tag + ".txt.gz")
    assert code == lib.OK and out.read_bytes() == want
    data = util.fixture_bytes(v["reads"] + "_reads.fa.gz")
    assert prof.read_bytes() == profile_ref(want, fasta_names(data), st.n_reads)


@pytest.mark.parametrize("cli,name,rc", [(lib.CLI_PATH, "toy", 1), (lib.CLI_PATH, "vote", 0), (lib.RANK_CLI_PATH, "toy", 0)])
def test_cli_profile(torch_cuda, cli, name, rc, tmp_path):
    ctr = util.fixture_ctr(name)
    fa = util.fixture_reads_path(name)
    args = ["4"] + (["RC"] if rc else [])
    env = dict(os.environ, UTREE_GPUS="1")
    plain = subprocess.run([cli, ctr, fa, str(tmp_path / "a.txt")] + args, capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0
    assert not list(tmp_path.glob("*.tsv"))                      # without the variable: no file
    prof = tmp_path / "p.tsv"
    withp = subprocess.run([cli, ctr, fa, str(tmp_path / "b.txt")] + args, capture_output=True, env=dict(env, UTREE_PROFILE=str(prof)), timeout=300)
    assert withp.returncode == 0
    assert withp.stdout == plain.stdout
    out = (tmp_path / "b.txt").read_bytes()
    assert out == (tmp_path / "a.txt").read_bytes()
    data = util.fixture_bytes(name + "_reads.fa.gz")
    assert prof.read_bytes() == profile_ref(out, fasta_names(data), data.count(b"\n") // 2)
    bad = subprocess.run([cli, ctr, fa, str(tmp_path / "c.txt")] + args, capture_output=True,
                         env=dict(env, UTREE_PROFILE=str(tmp_path / "no" / "dir" / "p.tsv")), timeout=300)
    assert bad.returncode == 1 and b"profile" in bad.stderr and not (tmp_path / "c.txt").exists()
    # a profile that cannot be written after the search: the search's stdout and output, the cause on stderr, exit 1
    full = subprocess.run([cli, ctr, fa, str(tmp_path / "d.txt")] + args, capture_output=True, env=dict(env, UTREE_PROFILE="/dev/full"),
                          timeout=300)
    assert full.returncode == 1 and full.stdout == plain.stdout and b"profile /dev/full" in full.stderr
    assert (tmp_path / "d.txt").read_bytes() == out


def test_cli_leaves_the_profile_path_alone_when_the_search_fails(torch_cuda, tmp_path):
    """the pre-check creates nothing, and a search that fails (here: an input file that does not exist) leaves the path as it was"""
    ctr = util.fixture_ctr("toy")
    env = dict(os.environ, UTREE_GPUS="1")
    prof = tmp_path / "p.tsv"
    r = subprocess.run([lib.CLI_PATH, ctr, str(tmp_path / "missing.fa"), str(tmp_path / "o.txt")], capture_output=True,
                       env=dict(env, UTREE_PROFILE=str(prof)), timeout=300)
    assert r.returncode == 1 and not prof.exists()
    prof.write_bytes(b"an earlier profile\n")
    r = subprocess.run([lib.CLI_PATH, ctr, str(tmp_path / "missing.fa"), str(tmp_path / "o.txt")], capture_output=True,
                       env=dict(env, UTREE_PROFILE=str(prof)), timeout=300)
    assert r.returncode == 1 and prof.read_bytes() == b"an earlier profile\n"


def test_file_search_with_a_table_too_small(torch_cuda, tmp_path, monkeypatch):
    """more truncated taxa than the table holds: the search and its output are complete, the profile is not written (UTREE_E_PROFILE)"""
    db, tree = tree_for("vote")
    data = util.fixture_bytes("vote_reads.fa.gz")
    monkeypatch.setenv("UTREE_PROFILE_CAPACITY", "1")                # 16 slots; the vote fixture prints 21 truncated taxa
    code, st, out, prof = gg_profile_run(db, [tree], data, tmp_path, False)
    assert code == lib.E_PROFILE and not prof.exists()
    assert out.read_bytes() == util.fixture_bytes("vote_out.txt.gz")
    assert b"too small" in lib.load().utree_last_hip_error()
    monkeypatch.delenv("UTREE_PROFILE_CAPACITY")
    code, st, out, prof = gg_profile_run(db, [tree], data, tmp_path, False)
    assert code == lib.OK and prof.exists()


def test_profile_add_refuses_what_it_cannot_count(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    p = tree.profile(64)
    good = torch.zeros((100, 6), dtype=torch.int32, device="cuda:0")
    for bad in (good[::2], good.to(torch.int64), good[:, :5].contiguous(), good.cpu(), good.view(-1)):
        with pytest.raises(ValueError):
            p.add(bad)
    with pytest.raises(ValueError):
        p.add(good, n=101)
    p.add(good, n=40)
    e, nr, nc = p.entries()
    assert nr == 40 and nc == 0 and len(e) == 0
    p.close()


def oracle_taxa(db, want):
    """texts of the oracle's records that print a line (GG)"""
    taxa = []
    for lab, cut, found in zip(want["label"], want["cut"], want["found"]):
        if not found:
            continue
        t = db.label(int(lab))
        taxa.append(b"" if cut == -1 else t if cut < 0 else t[:int(cut)])
    return taxa


def test_batch_api_many_batches_vs_oracle(torch_cuda, tmp_path):
    torch = torch_cuda
    db, tree = tree_for("vote")
    o = orc.OracleDB.load(util.fixture_ctr("vote"))
    data = util.fixture_bytes("vote_reads.fa.gz")
    fr = frame_fasta(data)
    n = len(fr["seq_off"])
    rng = np.random.default_rng(11)
    buf = np.frombuffer(data, dtype=np.uint8)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    prof = tree.profile(1 << 12)
    taxa, total = [], 0
    for rep in range(3):
        order = rng.permutation(n)                               # seeded shuffles of the reads, in batches of seeded sizes
        a = 0
        while a < n:
            b = min(n, a + int(rng.integers(1, 3000)))
            idx = order[a:b]
            off, ln = fr["seq_off"][idx], fr["seq_len"][idx]
            rc = bool(rep & 1)
            res = tree.classify(d_buf, torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda(), rc=rc)
            prof.add(res)
            taxa += oracle_taxa(db, o.classify_batch(buf, off, ln, rc=rc, threads=0))
            total += b - a
            a = b
    torch.cuda.synchronize()
    tree.poll()
    e, nr, nc = prof.entries()
    assert nr == total and nc == len(taxa)
    write_profile(db, e, nr, str(tmp_path / "p.tsv"))
    assert (tmp_path / "p.tsv").read_bytes() == profile_from_taxa(taxa, total)
    prof.reset()
    e, nr, nc = prof.entries()
    assert len(e) == 0 and nr == 0 and nc == 0
    prof.close()


def test_table_too_small_is_reported(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    n_lab = db.info.n_labels
    k = 4000                                                     # distinct truncated keys
    res = np.zeros((k, 6), dtype=np.int32)
    res[:, 0] = np.arange(k) % n_lab
    res[:, 1] = np.arange(k) // n_lab + 1
    res[:, 2] = 1
    d = torch.from_numpy(res).cuda()
    small = tree.profile(16)
    small.add(d)
    with pytest.raises(lib.UtreeError) as ei:
        small.entries()
    assert ei.value.code == lib.E_DEVICE
    small.close()
    big = tree.profile(2 * k)
    big.add(d)
    big.add(d)
    e, nr, nc = big.entries()
    assert nr == 2 * k and nc == 2 * k and len(e) == k and (e["reads"] == 2).all() and (e["cut"] >= 1).all()
    big.close()


def synth_records_tally(torch, res):
    """exact tally of records [n, 6] on the device: ({(label, cut): reads} of classified reads, unclassified)"""
    lab, cut, found = res[:, 0].long(), res[:, 1].long(), res[:, 2]
    cls = (found != 0) & (cut != -4)
    key = torch.where(cut == -1, torch.full_like(lab, -1), lab) * 4096 + torch.where(cut < -1, torch.full_like(cut, -2), cut) + 8
    u, c = torch.unique(key[cls], return_counts=True)
    return {(int(x) // 4096, int(x) % 4096 - 8): int(y) for x, y in zip(u.tolist(), c.tolist())}, int((~cls).sum())


def entries_tally(e):
    out = {}
    for lab, cut, r in e.tolist():
        k = (-1 if cut == -1 else lab, cut if cut >= -1 else -2)
        out[k] = out.get(k, 0) + r
    return out


def test_hot_taxon_unclassified_and_a_16m_batch(torch_cuda):
    torch = torch_cuda
    from utree_amd import synth
    sdb = synth.make_db(torch.device("cuda:0"), 50_000_000, W=8)
    try:
        reads = synth.make_reads(sdb, 16_000_000, 150)
        res = sdb.tree.classify(reads.bases, reads.off, reads.length, rc=False)
        del reads
        torch.cuda.synchronize()
        sdb.tree.poll()
        prof = sdb.tree.profile(1 << 20)
        prof.add(res)
        want, uncl = synth_records_tally(torch, res)
        e, nr, nc = prof.entries()
        assert nr == 16_000_000 and nr - nc == uncl and entries_tally(e) == want
        assert len(want) > 1000
        # one hot taxon: 5 M copies of one classified record
        i = int(torch.nonzero(res[:, 2] > 0)[0])
        hot = res[i:i + 1].expand(5_000_000, 6).contiguous()
        prof.reset()
        prof.add(hot)
        e, nr, nc = prof.entries()
        assert nr == nc == 5_000_000 and len(e) == 1 and int(e["reads"][0]) == 5_000_000
        # all unclassified
        none = torch.zeros((4_000_000, 6), dtype=torch.int32, device="cuda:0")
        prof.reset()
        prof.add(none)
        e, nr, nc = prof.entries()
        assert nr == 4_000_000 and nc == 0 and len(e) == 0
        prof.close()
    finally:
        sdb.tree.close()


def check_file_profile(db, data, out_bytes, prof, n_reads):
    assert prof.read_bytes() == profile_ref(out_bytes, fasta_names(data), n_reads)


@pytest.mark.parametrize("chunk", [300, 20000])
def test_small_chunks(torch_cuda, chunk, tmp_path, monkeypatch):
    monkeypatch.setenv("UTREE_CHUNK_BYTES", str(chunk))
    db, tree = tree_for("toy")
    data = util.fixture_bytes("toy_reads.fa.gz")
    code, st, out, prof = gg_profile_run(db, [tree], data, tmp_path, True)
    want = util.fixture_bytes("toy_out_rc.txt.gz")
    assert code == lib.OK and st.pipeline == 1 and out.read_bytes() == want
    check_file_profile(db, data, want, prof, st.n_reads)


@pytest.mark.parametrize("parts", [2, 8])
def test_output_parts(torch_cuda, parts, tmp_path, monkeypatch):
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "20000")
    monkeypatch.setenv("UTREE_OUTPUT_PARTS", str(parts))
    db, tree = tree_for("toy")
    data = util.fixture_bytes("toy_reads.fa.gz")
    code, st, out, prof = gg_profile_run(db, [tree], data, tmp_path, True)
    want = util.fixture_bytes("toy_out_rc.txt.gz")
    assert code == lib.OK
    assert b"".join((tmp_path / ("out.txt.part%03d" % i)).read_bytes() for i in range(parts)) == want
    check_file_profile(db, data, want, prof, st.n_reads)


@pytest.mark.parametrize("n_handles", [2, 8])
def test_several_device_handles_on_one_card(torch_cuda, n_handles, tmp_path, monkeypatch):
    torch = torch_cuda
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "20000")
    db, tree = tree_for("toy")
    ptr, used = tree.image_ptr()

    class _Raw:
        __cuda_array_interface__ = {"shape": (used,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    src = torch.as_tensor(_Raw(), device="cuda:0")
    copies, trees = [], [tree]
    for _ in range(n_handles - 1):
        c = torch.empty(used + 4096, dtype=torch.uint8, device="cuda:0")[4096:]
        c.copy_(src)
        copies.append(c)
    torch.cuda.synchronize()
    trees += [DeviceTree.attach(db, c, 0) for c in copies]
    data = util.fixture_bytes("toy_reads.fa.gz")
    want = util.fixture_bytes("toy_out_rc.txt.gz")
    try:
        for host in ("", "1"):                                    # the device pipeline, then the host pipeline's sharding
            if host:
                monkeypatch.setenv("UTREE_HOST_TEXT", host)
            code, st, out, prof = gg_profile_run(db, trees, data, tmp_path, True)
            assert code == lib.OK and out.read_bytes() == want
            check_file_profile(db, data, want, prof, st.n_reads)
    finally:
        for t in trees[1:]:
            t.close()


def test_fastq_gzip_input(torch_cuda, tmp_path):
    data = util.fixture_bytes("toy_reads.fa.gz")
    names, off, ln = util.parse_fasta(data)
    blob = b"".join(b"@" + names[i] + b" c\n" + data[off[i]:off[i] + ln[i]] + b"\n+\n" + b"#" * int(ln[i]) + b"\n" for i in range(len(names)))
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(gzip.compress(blob, 1))
    db, tree = tree_for("toy")
    out, prof = tmp_path / "o.txt", tmp_path / "p.tsv"
    code, st = search_gg(db, [tree], str(path), str(out), rc=True, threads=4, input_format=lib.INPUT_FASTQ, profile=str(prof))
    want = util.fixture_bytes("toy_out_rc.txt.gz")
    assert code == lib.OK and out.read_bytes() == want
    check_file_profile(db, data, want, prof, len(names))


@pytest.mark.parametrize("where", [0.02, 0.55, 0.97])
def test_hand_over_counts_each_read_once(torch_cuda, where, tmp_path, monkeypatch):
    """a NUL byte late in the file: into a FIFO the host pipeline continues behind the chunks already written (the profile carries
    their counts); into a regular file it starts over (so does the profile)"""
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "20000")
    db, tree = tree_for("toy")
    o = orc.OracleDB.load(util.fixture_ctr("toy"))
    data = bytearray(util.fixture_bytes("toy_reads.fa.gz")[:600_000])
    data = data[: data.rfind(b"\n>") + 1]
    at = data.index(b"\n", data.index(b"\n>", int(where * len(data))) + 1) + 30
    assert data[at] in b"ACGTacgtN"
    data[at] = 0
    data = bytes(data)
    fa, fifo, want_p = tmp_path / "in.fa", tmp_path / "out.fifo", tmp_path / "want.txt"
    fa.write_bytes(data)
    ocode, nr, good, err = o.search_file(str(fa), str(want_p), threads=4, rc=True)
    assert ocode == 0
    want = want_p.read_bytes()
    os.mkfifo(fifo)
    got = {}

    def reader():
        with open(fifo, "rb") as f:
            got["bytes"] = f.read()
    th = threading.Thread(target=reader)
    th.start()
    prof = tmp_path / "fifo.tsv"
    code, st = search_gg(db, [tree], str(fa), str(fifo), rc=True, threads=4, profile=str(prof))
    th.join(60)
    assert code == lib.OK and st.pipeline == 0 and got["bytes"] == want and st.n_reads == nr
    check_file_profile(db, data, want, prof, nr)
    code, st, out, prof = gg_profile_run(db, [tree], data, tmp_path, True)
    assert code == lib.OK and out.read_bytes() == want and st.n_reads == nr
    check_file_profile(db, data, want, prof, nr)
