"""GPU tests of the per-taxon k-mer coverage (csrc/coverage_kernels.hip, csrc/coverage.c, UTREE_COVERAGE): every coverage file must equal
tests/coverage_ref.py -- the contract restated with the CPU oracle and the .ctr reader, pinned in tests/test_coverage_cpu.py --, byte for
byte, and the per-read output must stay what it was.  All comparisons are exact: there is no tolerance in this feature.

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

import coverage_ref
from oracle import orc
from profile_ref import fasta_names, profile_ref
from test_coverage_cpu import PINNED, fixture_seqs, reference_file
from utree_amd import ctrfile, lib
from utree_amd.search import CtrDB, DeviceTree, frame_fasta, search_gg
import util


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


def gg_run(db, trees, data, tmp_path, rc, profile=False, **kw):
    fa, out, cov, prof = tmp_path / "in.fa", tmp_path / "out.txt", tmp_path / "coverage.tsv", tmp_path / "profile.tsv"
    fa.write_bytes(data)
    for p in (out, cov, prof):
        if p.exists():
            p.unlink()
    code, st = search_gg(db, trees, str(fa), str(out), rc=rc, threads=4, coverage=str(cov), profile=str(prof) if profile else None, **kw)
    return code, st, out, cov, prof


def fixture_data(name):
    return util.fixture_bytes(util.READS_OF.get(name, name) + "_reads.fa.gz")


def ref_file_of(ctr_path, seqs, rc):
    db, cov, hits, texts = coverage_ref.coverage_counts(ctr_path, seqs, rc)
    return coverage_ref.coverage_file(db, cov, hits, texts, len(seqs)), db, cov, hits


def framed_seqs(data):
    fr = frame_fasta(data)
    return [data[int(o):int(o) + int(l)] for o, l in zip(fr["seq_off"], fr["seq_len"])]


@pytest.mark.parametrize("name,rc", sorted(PINNED))
def test_gg_golden_coverage(torch_cuda, name, rc, tmp_path):
    db, tree = tree_for(name)
    data = fixture_data(name)
    want_out = util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
    want = reference_file(name, rc)[0]
    code, st, out, cov, prof = gg_run(db, [tree], data, tmp_path, bool(rc))
    assert code == lib.OK and st.n_reads == PINNED[(name, rc)][0]
    assert out.read_bytes() == want_out
    assert cov.read_bytes() == want
    reads, n_nodes, hits, covered = PINNED[(name, rc)][:4]
    assert want.startswith(b"# reads\t%d\thits\t%d\tcovered\t%d\tdb_kmers\t%d\n" % (reads, hits, covered, n_nodes))
    assert not prof.exists()
    # and with the profile as well: both files, the same output
    code, st, out, cov, prof = gg_run(db, [tree], data, tmp_path, bool(rc), profile=True)
    assert code == lib.OK and out.read_bytes() == want_out and cov.read_bytes() == want
    assert prof.read_bytes() == profile_ref(want_out, fasta_names(data), st.n_reads)


def test_gg_edge_case_coverage(torch_cuda, tmp_path):
    cases = json.load(open(os.path.join(util.GOLD, "edge_cases.json")))
    db, tree = tree_for("toy")
    ctr = util.fixture_ctr("toy")
    for nm, c in sorted(cases.items()):
        data = bytes.fromhex(c["input_hex"])
        code, st, out, cov, prof = gg_run(db, [tree], data, tmp_path, bool(c["rc"]))
        assert out.read_bytes() == bytes.fromhex(c["output_hex"]), nm
        if c["exit"] == 0:
            assert code == lib.OK, nm
            seqs = framed_seqs(data)
            assert len(seqs) == st.n_reads, nm
            assert cov.read_bytes() == ref_file_of(ctr, seqs, bool(c["rc"]))[0], nm
        else:
            assert code != lib.OK and not cov.exists(), nm            # a failed search writes no coverage file


def test_stored_index_beyond_the_labels(torch_cuda, tmp_path):
    """records whose stored index is >= n_labels are never hits (itree.c:929) and belong to no label's db_kmers"""
    rng = np.random.default_rng(7)
    labels = ["k__A;p__B", "k__A;p__C", "k__D"]
    lo = np.unique(rng.integers(0, 1 << 63, 600, dtype=np.uint64))
    ix = rng.integers(0, 5, len(lo)).astype(np.uint32)                 # 3 and 4 name no label
    path = str(tmp_path / "inv.ctr")
    ctrfile.write_ctr(path, 8, 2, np.zeros_like(lo), lo, ix, labels)
    seqs = [("N".join(ctrfile.decode_kmer(0, int(w), 32) for w in rng.choice(lo, 5))).encode() for _ in range(400)]
    data = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))
    want, dbk, covd, hits = ref_file_of(path, seqs, True)
    assert int(dbk.sum()) == int((ix < 3).sum()) < len(lo) and int(hits.sum()) > 500
    db = CtrDB.open(path)
    tree = DeviceTree.upload(db, 0)
    try:
        code, st, out, cov, prof = gg_run(db, [tree], data, tmp_path, True)
        assert code == lib.OK and cov.read_bytes() == want
    finally:
        tree.close()


def device_batch(torch, off, ln):
    return (torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())


def test_batch_api_shuffled_batches_streams_and_reset(torch_cuda, tmp_path):
    torch = torch_cuda
    for name in ("vote", "k64ix32", "k16"):
        db, tree = tree_for(name)
        data = fixture_data(name)
        _, off, ln = util.parse_fasta(data)
        n = len(off)
        rng = np.random.default_rng(11)
        d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        cov = tree.coverage()
        streams = [torch.cuda.Stream() for _ in range(4)]
        torch.cuda.synchronize()
        keep, total, use = [], 0, 0
        for rep in range(2):                                     # forward, then RC: seeded shuffles in batches of seeded sizes
            order = rng.permutation(n)
            a = 0
            while a < n:
                b = min(n, a + int(rng.integers(1, 1500)))
                idx = order[a:b]
                d_off, d_len = device_batch(torch, off[idx], ln[idx])
                keep.append((d_off, d_len))
                with torch.cuda.stream(streams[use % 4]):
                    cov.add(d_buf, d_off, d_len, rc=bool(rep))
                use += 1
                total += b - a
                a = b
        torch.cuda.synchronize()
        e, nr, nh = cov.entries()
        f0, f1 = reference_file(name, 0), reference_file(name, 1)
        assert nr == total == 2 * n and len(e) == db.info.n_labels and (e["label"] == np.arange(len(e))).all()
        assert (e["db_kmers"] == f0[1]).all() and (e["hits"] == f0[3] + f1[3]).all() and nh == int(f0[3].sum() + f1[3].sum())
        # distinct nodes over both passes: the RC pass covers everything the forward pass does
        assert (e["covered"] == f1[2]).all() and (e["covered"] <= e["db_kmers"]).all() and (e["covered"] <= e["hits"]).all()
        cov.reset()
        e, nr, nh = cov.entries()
        assert nr == 0 and nh == 0 and not e["covered"].any() and not e["hits"].any() and (e["db_kmers"] == f0[1]).all()
        # after the reset: one pass, written through the handle
        d_off, d_len = device_batch(torch, off, ln)
        cov.add(d_buf, d_off, d_len, rc=True)
        cov.write(str(tmp_path / "c.tsv"))
        assert (tmp_path / "c.tsv").read_bytes() == f1[0]
        cov.close()


def test_merge_of_two_handles(torch_cuda, tmp_path):
    torch = torch_cuda
    db, tree = tree_for("toy")
    data = fixture_data("toy")
    _, off, ln = util.parse_fasta(data)
    d_buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    a, b = tree.coverage(), tree.coverage()
    h = len(off) // 3
    o1, l1 = device_batch(torch, off[:h], ln[:h])
    o2, l2 = device_batch(torch, off[h:], ln[h:])
    a.add(d_buf, o1, l1, rc=True)
    b.add(d_buf, o2, l2, rc=True)
    a.merge(b)
    a.write(str(tmp_path / "c.tsv"))
    assert (tmp_path / "c.tsv").read_bytes() == reference_file("toy", 1)[0]
    with pytest.raises(lib.UtreeError):
        a.merge(a)
    a.close(); b.close()


def test_coverage_add_refuses_wrong_tensors(torch_cuda):
    torch = torch_cuda
    db, tree = tree_for("toy")
    cov = tree.coverage()
    bases = torch.zeros(1000, dtype=torch.uint8, device="cuda:0")
    off = torch.zeros(10, dtype=torch.int64, device="cuda:0")
    ln = torch.full((10,), 100, dtype=torch.int32, device="cuda:0")
    for bad in ((bases.cpu(), off, ln), (bases, off.int(), ln), (bases, off, ln.long()), (bases, off[:5], ln), (bases[::2], off, ln)):
        with pytest.raises(ValueError):
            cov.add(*bad)
    cov.add(bases, off, ln)                                      # ten reads of NUL bytes: reads, no window
    e, nr, nh = cov.entries()
    assert nr == 10 and nh == 0
    cov.close()


def long_and_odd_reads(name, seed, k):
    """reads of 10-200 kb made of fixture reads with stray Ns and lower case, reads shorter than k, empty reads"""
    rng = np.random.default_rng(seed)
    seqs = fixture_seqs(name)
    out = []
    for target in (10_000, 47_000, 131_072 + k - 1, 200_000, 4096 + k - 1, 4096 + k, 4097 + k):
        parts, n = [], 0
        while n < target:
            s = seqs[int(rng.integers(0, len(seqs)))]
            r = rng.random()
            if r < 0.2:
                s = s.lower()
            elif r < 0.3:
                s = s + b"N"
            elif r < 0.35:
                s = s[:len(s) // 2] + b"n" + s[len(s) // 2:]
            parts.append(s); n += len(s)
        out.append(b"".join(parts)[:target])
    short = seqs[0][:k - 1]
    odd = [b"", short, short.lower(), b"N" * (k + 5), seqs[1][:k], b"", seqs[2]]
    mixed = []
    for i, s in enumerate(out):
        mixed += [s] + odd[i % len(odd):] + [seqs[int(j)] for j in rng.integers(0, len(seqs), 40)]
    return mixed


@pytest.mark.parametrize("name,rc", [("toy", 1), ("k64", 0), ("k16", 1), ("ix32", 0)])
def test_long_and_odd_reads(torch_cuda, name, rc, tmp_path):
    torch = torch_cuda
    db, tree = tree_for(name)
    seqs = long_and_odd_reads(name, 5, db.info.k)
    assert max(len(s) for s in seqs) == 200_000 and min(len(s) for s in seqs) == 0
    want, dbk, covd, hits = ref_file_of(util.fixture_ctr(name), seqs, bool(rc))
    assert int(hits.sum()) > 1000
    blob = b"".join(seqs)
    ln = np.array([len(s) for s in seqs], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    d_buf = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_off, d_len = device_batch(torch, off, ln)
    cov = tree.coverage()
    cov.add(d_buf, d_off, d_len, rc=bool(rc))
    cov.write(str(tmp_path / "c.tsv"))
    assert (tmp_path / "c.tsv").read_bytes() == want
    # the same through the file search (empty sequence lines are an error of the reference's framing: leave those out there)
    reads = [s for s in seqs if s]
    data = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads))
    code, st, out, covf, prof = gg_run(db, [tree], data, tmp_path, bool(rc))
    assert code == lib.OK and st.n_reads == len(reads)
    want2 = want.replace(b"# reads\t%d\t" % len(seqs), b"# reads\t%d\t" % len(reads), 1)
    assert covf.read_bytes() == want2
    cov.close()


def test_created_from_device_pointers_at_scale_and_a_hot_word(torch_cuda):
    """50 M nodes, 2 M reads forward and RC against figures computed with torch from the kept records; then one read 5 M times"""
    torch = torch_cuda
    from utree_amd import synth
    sdb = synth.make_db(torch.device("cuda:0"), 50_000_000, W=8, keep_raw=True)
    MIN = -(1 << 63)
    try:
        N, nl = sdb.n_nodes, sdb.ctr.info.n_labels
        rec = sdb.records.view(N, 7)
        suf = torch.zeros((N, 8), dtype=torch.uint8, device="cuda:0")
        suf[:, :5] = rec[:, :5]
        ix = (rec[:, 5].long() | (rec[:, 6].long() << 8))
        bx = sdb.binix.long() & 0xFFFFFFFF
        pre = torch.repeat_interleave(torch.arange(1 << 24, device="cuda:0"), bx[1:] - bx[:-1])
        words = (suf.view(torch.int64).view(N) | (pre << 40)) ^ MIN          # signed order = the unsigned order of the words
        del suf, pre
        assert bool((words[1:] > words[:-1]).all()) and int(ix.max()) < nl
        cov = sdb.tree.coverage(sdb.binix.view(torch.uint8), sdb.records)
        n, L, K = 2_000_000, 150, 32
        reads = synth.make_reads(sdb, n, L)
        code = reads.bases.view(n, L).long()
        bad = ~((code == 65) | (code == 67) | (code == 71) | (code == 84))
        code = torch.where(code == 65, 0, torch.where(code == 67, 1, torch.where(code == 71, 2, 3)))
        nwin = L - K + 1
        fw = torch.zeros((n, nwin), dtype=torch.int64, device="cuda:0")
        rw = torch.zeros((n, nwin), dtype=torch.int64, device="cuda:0")
        nbad = torch.zeros((n, nwin), dtype=torch.int64, device="cuda:0")
        for j in range(K):
            fw |= code[:, j:j + nwin] << (62 - 2 * j)
            rw |= (3 - code[:, j:j + nwin]) << (2 * j)
            nbad += bad[:, j:j + nwin]
        ok = nbad == 0
        del nbad, code, bad

        def figures(q):
            q = q ^ MIN
            p = torch.searchsorted(words, q).clamp(max=N - 1)
            p = p[words[p] == q]
            return torch.bincount(ix[p], minlength=nl), torch.bincount(ix[torch.unique(p)], minlength=nl), p

        for rc in (False, True):
            cov.reset()
            cov.add(reads.bases, reads.off, reads.length, rc=rc)
            e, nr, nh = cov.entries()
            hits, covered, _ = figures(torch.cat([fw[ok], rw[ok]]) if rc else fw[ok])
            assert nr == n and (e["db_kmers"] == torch.bincount(ix, minlength=nl).cpu().numpy()).all()
            assert (e["hits"] == hits.cpu().numpy()).all() and (e["covered"] == covered.cpu().numpy()).all()
            res = sdb.tree.classify(reads.bases, reads.off, reads.length, rc=rc)
            torch.cuda.synchronize()
            sdb.tree.poll()
            assert nh == int(res[:, 2].long().sum()) == int(hits.sum()) and nh > 4 * n // 2
        # the hot-word case: one read, 5 M times
        q = fw[:1000] ^ MIN
        found = (words[torch.searchsorted(words, q.reshape(-1)).clamp(max=N - 1)] == q.reshape(-1)).view(1000, nwin)
        i = int(torch.nonzero((ok[:1000].sum(1) == nwin) & (found.sum(1) >= 4))[0])          # a read without an N that hits
        h1, c1, p1 = figures(torch.cat([fw[i], rw[i]]))
        assert int(h1.sum()) >= 4
        m = 5_000_000
        cov.reset()
        cov.add(reads.bases[i * L:(i + 1) * L].clone(), torch.zeros(m, dtype=torch.int64, device="cuda:0"),
                torch.full((m,), L, dtype=torch.int32, device="cuda:0"), rc=True)
        e, nr, nh = cov.entries()
        assert nr == m and nh == m * int(h1.sum())
        assert (e["hits"] == m * h1.cpu().numpy()).all() and (e["covered"] == c1.cpu().numpy()).all()
        assert int(e["covered"].sum()) == len(torch.unique(p1))
        cov.close()
    finally:
        sdb.tree.close()


def check_file_coverage(cov, name, rc=1):
    assert cov.read_bytes() == reference_file(name, rc)[0]


@pytest.mark.parametrize("chunk", [300, 20000])
def test_small_chunks(torch_cuda, chunk, tmp_path, monkeypatch):
    monkeypatch.setenv("UTREE_CHUNK_BYTES", str(chunk))
    db, tree = tree_for("toy")
    code, st, out, cov, prof = gg_run(db, [tree], fixture_data("toy"), tmp_path, True)
    assert code == lib.OK and st.pipeline == 1 and out.read_bytes() == util.fixture_bytes("toy_out_rc.txt.gz")
    check_file_coverage(cov, "toy")


@pytest.mark.parametrize("parts", [2, 8])
def test_output_parts(torch_cuda, parts, tmp_path, monkeypatch):
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "20000")
    monkeypatch.setenv("UTREE_OUTPUT_PARTS", str(parts))
    db, tree = tree_for("toy")
    code, st, out, cov, prof = gg_run(db, [tree], fixture_data("toy"), tmp_path, True)
    assert code == lib.OK
    assert b"".join((tmp_path / ("out.txt.part%03d" % i)).read_bytes() for i in range(parts)) == util.fixture_bytes("toy_out_rc.txt.gz")
    check_file_coverage(cov, "toy")


def test_host_pipeline(torch_cuda, tmp_path, monkeypatch):
    monkeypatch.setenv("UTREE_HOST_TEXT", "1")
    db, tree = tree_for("k64")
    code, st, out, cov, prof = gg_run(db, [tree], fixture_data("k64"), tmp_path, True, profile=True)
    want = util.fixture_bytes("k64_out_rc.txt.gz")
    assert code == lib.OK and st.pipeline == 0 and out.read_bytes() == want
    check_file_coverage(cov, "k64")
    assert prof.read_bytes() == profile_ref(want, fasta_names(fixture_data("k64")), st.n_reads)


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
    want = util.fixture_bytes("toy_out_rc.txt.gz")
    try:
        for host in ("", "1"):                                    # the device pipeline, then the host pipeline's sharding
            if host:
                monkeypatch.setenv("UTREE_HOST_TEXT", host)
            code, st, out, cov, prof = gg_run(db, trees, fixture_data("toy"), tmp_path, True)
            assert code == lib.OK and out.read_bytes() == want
            check_file_coverage(cov, "toy")                      # one handle per device handle, merged
    finally:
        for t in trees[1:]:
            t.close()


def test_fastq_gzip_input(torch_cuda, tmp_path):
    data = fixture_data("toy")
    names, off, ln = util.parse_fasta(data)
    blob = b"".join(b"@" + names[i] + b" c\n" + data[off[i]:off[i] + ln[i]] + b"\n+\n" + b"#" * int(ln[i]) + b"\n" for i in range(len(names)))
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(gzip.compress(blob, 1))
    db, tree = tree_for("toy")
    out, cov = tmp_path / "o.txt", tmp_path / "c.tsv"
    code, st = search_gg(db, [tree], str(path), str(out), rc=True, threads=4, input_format=lib.INPUT_FASTQ, coverage=str(cov))
    assert code == lib.OK and out.read_bytes() == util.fixture_bytes("toy_out_rc.txt.gz")
    check_file_coverage(cov, "toy")


@pytest.mark.parametrize("where", [0.02, 0.55, 0.97])
def test_hand_over_adds_each_read_once(torch_cuda, where, tmp_path, monkeypatch):
    """a NUL byte late in the file: into a FIFO the host pipeline continues behind the chunks already written (the coverage carries
    their reads); into a regular file it starts over (so does the coverage)"""
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "20000")
    db, tree = tree_for("toy")
    o = orc.OracleDB.load(util.fixture_ctr("toy"))
    data = bytearray(fixture_data("toy")[:600_000])
    data = data[: data.rfind(b"\n>") + 1]
    at = data.index(b"\n", data.index(b"\n>", int(where * len(data))) + 1) + 30
    assert data[at] in b"ACGTacgtN"
    data[at] = 0
    data = bytes(data)
    fa, fifo, want_p = tmp_path / "in.fa", tmp_path / "out.fifo", tmp_path / "want.txt"
    fa.write_bytes(data)
    ocode, nr, good, err = o.search_file(str(fa), str(want_p), threads=4, rc=True)
    assert ocode == 0
    want_out = want_p.read_bytes()
    seqs = framed_seqs(data)
    want, dbk, covd, hits = ref_file_of(util.fixture_ctr("toy"), seqs, True)
    assert len(seqs) == nr and int(hits.sum()) == sum(int(l.split(b"\t")[2]) for l in want_out.split(b"\n") if l)
    os.mkfifo(fifo)
    got = {}

    def reader():
        with open(fifo, "rb") as f:
            got["bytes"] = f.read()
    th = threading.Thread(target=reader)
    th.start()
    cov = tmp_path / "fifo.tsv"
    code, st = search_gg(db, [tree], str(fa), str(fifo), rc=True, threads=4, coverage=str(cov))
    th.join(60)
    assert code == lib.OK and st.pipeline == 0 and got["bytes"] == want_out and st.n_reads == nr
    assert cov.read_bytes() == want
    code, st, out, cov, prof = gg_run(db, [tree], data, tmp_path, True)
    assert code == lib.OK and out.read_bytes() == want_out and st.n_reads == nr
    assert cov.read_bytes() == want


@pytest.mark.parametrize("name,rc", [("toy", 1), ("vote", 0)])
def test_cli_coverage(torch_cuda, name, rc, tmp_path):
    cli = lib.CLI_PATH
    ctr = util.fixture_ctr(name)
    fa = util.fixture_reads_path(name)
    args = ["4"] + (["RC"] if rc else [])
    env = dict(os.environ, UTREE_GPUS="1")
    env.pop("UTREE_COVERAGE", None)
    plain = subprocess.run([cli, ctr, fa, str(tmp_path / "a.txt")] + args, capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0
    assert not list(tmp_path.glob("*.tsv"))                      # without the variable: no file
    cov, prof = tmp_path / "c.tsv", tmp_path / "p.tsv"
    withc = subprocess.run([cli, ctr, fa, str(tmp_path / "b.txt")] + args, capture_output=True, env=dict(env, UTREE_COVERAGE=str(cov)), timeout=300)
    assert withc.returncode == 0 and withc.stdout == plain.stdout
    out = (tmp_path / "b.txt").read_bytes()
    assert out == (tmp_path / "a.txt").read_bytes() == util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
    assert cov.read_bytes() == reference_file(name, rc)[0] and not prof.exists()
    cov.unlink()
    both = subprocess.run([cli, ctr, fa, str(tmp_path / "e.txt")] + args, capture_output=True,
                          env=dict(env, UTREE_COVERAGE=str(cov), UTREE_PROFILE=str(prof)), timeout=300)
    assert both.returncode == 0 and both.stdout == plain.stdout and (tmp_path / "e.txt").read_bytes() == out
    assert cov.read_bytes() == reference_file(name, rc)[0]
    data = util.fixture_bytes(name + "_reads.fa.gz")
    assert prof.read_bytes() == profile_ref(out, fasta_names(data), data.count(b"\n") // 2)
    bad = subprocess.run([cli, ctr, fa, str(tmp_path / "c.txt")] + args, capture_output=True,
                         env=dict(env, UTREE_COVERAGE=str(tmp_path / "no" / "dir" / "c.tsv")), timeout=300)
    assert bad.returncode == 1 and b"coverage" in bad.stderr and not (tmp_path / "c.txt").exists() and not (tmp_path / "no").exists()
    # a coverage file that cannot be written after the search: the search's stdout and output, the cause on stderr, exit 1
    full = subprocess.run([cli, ctr, fa, str(tmp_path / "d.txt")] + args, capture_output=True, env=dict(env, UTREE_COVERAGE="/dev/full"),
                          timeout=300)
    assert full.returncode == 1 and full.stdout == plain.stdout and b"coverage /dev/full" in full.stderr
    assert (tmp_path / "d.txt").read_bytes() == out
    # a search that fails leaves the path as it was
    cov.write_bytes(b"an earlier file\n")
    r = subprocess.run([cli, ctr, str(tmp_path / "missing.fa"), str(tmp_path / "o.txt")], capture_output=True,
                       env=dict(env, UTREE_COVERAGE=str(cov)), timeout=300)
    assert r.returncode == 1 and cov.read_bytes() == b"an earlier file\n"


def test_rank_specific_cli_ignores_the_variable(torch_cuda, tmp_path):
    ctr, fa = util.fixture_ctr("toy"), util.fixture_reads_path("toy")
    env = dict(os.environ, UTREE_GPUS="1")
    plain = subprocess.run([lib.RANK_CLI_PATH, ctr, fa, str(tmp_path / "a.txt"), "4"], capture_output=True, env=env, timeout=300)
    withc = subprocess.run([lib.RANK_CLI_PATH, ctr, fa, str(tmp_path / "b.txt"), "4"], capture_output=True,
                           env=dict(env, UTREE_COVERAGE=str(tmp_path / "no" / "dir" / "c.tsv")), timeout=300)
    assert plain.returncode == withc.returncode == 0 and plain.stdout == withc.stdout
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes() == util.fixture_bytes("toy_rank.txt.gz")
    assert not (tmp_path / "no").exists()
