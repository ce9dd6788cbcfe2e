"""GPU tests of paired-end reads (csrc/pairs_kernels.hip, search_reader.c's and search.c's second input, UTREE_MATES / UTREE_INTERLEAVED): the device join against a
numpy join, classify on the joined tensors against the CPU oracle on the numpy join, and the whole-file search against what the genuine
reference prints for mate 1 + "N" + mate 2 (tests/golden/pairs_*_out*.txt.gz, pinned in tests/test_pairs_cpu.py).  All comparisons are
exact: there is no tolerance in this feature.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import coverage_ref
import pairs_ref
from oracle import orc
from profile_ref import profile_ref
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, search_gg
import util

LENS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097)
COMBOS = np.array(list(itertools.product(LENS, LENS)), dtype=np.uint32)            # every (len1, len2)
SENTINEL, GUARD = 0xA5, 8192


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_TREES = {}
_PAIRS = {}


def tree_for(name):
    if name not in _TREES:
        db = CtrDB.open(util.fixture_ctr(name))
        _TREES[name] = (db, DeviceTree.upload(db, 0))
    return _TREES[name]


def pairs_of(name):
    if name not in _PAIRS:
        _PAIRS[name] = pairs_ref.Pairs(name)
    return _PAIRS[name]


# ---- the join kernels ------------------------------------------------------------------------------------------------------------
def lay_out(rng, lens):
    """(blob, offsets): mates of the given lengths laid out in SHUFFLED order with 0-3 stray bytes in front of each, the first byte of the
    blob unused -- so the sources sit at every alignment and in no order"""
    n = len(lens)
    order = rng.permutation(n)
    gaps = rng.integers(0, 4, n).astype(np.uint64)
    sizes = lens[order].astype(np.uint64) + gaps
    starts = 1 + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    off = np.empty(n, dtype=np.uint64)
    off[order] = starts + gaps
    blob = rng.integers(0, 256, size=int(1 + sizes.sum() + 3), dtype=np.uint8)
    return blob, off


def device_join(torch, tree, blob1, off1, len1, blob2, off2, len2, capacity=None, shift=0):
    """utree_pairs_join into a sentinel-filled buffer with `shift` bytes in front of the joined bytes and a guard behind them"""
    n = len(off1)
    total = int(len1.astype(np.uint64).sum() + len2.astype(np.uint64).sum()) + n
    cap = total if capacity is None else capacity
    d1 = torch.from_numpy(blob1).cuda()
    d2 = d1 if blob2 is blob1 else torch.from_numpy(blob2).cuda()
    t = [torch.from_numpy(a).cuda() for a in (off1.astype(np.int64), len1.astype(np.int32), off2.astype(np.int64), len2.astype(np.int32))]
    buf = torch.full((shift + total + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    joff = torch.full((n + 8,), -1, dtype=torch.int64, device="cuda")
    jlen = torch.full((n + 8,), -1, dtype=torch.int32, device="cuda")
    meta = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    lib.check(lib.load().utree_pairs_join(tree._h, d1.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), d2.data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                          n, buf.data_ptr() + shift, cap, joff.data_ptr(), jlen.data_ptr(), meta.data_ptr(), stream.cuda_stream),
              "utree_pairs_join")
    stream.synchronize()
    m = lib.PairsMeta.from_buffer_copy(meta.cpu().numpy().tobytes())
    return buf.cpu().numpy(), joff.cpu().numpy(), jlen.cpu().numpy(), m, total


def check_join(torch, tree, rng, len1, len2, same_buffer=False, shift=0):
    len1, len2 = np.asarray(len1, dtype=np.uint32), np.asarray(len2, dtype=np.uint32)
    n = len(len1)
    if same_buffer:
        blob1, off = lay_out(rng, np.concatenate([len1, len2]))
        blob2, off1, off2 = blob1, off[:n], off[n:]
    else:
        (blob1, off1), (blob2, off2) = lay_out(rng, len1), lay_out(rng, len2)
    want, woff, wlen = pairs_ref.numpy_join(blob1, off1, len1, blob2, off2, len2)
    buf, joff, jlen, m, total = device_join(torch, tree, blob1, off1, len1, blob2, off2, len2, shift=shift)
    assert m.error == 0 and m.total_bases == total == len(want) and m.max_len == int(wlen.max())
    assert np.array_equal(joff[:n].astype(np.uint64), woff) and np.array_equal(jlen[:n].view(np.uint32), wlen)
    assert (joff[n:] == -1).all() and (jlen[n:] == -1).all()
    assert np.array_equal(buf[shift:shift + total], want)
    assert (buf[:shift] == SENTINEL).all() and (buf[shift + total:] == SENTINEL).all(), "bytes outside [0, total) were written"
    return buf, total


def test_join_one_pair_every_combination(torch_cuda):
    db, tree = tree_for("toy")
    rng = np.random.default_rng(1)
    for a, b in COMBOS:
        check_join(torch_cuda, tree, rng, [a], [b])


def test_join_two_pairs(torch_cuda):
    db, tree = tree_for("toy")
    rng = np.random.default_rng(2)
    for i in rng.permutation(len(COMBOS) * len(COMBOS))[:60]:
        c, d = COMBOS[i // len(COMBOS)], COMBOS[i % len(COMBOS)]
        check_join(torch_cuda, tree, rng, [c[0], d[0]], [c[1], d[1]], shift=int(i) % 2)


@pytest.mark.parametrize("same_buffer,shift", [(False, 0), (True, 0), (False, 1), (True, 7)])
def test_join_257_pairs(torch_cuda, same_buffer, shift):
    """every combination of lengths, shuffled; both mates in one buffer; a joined buffer that is not 16-byte aligned"""
    db, tree = tree_for("toy")
    rng = np.random.default_rng(3)
    c = COMBOS[np.concatenate([rng.permutation(len(COMBOS)), rng.integers(0, len(COMBOS), 257 - len(COMBOS))])]
    check_join(torch_cuda, tree, rng, c[:, 0], c[:, 1], same_buffer=same_buffer, shift=shift)


def test_join_70000_pairs_and_a_capacity_one_byte_short(torch_cuda):
    """crosses the scan's blocks (1024 pairs) and thousands of gather tiles; tiles of tiny pairs next to 4 KiB mates"""
    torch = torch_cuda
    db, tree = tree_for("toy")
    rng = np.random.default_rng(4)
    c = COMBOS[rng.permutation(np.arange(70_000) % len(COMBOS))]
    len1, len2 = c[:, 0].copy(), c[:, 1].copy()
    (blob1, off1), (blob2, off2) = lay_out(rng, len1), lay_out(rng, len2)
    want, woff, wlen = pairs_ref.numpy_join(blob1, off1, len1, blob2, off2, len2)
    buf, joff, jlen, m, total = device_join(torch, tree, blob1, off1, len1, blob2, off2, len2)
    assert m.error == 0 and m.total_bases == total == len(want) and m.max_len == 4097 + 1 + 4097
    assert np.array_equal(joff[:70_000].astype(np.uint64), woff) and np.array_equal(jlen[:70_000].view(np.uint32), wlen)
    assert np.array_equal(buf[:total], want) and (buf[total:] == SENTINEL).all()
    # one byte short: reported, nothing written -- neither past the capacity nor in front of it
    buf, joff, jlen, m, total = device_join(torch, tree, blob1, off1, len1, blob2, off2, len2, capacity=total - 1)
    assert m.error == 1 and m.total_bases == total
    assert (buf == SENTINEL).all()
    # DeviceTree.join_pairs: the same through the Python surface
    t = [torch.from_numpy(a).cuda() for a in (blob1, off1.astype(np.int64), len1.astype(np.int32), blob2, off2.astype(np.int64), len2.astype(np.int32))]
    joined, d_joff, d_jlen, meta = tree.join_pairs(*t)
    assert meta == dict(total_bases=total, max_len=4097 + 1 + 4097, error=0) and joined.numel() == total
    assert np.array_equal(joined.cpu().numpy(), want) and np.array_equal(d_joff.cpu().numpy().astype(np.uint64), woff)
    joined, d_joff, d_jlen, meta = tree.join_pairs(*t, capacity=100)
    assert meta["error"] == 1


def test_join_100000_pairs_of_empty_mates(torch_cuda):
    """all 'N': every tile holds 4096 pairs, more than the gather pass keeps in LDS"""
    db, tree = tree_for("toy")
    z = np.zeros(100_000, dtype=np.uint32)
    buf, total = check_join(torch_cuda, tree, np.random.default_rng(5), z, z)
    assert total == 100_000 and (buf[:total] == 0x4E).all()


def test_join_a_3_MiB_mate_between_one_byte_mates(torch_cuda):
    db, tree = tree_for("toy")
    rng = np.random.default_rng(6)
    len1 = np.ones(6001, dtype=np.uint32)
    len2 = np.ones(6001, dtype=np.uint32)
    len1[3000] = 3 << 20
    check_join(torch_cuda, tree, rng, len1, len2)
    len1[3000], len2[3000] = 1, 3 << 20
    check_join(torch_cuda, tree, rng, len1, len2, same_buffer=True)


def test_join_refuses_null_pointers(torch_cuda):
    db, tree = tree_for("toy")
    assert lib.load().utree_pairs_join(tree._h, None, None, None, None, None, None, 3, None, 0, None, None, None, None) == lib.E_ARG


# ---- classify on the joined tensors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pairs_ref.FIXTURES)
def test_classify_on_the_joined_tensors_equals_the_oracle_on_the_numpy_join(torch_cuda, name):
    torch = torch_cuda
    db, tree = tree_for(name)
    P = pairs_of(name)
    rng = np.random.default_rng(7)
    len1 = np.array([len(s) for s in P.seq1], dtype=np.uint32)
    len2 = np.array([len(s) for s in P.seq2], dtype=np.uint32)
    order = rng.permutation(2 * P.n)                                               # both mates in one buffer, in no order
    seqs = P.seq1 + P.seq2
    lens = np.concatenate([len1, len2])
    starts = np.zeros(2 * P.n, dtype=np.uint64)
    starts[order] = 3 + np.concatenate([[0], np.cumsum(lens[order].astype(np.uint64) + 1)[:-1]])
    blob = np.full(int(3 + lens.sum() + 2 * P.n), ord("A"), dtype=np.uint8)         # stray bases between the mates: reading one would show
    for i, s in enumerate(seqs):
        blob[int(starts[i]):int(starts[i]) + len(s)] = np.frombuffer(s, dtype=np.uint8)
    off1, off2 = starts[:P.n], starts[P.n:]
    want_bytes, woff, wlen = pairs_ref.numpy_join(blob, off1, len1, blob, off2, len2)
    assert want_bytes.tobytes() == b"".join(P.joined_seqs())
    d_blob = torch.from_numpy(blob).cuda()
    t = [torch.from_numpy(a).cuda() for a in (off1.astype(np.int64), len1.astype(np.int32), off2.astype(np.int64), len2.astype(np.int32))]
    joined, joff, jlen, meta = tree.join_pairs(d_blob, t[0], t[1], d_blob, t[2], t[3])
    assert meta == dict(total_bases=len(want_bytes), max_len=int(wlen.max()), error=0)
    o = orc.OracleDB.load(util.fixture_ctr(name))
    for rc in (False, True):
        want = o.classify_batch(want_bytes, woff, wlen, rc=rc, threads=8)
        got = tree.classify(joined, joff, jlen, rc=rc, total_bases=meta["total_bases"], max_len=meta["max_len"])
        torch.cuda.synchronize()
        tree.poll()
        got = got.cpu().numpy()
        g = got.view(np.uint32)
        hit = want["found"] > 0
        multi = hit & (want["uix"] > 1)
        assert np.array_equal(g[:, 2], want["found"]) and int(hit.sum()) > P.n // 2
        assert np.array_equal(g[hit, 0], want["label"][hit]) and np.array_equal(g[hit, 3], want["uix"][hit])
        assert np.array_equal(got[hit, 1], want["cut"][hit])
        assert np.array_equal(g[multi, 4], want["sl"][multi]) and np.array_equal(g[multi, 5], want["ol"][multi])


# ---- the whole-file search -------------------------------------------------------------------------------------------------------
def run_pairs(db, tree, tmp_path, reads, mates, rc, tag="p", **kw):
    """reads / mates: bytes (mates None: interleaved).  Returns (code, stats, output bytes)."""
    rp, mp, out = tmp_path / (tag + "_1.in"), tmp_path / (tag + "_2.in"), tmp_path / (tag + "_out.txt")
    rp.write_bytes(reads)
    if mates is not None:
        mp.write_bytes(mates)
    code, st = search_gg(db, [tree], str(rp), str(out), rc=bool(rc), threads=4, mates=str(mp) if mates is not None else None,
                         interleaved=mates is None, **kw)
    return code, st, out.read_bytes()


@pytest.mark.parametrize("name,rc", [(n, r) for n in pairs_ref.FIXTURES for r in (0, 1)])
def test_search_gg_pairs_equals_the_reference_on_the_joined_reads(torch_cuda, name, rc, tmp_path):
    db, tree = tree_for(name)
    P = pairs_of(name)
    want = pairs_ref.golden(name, rc)
    prof = tmp_path / "profile.tsv"
    code, st, out = run_pairs(db, tree, tmp_path, P.reads_fasta(), P.mates_fasta(), rc, profile=str(prof))
    assert code == lib.OK and st.n_reads == P.n and st.pipeline == 0 and st.good_finds == want.count(b"\n")
    assert out == want
    assert prof.read_bytes() == profile_ref(want, P.names1, P.n)                 # "# reads" counts pairs
    code, st, out = run_pairs(db, tree, tmp_path, P.interleaved_fasta(), None, rc, tag="i")
    assert code == lib.OK and st.n_reads == P.n and out == want


def test_search_gg_pairs_fastq_with_gzip_mates(torch_cuda, tmp_path):
    db, tree = tree_for("toy")
    P = pairs_of("toy")
    code, st, out = run_pairs(db, tree, tmp_path, P.reads_fastq(), pairs_ref.gz(P.mates_fastq()), 1, input_format=lib.INPUT_FASTQ)
    assert code == lib.OK and st.n_reads == P.n and out == pairs_ref.golden("toy", 1)
    code, st, out = run_pairs(db, tree, tmp_path, pairs_ref.gz(P.reads_fastq()), P.mates_fastq(), 0, input_format=lib.INPUT_AUTO, tag="a")
    assert code == lib.OK and st.n_reads == P.n and out == pairs_ref.golden("toy", 0)


@pytest.mark.parametrize("name,rc,interleaved", [("toy", 1, False), ("k64", 0, False), ("vote", 1, True)])
def test_search_gg_pairs_small_chunks(torch_cuda, name, rc, interleaved, tmp_path, monkeypatch):
    """hundreds of slots and a carry in each file; the mates' headers are longer than the reads', so the two files' chunks fall out of step"""
    monkeypatch.setenv("UTREE_CHUNK_BYTES", "4096")
    db, tree = tree_for(name)
    P = pairs_of(name)
    assert len(P.mates_fasta()) > len(P.reads_fasta()) + 40 * P.n and len(P.reads_fasta()) > 20 * 4096
    reads, mates = (P.interleaved_fasta(), None) if interleaved else (P.reads_fasta(), P.mates_fasta())
    code, st, out = run_pairs(db, tree, tmp_path, reads, mates, rc)
    assert code == lib.OK and st.n_reads == P.n and out == pairs_ref.golden(name, rc)


@pytest.mark.parametrize("interleaved,chunk", [(False, 4096), (True, 4096), (False, 700)])
def test_search_gg_pairs_multiline_fasta_small_chunks(torch_cuda, interleaved, chunk, tmp_path, monkeypatch):
    """multi-line FASTA is compacted in place when it is framed: the framed records a slot does not commit -- the reads file runs ahead of the
    mates file, whose headers are longer -- are written out again for the next slot; the two files wrap their lines differently, one is gzip"""
    monkeypatch.setenv("UTREE_CHUNK_BYTES", str(chunk))
    db, tree = tree_for("toy")
    P = pairs_of("toy")
    if interleaved:
        reads, mates = pairs_ref.wrap(P.interleaved_fasta(), 11), None
    else:
        reads, mates = pairs_ref.wrap(P.reads_fasta(), 7), pairs_ref.gz(pairs_ref.wrap(P.mates_fasta(), 13))
    assert reads.count(b"\n") > 3 * P.n
    code, st, out = run_pairs(db, tree, tmp_path, reads, mates, 1, input_format=lib.INPUT_FASTA_MULTILINE)
    assert code == lib.OK and st.n_reads == P.n and out == pairs_ref.golden("toy", 1)


@pytest.mark.parametrize("chunk", [0, 4096])
@pytest.mark.parametrize("bad_in", ["mates", "reads", "interleaved"])
def test_a_malformed_record_keeps_its_code_and_its_files_record_number(torch_cuda, bad_in, chunk, tmp_path, monkeypatch):
    """the pairs in front of a malformed record are written; read_index counts the records of the file the record is in"""
    if chunk:
        monkeypatch.setenv("UTREE_CHUNK_BYTES", str(chunk))
    db, tree = tree_for("toy")
    P = pairs_of("toy")
    at = 1234                                                                      # complete pairs in front of the bad record

    def spoil(fasta, n_good):
        cut = len(b"".join(fasta.split(b">")[1:n_good + 1])) + n_good               # bytes of the first n_good records
        assert fasta[cut:cut + 1] == b">"
        return fasta[:cut] + b"no header here\nACGT\n" + fasta[cut:]
    if bad_in == "interleaved":
        reads, mates, index = spoil(P.interleaved_fasta(), 2 * at + 1), None, 2 * at + 2       # the bad record is pair `at`'s mate
    elif bad_in == "mates":
        reads, mates, index = P.reads_fasta(), spoil(P.mates_fasta(), at), at + 1
    else:
        reads, mates, index = spoil(P.reads_fasta(), at), P.mates_fasta(), at + 1
    code, st, out = run_pairs(db, tree, tmp_path, reads, mates, 0)
    got = pairs_ref.lines_by_name(pairs_ref.golden("toy", 0), P.names1)
    assert code == lib.E_FASTA and st.fasta_error.code == 2 and st.fasta_error.read_index == index and st.n_reads == at
    assert out == b"".join(got[i] + b"\n" for i in range(at) if i in got)


@pytest.mark.parametrize("rc", [0, 1])
def test_reports_see_the_joined_queries(torch_cuda, rc, tmp_path):
    """profile and coverage of a paired search are those of the joined input: each mate's windows, none across the 'N'"""
    db, tree = tree_for("toy")
    P = pairs_of("toy")
    n = 600
    prof, cov = tmp_path / "p.tsv", tmp_path / "c.tsv"
    code, st, out = run_pairs(db, tree, tmp_path, P.reads_fasta(n), P.mates_fasta(n), rc, profile=str(prof), coverage=str(cov))
    got = pairs_ref.lines_by_name(pairs_ref.golden("toy", rc), P.names1)
    want_out = b"".join(got[i] + b"\n" for i in range(n) if i in got)
    assert code == lib.OK and st.n_reads == n and out == want_out
    assert prof.read_bytes() == profile_ref(want_out, P.names1[:n], n)
    ctr = util.fixture_ctr("toy")
    dbk, covd, hits, texts = coverage_ref.coverage_counts(ctr, P.joined_seqs()[:n], bool(rc))
    assert cov.read_bytes() == coverage_ref.coverage_file(dbk, covd, hits, texts, n)
    # every hit window is one of some line's `found`, and most pairs have a line
    assert int(hits.sum()) == sum(int(l.split(b"\t")[2]) for l in want_out.split(b"\n") if l) >= want_out.count(b"\n") > n // 2


@pytest.mark.parametrize("case", ["mates_one_short", "mates_one_long", "interleaved_odd"])
def test_unequal_record_counts(torch_cuda, case, tmp_path):
    db, tree = tree_for("toy")
    P = pairs_of("toy")
    n = P.n - 1                                                                    # the complete pairs
    reads, mates = {"mates_one_short": (P.reads_fasta(), P.mates_fasta(n)), "mates_one_long": (P.reads_fasta(n), P.mates_fasta()),
                    "interleaved_odd": (P.interleaved_fasta(2 * P.n - 1), None)}[case]
    code, st, out = run_pairs(db, tree, tmp_path, reads, mates, 0)
    why = lib.load().utree_last_hip_error().decode()
    got = pairs_ref.lines_by_name(pairs_ref.golden("toy", 0), P.names1)
    assert code == lib.E_PAIRS == 14 and st.n_reads == n
    assert out == b"".join(got[i] + b"\n" for i in range(n) if i in got)
    # utree_last_hip_error names the shorter file
    assert {"mates_one_short": "p_2.in ends after %d records" % n, "mates_one_long": "p_1.in ends after %d records" % n,
            "interleaved_odd": "p_1.in holds an odd number of records (%d)" % (2 * P.n - 1)}[case] in why


def test_a_pair_longer_than_a_line_is_a_framing_error(torch_cuda, tmp_path):
    db, tree = tree_for("toy")
    P = pairs_of("toy")
    half = b"ACGT" * (2 << 20)                                                    # 8 Mi + 1 + 8 Mi > LINELEN (16 Mi)
    reads = P.reads_fasta(3) + b">long\n" + half + b"\n" + P.reads_fasta(5)[len(P.reads_fasta(4)):]
    mates = P.mates_fasta(3) + b">long/2\n" + half + b"\n" + P.mates_fasta(5)[len(P.mates_fasta(4)):]
    code, st, out = run_pairs(db, tree, tmp_path, reads, mates, 0)
    got = pairs_ref.lines_by_name(pairs_ref.golden("toy", 0), P.names1)
    assert code == lib.E_FASTA and st.fasta_error.code == 5 and st.fasta_error.read_index == 4 and st.n_reads == 3
    assert out == b"".join(got[i] + b"\n" for i in range(3) if i in got)


def test_missing_mates_file(torch_cuda, tmp_path):
    db, tree = tree_for("toy")
    rp = tmp_path / "r.fa"
    rp.write_bytes(pairs_of("toy").reads_fasta(10))
    code, st = search_gg(db, [tree], str(rp), str(tmp_path / "o.txt"), mates=str(tmp_path / "nope.fa"))
    assert code == lib.E_IO


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_cli_pairs(torch_cuda, tmp_path):
    P = pairs_of("toy")
    ctr = util.fixture_ctr("toy")
    rp, mp, jp = tmp_path / "r1.fa", tmp_path / "r2.fa", tmp_path / "joined.fa"
    rp.write_bytes(P.reads_fasta()); mp.write_bytes(P.mates_fasta()); jp.write_bytes(P.joined_fasta())
    env = dict(os.environ, UTREE_GPUS="1")
    for v in ("UTREE_MATES", "UTREE_INTERLEAVED", "UTREE_INPUT", "UTREE_PROFILE", "UTREE_COVERAGE", "UTREE_CHUNK_BYTES"):
        env.pop(v, None)
    cli = lib.CLI_PATH

    def run(exe, reads, out, **extra):
        return subprocess.run([exe, ctr, str(reads), str(tmp_path / out), "4", "RC"], capture_output=True, env=dict(env, **extra), timeout=300)
    want = pairs_ref.golden("toy", 1)
    single = run(cli, jp, "single.txt")                                            # the joined reads as one file: the usual stdout
    assert single.returncode == 0 and (tmp_path / "single.txt").read_bytes() == want
    paired = run(cli, rp, "paired.txt", UTREE_MATES=str(mp))
    assert paired.returncode == 0 and (tmp_path / "paired.txt").read_bytes() == want
    assert paired.stdout == single.stdout and b"Searched %d queries\n" % P.n in paired.stdout
    ip = tmp_path / "il.fa"
    ip.write_bytes(P.interleaved_fasta())
    inter = run(cli, ip, "inter.txt", UTREE_INTERLEAVED="1")
    assert inter.returncode == 0 and (tmp_path / "inter.txt").read_bytes() == want and inter.stdout == single.stdout
    # a mates file that does not open: before the tree is loaded
    missing = run(cli, rp, "missing.txt", UTREE_MATES=str(tmp_path / "nope.fa"))
    assert missing.returncode == 1 and b"Invalid input files" in missing.stdout and b"Tree read." not in missing.stdout
    assert not (tmp_path / "missing.txt").exists()
    both = run(cli, rp, "both.txt", UTREE_MATES=str(mp), UTREE_INTERLEAVED="1")
    assert both.returncode == 1 and b"UTREE_INTERLEAVED" in both.stderr and not (tmp_path / "both.txt").exists()
    # the rank-specific search reads no pairs
    for extra in (dict(UTREE_MATES=str(mp)), dict(UTREE_INTERLEAVED="1")):
        rank = run(lib.RANK_CLI_PATH, rp, "rank.txt", **extra)
        assert rank.returncode == 1 and rank.stderr.count(b"\n") == 1 and b"pairs" in rank.stderr and b"Tree read." not in rank.stdout
    # unequal record counts: the complete pairs, a message, exit 2
    sp = tmp_path / "short.fa"
    sp.write_bytes(P.mates_fasta(P.n - 7))
    short = run(cli, rp, "short.txt", UTREE_MATES=str(sp))
    got = pairs_ref.lines_by_name(want, P.names1)
    assert short.returncode == 2 and b"short.fa" in short.stderr
    assert (tmp_path / "short.txt").read_bytes() == b"".join(got[i] + b"\n" for i in range(P.n - 7) if i in got)
    # without the variables: today's output, byte for byte
    plain = run(cli, util.fixture_reads_path("toy"), "plain.txt")
    assert plain.returncode == 0 and (tmp_path / "plain.txt").read_bytes() == util.fixture_bytes("toy_out_rc.txt.gz")
    assert b"Searched 10000 queries\n" in plain.stdout
