"""Reads up to the 16 MiB line limit (tests/long_inputs.py) on every path that takes them, against the CPU oracle, which
tests/test_long_cpu.py holds to the genuine reference on these very inputs.

What exists only between the suite's 200 kb reads and the limit, and is reached here: a read in hundreds (MID) and thousands (LMAX) of pieces
(pieces_k, the PIECE instantiations of the lane kernels, finish_long_k), classify_long_k's histogram and the (rank, count) lists at counts
beyond 2^16, 2^19, 2^20 and 2^24, the vote's arithmetic and the formatter's digits at those counts, frame_k's long-line flag at exactly the
byte where fgets splits, a 16 MiB record carried across the 64 MiB chunk of the device pipeline and the 96 MiB slot of the host pipeline, a
pair joined to exactly LINELEN bases, the rank-specific search with millions of hits in one read and its state grown in mid-file, a hit map
of 2^24 windows and more than 2^20 runs, coverage of a read that hits one word millions of times.

Every comparison is equality: all six record words, or the bytes of a file.  MID cases come before LMAX cases.

What reaches what:
  fasta.c's giant path, frame_k's long-line edge   test_whole_file_search_at_the_line_limit (max_plus_one, max_header_plus, lower_crlf leave the
                                                   device pipeline; one_max, max_header, lower_crlf_whole -- one byte less -- stay), the CLI test;
                                                   tests/test_long_cpu.py: test_host_framing_splits_lines_as_fgets_does
  a 16 MiB carry                                   test_whole_file_search_at_the_line_limit[five_max-device] (64 MiB chunks), [five_max-host] (96 MiB slots)
  pieces_k / classify_long_pieces at scale         test_reads_of_2_20_windows[*-1] (509 pieces at k = 32, 676 at k = 64), test_reads_at_the_line_limit (8 129 pieces),
                                                   test_one_maximal_read_among_short_ones
  large counts                                     the same tests: ltab_cnt with lane pass 1, classify_long_k's histogram with 0; found = 33 554 366;
                                                   test_a_pair_of_exactly_a_line_is_classified
  rank-specific search at scale                    test_rank_search_with_millions_of_hits_in_one_read
  hit map and coverage                             test_hit_map_and_coverage_of_maximal_reads

What would fail them: frame_k comparing a line with LINELEN instead of LINELEN - 1 keeps max_plus_one (a line of exactly LINELEN bytes) on
the device: st.pipeline == 1, exit code 0 and one read of LMAX + 1 bases instead of the reference's split and exit 2.  A 16-bit ltab_cnt or
histogram count wraps at MID already (2^20 hits of one label); a 24-bit one holds a strand of LMAX (16 777 183) but not dense, mixed and
n_every with both strands (33.5 M, 18.9 M of label 0).  A reader that drops what is left of a chunk behind the last whole record, instead
of moving it to the front of the next (search_reader.c: R->carry; search_dev.c looks for the next record start), loses or cuts the record
that straddles 64 MiB / 96 MiB in five_max: its line is missing or its count differs.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, frame_fasta, search_gg, search_rank
import coverage_ref
import hitmap_ref
import long_inputs as li
from test_gpu_tally_inline import assert_records, records


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_CASES, _TREES = {}, {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("long")
    yield d
    for db, tree in _TREES.values():
        tree.close()
        db.close()
    _TREES.clear()
    for c in _CASES.values():
        c.o.close()
        if os.path.exists(c.built.ctr):
            os.remove(c.built.ctr)
    _CASES.clear()


class Case:
    """One database, made once per module and never changed; its inputs and the oracle's answers, made when first asked for (a maximal
    record costs the oracle a second per strand mode: every answer is computed once)."""

    def __init__(self, name, workdir):
        self.built = li.build(name, workdir)
        self.o = orc.OracleDB.load(self.built.ctr)
        self.k = self.built.k
        self.dir = workdir
        self._batch, self._file, self._text = {}, {}, {}

    def batch(self, n):
        """(FASTA of the five read kinds at n bases, its framing, {rc: the oracle's records}); one length at a time is kept"""
        if n not in self._batch:
            self._batch.clear()
            data = li.batch_fasta(self.built, n)
            fr = frame_fasta(data)
            buf = np.frombuffer(data, dtype=np.uint8)
            self._batch[n] = (data, fr, {rc: self.o.classify_batch(buf, fr["seq_off"], fr["seq_len"], rc=rc, threads=5) for rc in (False, True)})
        return self._batch[n]

    def file(self, fname):
        """path of the file (written once)"""
        p = self.dir / ("%s_%s.fa" % (self.built.name, fname))
        if fname not in self._file:
            p.write_bytes(li.file_bytes(self.built, fname))
            self._file[fname] = str(p)
        return self._file[fname]

    def text(self, fname, rc, rank=False, **prm):
        """(exit code, bytes) of the oracle's search of the file"""
        key = (fname, rc, rank, tuple(sorted(prm.items())))
        if key not in self._text:
            out = self.dir / "oracle.txt"
            if out.exists():
                out.unlink()
            if rank:
                code, nr, good, err = orc.rank_search_file(self.o, self.file(fname), str(out), rc=rc, **prm)
            else:
                code, nr, good, err = self.o.search_file(self.file(fname), str(out), threads=8, rc=rc)
            assert good > 0, err
            self._text[key] = (code, out.read_bytes(), nr)
        return self._text[key]


def case(name, workdir):
    if name not in _CASES:
        _CASES[name] = Case(name, workdir)
    return _CASES[name]


def tree_for(name, workdir):
    """The handle of a kind, kept for the module (a handle that has searched a file keeps its lanes' buffers: at most two are open)."""
    if name not in _TREES:
        while len(_TREES) >= 2:
            db, tree = _TREES.pop(next(iter(_TREES)))
            tree.close()
            db.close()
        db = CtrDB.open(case(name, workdir).built.ctr)
        tree = DeviceTree.upload(db, 0)
        assert tree.info.irregular_bins == 0 and not tree.info.generic_mode and tree.info.lane_pass == li.LANE_PASS[name]
        _TREES[name] = (db, tree)
    return _TREES[name]


def set_lane_pass(monkeypatch, lane_pass):
    if lane_pass is None:
        monkeypatch.delenv("UTREE_LANE_PASS", raising=False)
    else:
        monkeypatch.setenv("UTREE_LANE_PASS", lane_pass)


def check_batch(torch, c, tree, n, lane_pass, monkeypatch):
    """The five read kinds at n bases in one batch, both strand modes: all six record words, and the kernels that ran -- the pieces pass
    (classify_lanes_k<W, I, 16, ...>) where the handle has a lane pass and it is on, else classify_long_k."""
    set_lane_pass(monkeypatch, lane_pass)
    data, fr, want = c.batch(n)
    W, I = c.k // 4, c.built.I
    for rc in (False, True):
        got = records(torch, tree, data, fr, rc)
        name = tree.kernel_name()
        if tree.info.lane_pass and lane_pass != "0":
            assert name.startswith("classify_lanes_k<%d, %d, 16, false, 2," % (W, I)), name
        else:
            assert "classify_long_k" in name, name
        print(c.built.name, n, rc, lane_pass, name, got.view(np.uint32)[:, 2].tolist())
        assert_records(got, want[rc], (c.built.name, n, rc, lane_pass))


# ---- 1. the classify API: MID, then LMAX ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lane_pass", ["1", "0"])
@pytest.mark.parametrize("name", list(li.KINDS))
def test_reads_of_2_20_windows(torch_cuda, workdir, monkeypatch, name, lane_pass):
    """MID = 2^20 forward windows: 509 pieces at k = 32 (676 at k = 64), more than a workgroup's threads; one label's count reaches 2^20
    (2^21 with both strands): beyond the 13, 16 and 19 bits the lane pass packs short reads' counts into."""
    c = case(name, workdir)
    db, tree = tree_for(name, workdir)
    assert li.n_pieces(li.mid(c.k), c.k) > 256
    check_batch(torch_cuda, c, tree, li.mid(c.k), lane_pass, monkeypatch)


@pytest.mark.parametrize("name,lane_pass", [("k32", "1"), ("k32", "0"), ("k32u32", None), ("k64", None), ("k64u32", None), ("k16", None)])
def test_reads_at_the_line_limit(torch_cuda, workdir, monkeypatch, name, lane_pass):
    """LMAX = 16 777 214 bases: 8 129 pieces at k = 32; dense with both strands has found = 33 554 366 (25 bits) in one label, mixed three labels
    beyond 2^20 and the vote's cut at those counts.  k = 32 / u16 through both kernel families, the other kinds through their default."""
    c = case(name, workdir)
    db, tree = tree_for(name, workdir)
    check_batch(torch_cuda, c, tree, li.LMAX, lane_pass, monkeypatch)
    _, _, want = c.batch(li.LMAX)
    assert int(want[True]["found"][0]) >= 1 << 24


@pytest.mark.parametrize("rc", [False, True])
def test_one_maximal_read_among_short_ones(torch_cuda, workdir, monkeypatch, rc):
    """The mixed launch: 4000 reads of 150 bases (one lane), a few of 3 .. 12 kb (sixteen lanes, or pieces) and one of LMAX bases in one
    batch: the class lists, then the pieces, then the left-overs."""
    c = case("k32", workdir)
    db, tree = tree_for("k32", workdir)
    monkeypatch.delenv("UTREE_LANE_PASS", raising=False)
    data = li.mixed_batch(c.built)
    fr = frame_fasta(data)
    assert len(fr["seq_len"]) == 4006 and int(fr["seq_len"].max()) == li.LMAX and int((fr["seq_len"] == 150).sum()) == 4000
    want = c.o.classify_batch(np.frombuffer(data, dtype=np.uint8), fr["seq_off"], fr["seq_len"], rc=rc, threads=8)
    got = records(torch_cuda, tree, data, fr, rc)
    assert tree.kernel_name().startswith("classify_lanes_k<8, 2, 16, false, 2,"), tree.kernel_name()
    assert_records(got, want, ("mixed batch", rc))
    assert int((want["found"] > 0).sum()) > 3000


# ---- 2. the whole-file search ----------------------------------------------------------------------------------------------------------------
# file: the pipeline that must finish it without UTREE_HOST_TEXT (1: framed and formatted on the device; 0: handed to the host framing)
PIPELINE = {"one_max": 1, "five_max": 1, "last_no_newline": 1, "lower_crlf_whole": 1, "max_header": 1,
            "max_plus_one": 0, "max_header_plus": 0, "lower_crlf": 0}
CODE = {0: lib.OK, 2: lib.E_FASTA}


@pytest.mark.parametrize("host_text", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("fname", li.FILES)
def test_whole_file_search_at_the_line_limit(torch_cuda, workdir, tmp_path, monkeypatch, fname, host_text):
    """utree_search_run on every file of long_inputs, both strand modes: the oracle's exit code and output bytes.  A line of LINELEN - 1 bytes
    with its newline (one_max, five_max, max_header, lower_crlf_whole) is the longest fgets returns whole and stays on the device text
    pipeline; one byte more (max_plus_one, max_header_plus, lower_crlf) raises frame_k's long-line flag and the host framing splits it as
    the reference does.  five_max: 84 MB, records carried whole across the 64 MiB device chunk and, with UTREE_HOST_TEXT, the 96 MiB slot."""
    c = case("k32", workdir)
    db, tree = tree_for("k32", workdir)
    if host_text:
        monkeypatch.setenv("UTREE_HOST_TEXT", "1")
    else:
        monkeypatch.delenv("UTREE_HOST_TEXT", raising=False)
    for rc in (False, True):
        code, want, nr = c.text(fname, rc)
        out = tmp_path / "o.txt"
        got_code, st = search_gg(db, [tree], c.file(fname), str(out), rc=rc, threads=8)
        print(fname, host_text, rc, got_code, st.pipeline, st.n_reads, st.fasta_error.code, st.fasta_error.read_index)
        assert got_code == CODE[code], (fname, rc, got_code)
        assert out.read_bytes() == want, (fname, rc)
        assert st.pipeline == (0 if host_text else PIPELINE[fname]), (fname, rc, st.pipeline)
        assert st.n_reads == nr
        if code:
            assert (st.fasta_error.code, st.fasta_error.read_index) == (2, nr + 1)


def test_cli_on_a_line_one_byte_too_long(torch_cuda, workdir, tmp_path):
    """xtree-searchGG on max_plus_one: the reference's exit code 2, and the records in front of the error written."""
    c = case("k32", workdir)
    code, want, nr = c.text("max_plus_one", True)
    out = tmp_path / "cli.txt"
    env = dict(os.environ, UTREE_GPUS="1")
    env.pop("UTREE_HOST_TEXT", None)
    r = subprocess.run([lib.CLI_PATH, c.built.ctr, c.file("max_plus_one"), str(out), "4", "RC"], env=env, capture_output=True, timeout=300)
    assert r.returncode == code == 2, r.stderr.decode(errors="replace")[-2000:]
    assert out.read_bytes() == want


def test_fastq_gzip_and_wrapped_fasta_at_the_line_limit(torch_cuda, workdir, tmp_path):
    """The opt-in formats are not framed by fgets: a FASTQ record whose sequence and quality lines both have LMAX bytes -- plain and gzip --
    and one_max wrapped at 70 columns are framed whole and give the lines of the two-line FASTA (include/utree_amd.h)."""
    c = case("k32", workdir)
    db, tree = tree_for("k32", workdir)
    data = open(c.file("one_max"), "rb").read()
    fr = frame_fasta(data)
    recs = [(data[int(a):int(a) + int(b)], data[int(s):int(s) + int(l)]) for a, b, s, l in zip(fr["name_off"], fr["name_len"], fr["seq_off"], fr["seq_len"])]
    assert max(len(s) for _, s in recs) == li.LMAX
    fq = b"".join(b"@" + n + b" some text\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in recs)
    wrapped = b"".join(b">" + n + b"\n" + b"\n".join(s[a:a + 70] for a in range(0, len(s), 70)) + b"\n" for n, s in recs)
    inputs = {"fq": (lib.INPUT_FASTQ, fq), "fq.gz": (lib.INPUT_FASTQ, gzip.compress(fq, 1)), "wrapped.fa": (lib.INPUT_FASTA_MULTILINE, wrapped),
              "auto.fq.gz": (lib.INPUT_AUTO, gzip.compress(fq, 1))}
    for rc in (False, True):
        code, want, nr = c.text("one_max", rc)
        for tag, (fmt, blob) in inputs.items():
            if rc and tag != "fq":
                continue
            p, out = tmp_path / ("in." + tag), tmp_path / "o.txt"
            p.write_bytes(blob)
            got_code, st = search_gg(db, [tree], str(p), str(out), rc=rc, threads=8, input_format=fmt)
            assert got_code == lib.OK and st.n_reads == nr, (tag, rc, got_code)
            assert out.read_bytes() == want, (tag, rc)
            p.unlink()


# ---- 3. pairs ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True])
def test_a_pair_of_exactly_a_line_is_classified(torch_cuda, workdir, tmp_path, rc):
    """Mate 1 + N + mate 2 of exactly LINELEN bases is the longest pair: classified as the oracle classifies the joined read (one base more is
    the framing error tests/test_gpu_pairs.py holds)."""
    c = case("k32", workdir)
    db, tree = tree_for("k32", workdir)
    b = c.built
    n1 = li.LINELEN // 2
    m1, m2 = li.read(b, "dense", n1), li.read(b, "mixed", li.LINELEN - 1 - n1)
    sh = li.short_reads(b, 6, 77)
    names = [b"p0", b"p1", b"long", b"p3"]
    first = [sh[0], sh[1], m1, sh[2]]
    second = [sh[3], sh[4], m2, sh[5]]
    assert len(m1) + 1 + len(m2) == li.LINELEN
    want = b""
    for nm, a, z in zip(names, first, second):
        r = c.o.classify_read(a.tobytes() + b"N" + z.tobytes(), rc=rc)
        want += c.o.format(nm, r)
    rp, mp, out = tmp_path / "r1.fa", tmp_path / "r2.fa", tmp_path / "o.txt"
    rp.write_bytes(li.fasta(list(zip(names, first))))
    mp.write_bytes(li.fasta([(nm + b"/2", s) for nm, s in zip(names, second)]))
    code, st = search_gg(db, [tree], str(rp), str(out), rc=rc, threads=4, mates=str(mp))
    assert code == lib.OK and st.n_reads == 4, (code, st.fasta_error.code)
    assert out.read_bytes() == want and want.count(b"\n") == 4


# ---- 4. the rank-specific search -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fname,prm", [("k32", "one_max", {}), ("k32", "five_max", {}), ("k32", "one_max", {"sparsity": 1}),
                                            ("k64", "one_max", {}), ("k32u32", "one_max", {})],
                         ids=["k32-one_max", "k32-five_max", "k32-one_max-sparsity1", "k64-one_max", "k32u32-one_max"])
@pytest.mark.parametrize("rc", [False, True])
def test_rank_search_with_millions_of_hits_in_one_read(torch_cuda, workdir, tmp_path, name, fname, prm, rc):
    """xtree-search on a maximal record between short reads, both strands: hundreds of thousands of kept hits in one read, more than a million
    in five_max with both strands (rank_vote_k<true>'s histogram), rank_state grown from 4 096 entries in the middle of a file, and the reads
    after it pick their extra entry from that state.  Once with sparsity = 1.  (The hit counts: tests/test_long_cpu.py,
    test_rank_search_keeps_a_million_hits.)"""
    c = case(name, workdir)
    db, tree = tree_for(name, workdir)
    code, want, nr = c.text(fname, rc, rank=True, **prm)
    out = tmp_path / "rank.txt"
    got_code, st = search_rank(db, tree, c.file(fname), str(out), rc=rc, threads=8, **prm)
    assert got_code == lib.OK and code == 0 and st.n_reads == nr
    assert out.read_bytes() == want, (name, fname, rc, prm)


# ---- 5. hit map and coverage -------------------------------------------------------------------------------------------------------------------------
HM_READS = ("striped", "striped_fine", "dense", "sparse")
_HM = {}


def hm_case(c, rc):
    """the three maximal reads, and the models' answers through the oracle's batch lookup (computed once)"""
    if "seqs" not in _HM:
        _HM["seqs"] = [li.read(c.built, kind, li.LMAX) for kind in HM_READS]
    if rc not in _HM:
        runs = [hitmap_ref.runs_arrays(hitmap_ref.codes_batch(c.o, s, rc)) for s in _HM["seqs"]]
        _HM[rc] = (runs, coverage_ref.coverage_counts_batch(c.built.ctr, _HM["seqs"], rc))
    return _HM["seqs"], _HM[rc][0], _HM[rc][1]


def map_file(names, runs):
    out = []
    for nm, (code, count) in zip(names, runs):
        hit = code < hitmap_ref.INVALID
        toks = b" ".join(hitmap_ref.token(a, b) for a, b in zip(code.tolist(), count.tolist()))
        out.append(b"%s\t%d\t%d\t%s\n" % (nm, int(count.sum()), int(count[hit].sum()), toks))
    return b"".join(out)


@pytest.mark.parametrize("rc", [False, True])
def test_hit_map_and_coverage_of_maximal_reads(torch_cuda, workdir, tmp_path, rc):
    """utree_hitmap_batch and utree_coverage_add on striped, striped_fine, dense and sparse at LMAX, then the same reads through the file
    search with hitmap= and coverage=: 2^24 windows per strand in one query, more than 2^20 runs in one line (striped_fine with both
    strands), the longest run a line can hold (dense: LMAX - k + 1 windows), a read that hits 37 words 16 M times."""
    torch = torch_cuda
    c = case("k32", workdir)
    db, tree = tree_for("k32", workdir)
    seqs, runs, (dbk, cov, hits, texts) = hm_case(c, rc)
    assert int(runs[2][1].max()) == li.LMAX - c.k + 1 > (1 << 24) - 64                  # the longest run a line can hold: all 24 bits
    if rc:
        assert len(runs[1][0]) > 1 << 20
    ln = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln.astype(np.int64))[:-1]]).astype(np.int64)
    t = (torch.from_numpy(np.concatenate(seqs + [np.zeros(1, np.uint8)])).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda())
    run_off, got, meta = tree.hitmap(*t, rc=rc)
    want_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in runs])])
    assert meta == dict(total_runs=int(want_off[-1]), total_windows=int(sum(int(b.sum()) for _, b in runs)), error=0)
    assert np.array_equal(run_off.cpu().numpy(), want_off)
    g = got.cpu().numpy().view(np.uint32)[:int(want_off[-1])]
    assert np.array_equal(g[:, 0], np.concatenate([a for a, _ in runs])) and np.array_equal(g[:, 1], np.concatenate([b for _, b in runs]).astype(np.uint32))
    del got, g
    cv = tree.coverage()
    cv.add(*t, rc=rc)
    torch.cuda.synchronize()
    e, nr, nh = cv.entries()
    cv.close()
    assert nr == len(seqs) and nh == int(hits.sum()) and int(hits.max()) > 1 << 24
    assert np.array_equal(e["db_kmers"], dbk) and np.array_equal(e["covered"], cov) and np.array_equal(e["hits"], hits)
    del t
    # the file search with both reports
    names = [kind.encode() for kind in HM_READS]
    fa, out, hm, cf = tmp_path / "hm.fa", tmp_path / "o.txt", tmp_path / "map.tsv", tmp_path / "cov.tsv"
    fa.write_bytes(li.fasta(list(zip(names, seqs))))
    code, st = search_gg(db, [tree], str(fa), str(out), rc=rc, threads=8, hitmap=str(hm), coverage=str(cf))
    assert code == lib.OK and st.n_reads == len(seqs)
    assert cf.read_bytes() == coverage_ref.coverage_file(dbk, cov, hits, texts, len(seqs))
    assert hm.read_bytes() == map_file(names, runs)
    res = c.o.classify_batch(np.frombuffer(fa.read_bytes(), dtype=np.uint8), *[frame_fasta(fa.read_bytes())[k] for k in ("seq_off", "seq_len")], rc=rc, threads=4)
    assert out.read_bytes() == b"".join(c.o.format(nm, orc.Result(*[int(x) for x in r])) for nm, r in zip(names, res))
