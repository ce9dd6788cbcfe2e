"""Reads at the reference's 16 MiB line limit (tests/long_inputs.py), the part that needs no GPU.

1. The CPU oracle against the genuine reference: every file of long_inputs on every record format, both strand modes, xtree-searchGG and
   xtree-search (golden/reference_runs.json, `make_golden.py reference_runs long`: only hashes are committed, and for the runs that end in
   an error the lines the reference printed).  The inputs rebuilt here are the ones the reference ran on.
2. The library's host framing (utree_fasta_frame, the giant path of csrc/fasta.c: a line of LINELEN - 1 bytes or more is split as fgets
   splits it) against a plain model of two fgets per record and against the oracle's error, parallel and with UTREE_FRAME_SERIAL.
3. The conditions that give tests/test_gpu_long.py its meaning, from the oracle's own records.
4. The vectorised paths of hitmap_ref / coverage_ref (OracleDB.lookup_batch) against their per-window forms on the fixtures those are
   pinned on.
No GPU.
"""
import os
import re

import numpy as np
import pytest

from oracle import orc
from utree_amd.search import frame_fasta
import coverage_ref
import hitmap_ref
import long_inputs as li
import util

_BUILT = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("long_cpu")
    yield d
    for b, o in _BUILT.values():
        o.close()
        os.remove(b.ctr)
    _BUILT.clear()


def built(name, workdir):
    if name not in _BUILT:
        b = li.build(name, workdir)
        _BUILT[name] = (b, orc.OracleDB.load(b.ctr))
    return _BUILT[name]


# ---- 1. the oracle against the reference -----------------------------------------------------------------------------------------------
ERR_KIND = {"can't read sequence": 1, "no header": 2, "sequence begins": 3, "empty query": 4}


def oracle_error(err):
    """(code as utree_fasta_error counts them, record number) of the oracle's message"""
    kind = [c for t, c in ERR_KIND.items() if t in err]
    return kind[0], int(re.findall(r"(\d+)", err)[-1])


@pytest.mark.parametrize("fname", li.FILES)
@pytest.mark.parametrize("name", list(li.KINDS))
def test_oracle_equals_reference_at_the_line_limit(name, fname, workdir):
    """The oracle writes the reference's bytes and ends as the reference ends: LMAX bases are read whole, LMAX + 1 are split and the search
    stops with `no header` at the record after, exit 2, the records before it written."""
    b, o = built(name, workdir)
    ctr_sha = util.sha256_of(b.ctr)
    data = li.file_bytes(b, fname)
    fa, out = workdir / "r.fa", workdir / "o.txt"
    fa.write_bytes(data)
    for rank in (False, True):
        if rank and name not in li.RANK_RUNS:
            continue
        for rc in (False, True):
            want = util.reference_run(li.run_key(name, fname, rc, rank), fa=data)
            assert want["inputs"]["ctr"] == ctr_sha, "the database is not the one the reference was run on"
            assert want["exit"] == (2 if fname in li.SPLITS else 0)
            if out.exists():
                out.unlink()
            if rank:
                code, nr, good, err = orc.rank_search_file(o, str(fa), str(out), rc=rc)
            else:
                code, nr, good, err = o.search_file(str(fa), str(out), threads=4, rc=rc)
            assert code == want["exit"], (name, fname, rc, rank, err)
            assert util.sha256_of(str(out)) == want["outputs"]["out"], (name, fname, rc, rank)
            assert good == out.read_bytes().count(b"\n") and (good > 0 or fname == "max_header_plus")     # (there one short read precedes the error)
            if code:
                # the reference's own message, "ERROR: no header '>' [L 4, '<the line>']": kind and record number
                assert any(line.startswith(err.strip().rstrip("]")) for line in want["stderr"]), (err, want["stderr"])
    fa.unlink()


# ---- 2. the host framing's giant path ----------------------------------------------------------------------------------------------------
def find_name_end(data, pos, hl):
    """end of the name that starts at pos + 1: the first space, newline or NUL of the header line (a 16 MiB name: no Python loop)"""
    ends = [j for j in (data.find(c, pos + 1, pos + hl) for c in (b" ", b"\n", b"\0")) if j >= 0]
    return min(ends) if ends else pos + hl


def fgets_model(data):
    """Two fgets(line, LINELEN, in) per record (itree.c:866-890): ([(name_off, name_len, seq_off, seq_len)], error code, its record number)."""
    n, pos, recs = len(data), 0, []

    def line(at):
        lim = min(n - at, li.LINELEN - 1)
        j = data.find(b"\n", at, at + lim)
        return j + 1 - at if j >= 0 else lim
    while pos < n:
        hl = line(pos)
        spos = pos + hl
        if spos >= n:
            return recs, 1, len(recs)
        sl = line(spos)
        if data[pos] != 0x3E:
            return recs, 2, len(recs) + 1
        e = find_name_end(data, pos, hl)
        if data[spos] == 0x3E:
            return recs, 3, len(recs) + 1
        z = data.find(b"\0", spos, spos + sl)
        length = z - spos if z >= 0 else sl
        if not length:
            return recs, 4, len(recs) + 1
        if data[spos + length - 1] == 0x0A:
            length -= 1
        if length and data[spos + length - 1] == 0x0D:
            length -= 1
        recs.append((pos + 1, e - pos - 1, spos, length))
        pos = spos + sl
    return recs, 0, 0


@pytest.mark.parametrize("fname", ["max_plus_one", "max_header", "max_header_plus", "lower_crlf", "lower_crlf_whole", "one_max", "last_no_newline"])
def test_host_framing_splits_lines_as_fgets_does(fname, workdir, monkeypatch):
    """utree_fasta_frame on a line of LINELEN - 2, LINELEN - 1 and LINELEN bytes (sequence and header; LF and CRLF): the spans of the model,
    the oracle's error and record number -- by the parallel framing (which must notice the giant line and step aside) and by the serial one."""
    b, o = built("k32", workdir)
    data = li.file_bytes(b, fname)
    fa, out = workdir / "f.fa", workdir / "f.txt"
    fa.write_bytes(data)
    code, nr, good, err = o.search_file(str(fa), str(out), threads=4, rc=False)
    fa.unlink()
    recs, ecode, eread = fgets_model(data)
    want_err = (ecode, eread)
    assert (code != 0) == (want_err[0] != 0) == (fname in li.SPLITS)
    if code:
        assert oracle_error(err) == want_err == (2, nr + 1)
    assert nr == len(recs)
    longest = max(r[3] for r in recs)
    # (lower_crlf: fgets returns LMAX bases and the '\r', which is stripped; max_header_plus: the record of the long header has no bases)
    assert longest == {"max_plus_one": li.LINELEN - 1, "lower_crlf": li.LMAX, "lower_crlf_whole": li.LMAX - 1, "max_header": 4000,
                       "max_header_plus": 150}.get(fname, li.LMAX)
    if fname == "max_header_plus":
        assert recs[1][1:] == (li.LINELEN - 2, recs[1][2], 0) and recs[1][2] == recs[1][0] + li.LINELEN - 2
    for serial in (False, True):
        if serial:
            monkeypatch.setenv("UTREE_FRAME_SERIAL", "1")
        else:
            monkeypatch.delenv("UTREE_FRAME_SERIAL", raising=False)
        fr = frame_fasta(data, final=True)
        got = list(zip(fr["name_off"].tolist(), fr["name_len"].tolist(), fr["seq_off"].tolist(), fr["seq_len"].tolist()))
        assert got == recs, (fname, serial)
        assert (fr["error_code"], fr["error_read"] if fr["error_code"] else 0) == want_err, (fname, serial)


def test_fgets_model_on_small_records():
    """The model itself on the cases whose answer is known by hand."""
    assert fgets_model(b">a b\nACGT\n>c\nAC\r\n") == ([(1, 1, 5, 4), (11, 1, 13, 2)], 0, 0)
    assert fgets_model(b">a\nACGT\nACGT\n")[1:] == (1, 1)
    assert fgets_model(b">a\nACGT\nx\nACGT\n")[1:] == (2, 2)
    assert fgets_model(b">a\n>b\n")[1:] == (3, 1)
    assert fgets_model(b">a\n\0\n")[1:] == (4, 1)
    assert fgets_model(b">a\nACGT") == ([(1, 1, 3, 4)], 0, 0)


# ---- 3. the generator's conditions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(li.KINDS))
def test_reads_are_what_the_module_says(name, workdir):
    """dense with both strands at LMAX: found >= 2^24; mixed at LMAX: four labels, three of them with >= 2^20 hits; striped: the five labels;
    sparse: a hit in the first and in the last window; every read of the MID set: more than 256 pieces."""
    b, o = built(name, workdir)
    k = b.k
    assert li.n_pieces(li.mid(k), k) > 256 and li.mid(k) - k + 1 == 1 << 20
    assert li.N_PERIOD % 2 and all(li.piece_windows(kk) % li.N_PERIOD for kk in (16, 32, 64))
    for n in (li.mid(k), li.LMAX):
        data = li.batch_fasta(b, n)
        fr = frame_fasta(data)
        assert fr["seq_len"].tolist() == [n] * 5
        buf = np.frombuffer(data, dtype=np.uint8)
        fwd = o.classify_batch(buf, fr["seq_off"], fr["seq_len"], rc=False, threads=5)
        both = o.classify_batch(buf, fr["seq_off"], fr["seq_len"], rc=True, threads=5)
        w = dict(zip(li.READ_KINDS, fwd))
        assert int(w["dense"]["found"]) == n - k + 1 and int(w["dense"]["uix"]) == 1            # every window hits
        assert int(both[0]["found"]) == 2 * (n - k + 1)
        assert int(w["mixed"]["uix"]) == 4 and int(w["striped"]["uix"]) == 5
        assert int(w["n_every"]["found"]) < n - k + 1 - (n // li.N_PERIOD) * (k - 1) + k        # each N takes k windows
        if n == li.LMAX:
            assert int(both[0]["found"]) >= 1 << 24
            seq = buf[int(fr["seq_off"][1]):int(fr["seq_off"][1]) + n]
            c = hitmap_ref.codes_batch(o, seq, False)
            per = np.bincount(c[c < o.n_labels], minlength=5)
            assert sorted(per.tolist(), reverse=True)[2] >= 1 << 20 and int((per > 0).sum()) == 4
            # the junction windows miss (a few of them hit where the next unit happens to go on as the last one would)
            assert 3 * (k - 1) - 12 <= int((c == hitmap_ref.MISS).sum()) <= 3 * (k - 1)
        seq = buf[int(fr["seq_off"][3]):int(fr["seq_off"][3]) + n]                              # sparse
        c = hitmap_ref.codes_batch(o, seq, False)
        assert c[0] < o.n_labels and c[-1] < o.n_labels and n // li.SPARSE_STEP <= int((c < o.n_labels).sum()) < n // 10000


def test_rank_search_keeps_a_million_hits(workdir):
    """The rank-specific search looks up one window in 32: a maximal read keeps 2^19 hits a strand (2^18 at k = 64), dense and n_every in
    five_max with both strands more than 2^20 -- what tests/test_gpu_long.py's rank-specific cases rely on."""
    for name, fname, least in (("k32", "five_max", 1 << 20), ("k32", "one_max", 1 << 19), ("k64", "one_max", 1 << 18), ("k32u32", "one_max", 1 << 19)):
        b, o = built(name, workdir)
        data = li.file_bytes(b, fname)
        fr = frame_fasta(data)
        rs = orc.RankSearch(o)
        r = rs.read_batch(np.frombuffer(data, dtype=np.uint8), fr["seq_off"], fr["seq_len"], rc=True)
        rs.close()
        assert int(r["found"].max()) > least, (name, fname, r["found"].tolist())
        if fname == "five_max":
            assert int((r["found"] > 1 << 20).sum()) == 2 and r["found"][-1] > 0            # (and the short read behind them still finds its entry)


def test_striped_runs(workdir):
    """striped at LMAX: a run of hits and a run of misses per stripe of 64 + k bases, 2 * LMAX / 96 of them per strand at k = 32.  A stripe
    cannot be shorter than k bases, so one strand of a read has at most LMAX / 16 < 2^20 runs; striped_fine (2 + k bases) with both strands
    has more than 2^20.  dense has the longest run a line can hold: LMAX - k + 1 windows, all 24 bits of a count (the N between the
    strands ends it: no run needs 25)."""
    b, o = built("k32", workdir)
    code, count = hitmap_ref.runs_arrays(hitmap_ref.codes_batch(o, li.read(b, "striped", li.LMAX), False))
    assert len(code) >= 2 * (li.LMAX // (64 + b.k)) - 1 > 1 << 18 and set(code[code < hitmap_ref.INVALID].tolist()) == {0, 1, 2, 3, 4}
    code, count = hitmap_ref.runs_arrays(hitmap_ref.codes_batch(o, li.read(b, "striped_fine", li.LMAX), True))
    assert len(code) > 1 << 20
    code, count = hitmap_ref.runs_arrays(hitmap_ref.codes_batch(o, li.read(b, "dense", li.LMAX), True))
    assert code.tolist() == [0, hitmap_ref.INVALID, 0] and int(count[0]) == int(count[2]) == li.LMAX - b.k + 1 > (1 << 24) - 64


# ---- 4. the models' vectorised paths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "vote", "ix32", "k64", "k64ix32", "k16"])
def test_batch_lookup_equals_the_per_window_hit_map(name):
    """hitmap_ref.codes_batch / runs_arrays == codes / runs_of on the fixtures the per-window form is pinned to the reference on, both strand
    modes: reads with N, lower case, shorter than a window."""
    from test_coverage_cpu import fixture_seqs
    o = orc.OracleDB.load(util.fixture_ctr(name))
    seqs = fixture_seqs(name)
    seqs = seqs[:150] + seqs[-50:] + [b"", b"ACGT", b"N" * 100]
    for rc in (False, True):
        for s in seqs:
            a = hitmap_ref.codes(o, s, rc)
            c = hitmap_ref.codes_batch(o, s, rc)
            assert np.array_equal(a, c)
            code, count = hitmap_ref.runs_arrays(c)
            assert list(zip(code.tolist(), count.tolist())) == hitmap_ref.runs_of(a)
            assert hitmap_ref.query_array(s, rc).tobytes() == hitmap_ref.query(s, rc)


@pytest.mark.parametrize("name,rc", [("toy", 1), ("k64", 0), ("ix32", 0), ("k16", 1), ("katq2", 0)])
def test_batch_lookup_equals_the_per_window_coverage(name, rc):
    """coverage_ref.coverage_counts_batch == coverage_counts (whose figures tests/test_coverage_cpu.py pins to the reference)."""
    from test_coverage_cpu import fixture_seqs
    seqs = fixture_seqs(name)[:400]
    a = coverage_ref.coverage_counts(util.fixture_ctr(name), seqs, bool(rc))
    c = coverage_ref.coverage_counts_batch(util.fixture_ctr(name), seqs, bool(rc))
    assert int(a[2].sum()) > 0 and int(a[1].sum()) > 0
    for x, y in zip(a[:3], c[:3]):
        assert np.array_equal(x, y)
    assert a[3] == c[3]
