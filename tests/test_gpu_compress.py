"""`.ubt` -> `.ctr` on the GPU (utree_compress_file / xtree-compress) must write byte-identical
files to the reference's xtree-compress (itree.c:1234-1315).  Expected SHA-256s come from the genuine reference at
golden time (tests/golden/make_golden.py)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from utree_amd import ctrfile, lib
from utree_amd.search import compress
import util


def _ubt_from_db_fixture(name, path):
    d = util.load_db_fixture(name)
    hi, lo = d.words()
    ctrfile.write_ubt(path, d.W, d.I, hi, lo, d.ix(), d.label_text)
    return d


@pytest.mark.parametrize("name", ["toy", "k64", "ix32", "k64ix32", "k16"])
def test_compress_reference_built_databases(name, tmp_path):
    """The toy databases went through the reference's BUILD_GG + COMPRESS; re-compressing their `.ubt` must give the
    same `.ctr` bytes."""
    ubt, ctr = str(tmp_path / "a.ubt"), str(tmp_path / "a.ctr")
    d = _ubt_from_db_fixture(name, ubt)
    code, st = compress(ubt, ctr)
    assert code == lib.OK and st.n_nodes == d.n_nodes and (st.W, st.I) == (d.W, d.I)
    assert ctrfile.sha256_file(ctr) == util.manifest()[name + "_ctr_sha256"]


@pytest.mark.parametrize("name", ["cq_single_first", "cq_multi_first", "cq_dup_labels", "cq_unsorted"])
def test_compress_corner_cases_match_reference(name, tmp_path):
    z = np.load(os.path.join(util.GOLD, name + "_ubt.npz"))
    ubt, ctr = str(tmp_path / "a.ubt"), str(tmp_path / "a.ctr")
    ctrfile.write_ubt(ubt, 8, 2, np.zeros_like(z["lo"]), z["lo"], z["ix"], z["tail"].tobytes())
    r = subprocess.run([lib.COMPRESS_CLI_PATH, ubt, ctr], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    m = util.manifest()
    assert ctrfile.sha256_file(ctr) == m[name + "_ctr_sha256"]
    assert m[name + "_stdout_tail"] in r.stdout.decode()              # "Total nodes in tree: N [L labels]"


def test_compress_large_random_matches_numpy_model(tmp_path):
    """2 M nodes over many chunks: against the numpy model of COMPRESS (ctrfile.binix_like_compress), which
    tests/test_oracle_golden.py pins to the reference's table on the reference-built databases."""
    rng = np.random.default_rng(3)
    lo = np.unique(rng.integers(0, 1 << 63, size=6_000_000, dtype=np.uint64) << np.uint64(1))
    ix = rng.integers(0, 50, size=len(lo)).astype(np.uint32)
    labels = ["k__R;p__%d" % i for i in range(50)]
    cnt = np.bincount(ix, minlength=50)
    tail = b"".join(("%s\t%d\n" % (l, c)).encode() for l, c in zip(labels, cnt))
    ubt, ctr, want = str(tmp_path / "r.ubt"), str(tmp_path / "r.ctr"), str(tmp_path / "w.ctr")
    ctrfile.write_ubt(ubt, 8, 2, np.zeros_like(lo), lo, ix, tail)
    code, st = compress(ubt, ctr)
    assert code == lib.OK and st.n_nodes == len(lo) and st.label_count_total == len(lo)
    ctrfile.write_ctr(want, 8, 2, np.zeros_like(lo), lo, ix, labels, label_counts=cnt, like_compress=True)
    assert ctrfile.sha256_file(ctr) == ctrfile.sha256_file(want)


def test_compress_errors(tmp_path):
    code, _ = compress(str(tmp_path / "missing.ubt"), str(tmp_path / "o.ctr"))
    assert code == lib.E_IO
    p = tmp_path / "bad.ubt"
    p.write_bytes(np.array([8, 0, 2, 0], dtype="<u8").tobytes())
    assert compress(str(p), str(tmp_path / "o.ctr"))[0] == lib.E_FORMAT
    p.write_bytes(np.array([2, 0, 2, 3], dtype="<u8").tobytes() + b"\0" * 64)            # PACKSIZE=8: no build of the reference reads it either
    assert compress(str(p), str(tmp_path / "o.ctr"))[0] == lib.E_UNSUPPORTED


def _chunked_words(W, n, chunk, seed):
    """n unique ascending words: records 0-4 share one 24-bit prefix (the first-bin quirk: `if (!BinIx[v]) BinIx[v] = i` sees record 0 as
    unset), and one prefix straddles every chunk boundary; elsewhere prefixes run for 1-6 records with random gaps between them."""
    rng = np.random.default_rng(seed)
    step = np.where(rng.random(n) < 0.6, 0, rng.integers(1, 4000, n))
    step[:5] = 0
    for b in range(chunk, n, chunk):
        step[max(1, b - 1):b + 2] = 0                                  # records b-2 .. b+1 in one bin
    prefix = np.cumsum(step).astype(np.uint64) + np.uint64(7)
    assert int(prefix[-1]) < (1 << 24)
    run_start = np.flatnonzero(np.concatenate([[True], step[1:] != 0]))
    pos = (np.arange(n) - np.repeat(run_start, np.diff(np.concatenate([run_start, [n]])))).astype(np.uint64)
    assert int(pos.max()) < 256                                        # W = 4: the suffix is one byte
    if W == 4:
        return np.zeros(n, dtype=np.uint64), (prefix << np.uint64(8)) | pos
    if W == 8:
        return np.zeros(n, dtype=np.uint64), (prefix << np.uint64(40)) | (pos << np.uint64(32)) | rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return (prefix << np.uint64(40)) | (pos << np.uint64(32)) | rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 63, n, dtype=np.uint64)


@pytest.mark.parametrize("W,I,sizes", [(16, 4, [(1, 0), (2, 1), (4, 3)]), (4, 2, [(1, 0), (2, 1), (4, 3)]),
                                       (8, 4, [(1, -1), (1, 0), (1, 1), (2, 0), (2, 1), (4, 3)])])        # (a, b): a * chunk + b records
def test_compress_chunk_boundaries(W, I, sizes, tmp_path, monkeypatch):
    """Several chunks per file at W = 16, W = 4 and 4-byte indices, through the hook UTREE_TEST_COMPRESS_CHUNK (records per chunk; a
    production chunk is 32 MiB of records, (32 << 20) // (W + I)): exactly one chunk and one record either side of it, a third chunk in
    the first slot again (2c+1), both slots used twice and a fifth chunk (4c+3).  A bin straddles every boundary, and the first bin holds
    five records, so the kernel's `first` offset, its atomicMin across launches and the first-bin quirk all show in the bin table."""
    c = 1000
    monkeypatch.setenv("UTREE_TEST_COMPRESS_CHUNK", str(c))
    labels = ["k__R;p__%d" % i for i in range(300 if I == 4 else 50)]
    for n in [a * c + b for a, b in sizes]:
        hi, lo = _chunked_words(W, n, c, 100 * W + n % 97)
        ix = np.random.default_rng(n).integers(0, len(labels), n).astype(np.uint32)
        cnt = np.bincount(ix, minlength=len(labels))
        tail = b"".join(("%s\t%d\n" % (l, k)).encode() for l, k in zip(labels, cnt))
        ubt, ctr, want = str(tmp_path / "r.ubt"), str(tmp_path / "r.ctr"), str(tmp_path / "w.ctr")
        ctrfile.write_ubt(ubt, W, I, hi, lo, ix, tail)
        code, st = compress(ubt, ctr)
        assert code == lib.OK and st.n_nodes == n and (st.W, st.I) == (W, I) and st.label_count_total == n
        ctrfile.write_ctr(want, W, I, hi, lo, ix, labels, label_counts=cnt, like_compress=True)
        assert open(ctr, "rb").read() == open(want, "rb").read(), n
