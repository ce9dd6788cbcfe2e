"""The per-query k-mer hit map, the part that needs no GPU: tests/hitmap_ref.py -- the contract in plain Python -- is pinned to the GENUINE
reference's committed outputs (a map's hit counts sum to column 3 of the read's line, its distinct hit labels number column 4, a read
without a line has no hit), utree_hitmap_format is checked on hand-made runs, and the C-ABI carries the new names."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hitmap_ref
import pairs_ref
import util
from oracle import orc
from test_coverage_cpu import fixture_seqs
from utree_amd import lib

FIXTURES = ("toy", "vote", "ix32", "k64", "k64ix32", "k16")
# the genuine reference's output on the vote fixture with RC (tests/golden/make_golden_vote_rc.py), 4021 lines
VOTE_RC_SHA256 = "42c111585454236230363eeb3cac0041499d2ff0fca9b0cf8886101e92861f41"
_MAPS = {}


def reference_maps(name, rc, n=None):
    """hitmap_ref's maps of the first n reads of a fixture (cached: the GPU tests compare against them too)"""
    key = (name, rc)
    have = _MAPS.get(key, [])
    seqs = fixture_seqs(name)
    n = len(seqs) if n is None else min(n, len(seqs))
    if len(have) < n:
        o = orc.OracleDB.load(util.fixture_ctr(name))
        have = have + hitmap_ref.hitmap(None, seqs[len(have):n], rc, o)
        _MAPS[key] = have
    return have[:n]


def check_against_lines(maps, names, golden):
    lines = pairs_ref.lines_by_name(golden, names)
    assert len(lines) == golden.count(b"\n")
    for i, m in enumerate(maps):
        found, uix = hitmap_ref.found_uix(m)
        if i in lines:
            col = lines[i].split(b"\t")
            assert (found, uix) == (int(col[2]), int(col[3])), (i, lines[i])
        else:
            assert found == 0 and uix == 0, i                       # a read without a line has no hit


# ---- 1. hitmap_ref against the genuine reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rc", [(n, r) for n in FIXTURES for r in (0, 1)])
def test_reference_maps_sum_to_the_genuine_output(name, rc):
    data = util.fixture_bytes(name + "_reads.fa.gz")
    names, _, _ = util.parse_fasta(data)
    maps = reference_maps(name, rc)
    assert len(maps) == len(names)
    if (name, rc) == ("vote", 1):
        assert util.sha256_of(util.fixture_bytes("vote_out_rc.txt.gz")) == VOTE_RC_SHA256
    check_against_lines(maps, names, util.fixture_bytes("%s_out%s.txt.gz" % (name, "_rc" if rc else "")))
    o = orc.OracleDB.load(util.fixture_ctr(name))
    seqs = fixture_seqs(name)
    for s, m in list(zip(seqs, maps))[:200]:                        # the runs cover every window of the query, and no two neighbours are equal
        q = len(s) * 2 + 1 if rc else len(s)
        assert sum(n for _, n in m) == (q - o.k + 1 if q >= o.k else 0)
        assert all(a[0] != b[0] for a, b in zip(m, m[1:])) and all(n > 0 for _, n in m)


@pytest.mark.parametrize("name,rc", [(n, r) for n in pairs_ref.FIXTURES for r in (0, 1)])
def test_reference_maps_of_pairs_sum_to_the_genuine_output(name, rc):
    P = pairs_ref.Pairs(name)
    maps = hitmap_ref.hitmap(util.fixture_ctr(name), P.joined_seqs(), rc)
    check_against_lines(maps, P.names1, pairs_ref.golden(name, rc))
    k = orc.OracleDB.load(util.fixture_ctr(name)).k
    for a, b, m in list(zip(P.seq1, P.seq2, maps))[:50]:            # the k windows around the joining 'N' are invalid
        if not rc and len(a) >= k and len(b) >= k:
            c = np.concatenate([np.full(n, code, dtype=np.int64) for code, n in m])
            assert (c[len(a) - k + 1:len(a) + 1] == hitmap_ref.INVALID).all()


# ---- 2. the formatter ----------------------------------------------------------------------------------------------------------------------
def fmt(names, maps, cap=None, slack=64):
    """utree_hitmap_format on hand-made runs; returns (return value, the output buffer with `slack` guard bytes behind cap)"""
    buf = b"".join(names)
    name_len = np.array([len(n) for n in names], dtype=np.uint32)
    name_off = np.concatenate([[0], np.cumsum(name_len.astype(np.uint64))[:-1]]).astype(np.uint64)
    off, runs = hitmap_ref.flat(maps)
    off = off.astype(np.uint64)
    runs = np.ascontiguousarray(runs, dtype=np.uint32)
    want = hitmap_ref.file_bytes(names, maps)
    if cap is None:
        cap = len(want)
    out = np.full(cap + slack, 0xA5, dtype=np.uint8)
    hb = np.frombuffer(buf + b"\0", dtype=np.uint8)
    r = lib.load().utree_hitmap_format(hb.ctypes.data, name_off.ctypes.data, name_len.ctypes.data, off.ctypes.data,
                                       runs.ctypes.data if len(runs) else None, len(names), out.ctypes.data, cap)
    return r, out, want


M, N = hitmap_ref.MISS, hitmap_ref.INVALID
HAND_NAMES = [b"read/1", b"empty", b"r3", b"big", b"x"]
HAND_MAPS = [[(7, 3), (M, 2), (N, 32), (0, 1), (4294967293, 5)], [], [(M, 119)], [(12, 4294967295), (N, 1234567890)], [(N, 1)]]


def test_format_all_code_kinds_and_an_empty_query():
    r, out, want = fmt(HAND_NAMES, HAND_MAPS)
    assert want == (b"read/1\t43\t9\t7:3 -:2 N:32 0:1 4294967293:5\n" b"empty\t0\t0\t\n" b"r3\t119\t0\t-:119\n"
                    b"big\t5529535185\t4294967295\t12:4294967295 N:1234567890\n" b"x\t1\t0\tN:1\n")
    assert r == len(want) and out[:r].tobytes() == want and (out[r:] == 0xA5).all()
    r, out, want = fmt([], [])
    assert r == 0 and (out == 0xA5).all()


def test_format_cap_one_byte_short():
    full = len(hitmap_ref.file_bytes(HAND_NAMES, HAND_MAPS))
    bad = C.c_size_t(-1).value
    for cap in (full - 1, full - 2, 10, 1, 0):
        r, out, _ = fmt(HAND_NAMES, HAND_MAPS, cap=cap)
        assert r == bad and (out[cap:] == 0xA5).all()               # nothing behind cap was touched
    r, out, want = fmt(HAND_NAMES, HAND_MAPS, cap=full)
    assert r == full and out[:full].tobytes() == want


def test_format_equals_the_reference_on_fixture_maps():
    data = util.fixture_bytes("toy_reads.fa.gz")
    names, _, _ = util.parse_fasta(data)
    maps = reference_maps("toy", 1, 300)
    r, out, want = fmt(names[:300], maps)
    assert r == len(want) and out[:r].tobytes() == want


# ---- 3. the C-ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_the_error_code():
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in ("utree_hitmap_workspace_bytes", "utree_hitmap_batch", "utree_hitmap_format", "utree_search_file_hitmap"):
        assert name in lib.SYMBOLS and hasattr(L, name) and re.search(r"\b%s\(" % name, hdr), name
    assert re.search(r"\bUTREE_E_HITMAP\s*=\s*15\b", hdr) and lib.E_HITMAP == 15
    assert len(L.utree_strerror(15)) > 0
    assert re.search(r"#define\s+UTREE_ABI_VERSION\s+4\b", hdr) and L.utree_abi_version() == 4
    assert re.search(r"#define\s+UTREE_HIT_MISS\s+0xFFFFFFFFu", hdr) and re.search(r"#define\s+UTREE_HIT_INVALID\s+0xFFFFFFFEu", hdr)
    assert (lib.HIT_MISS, lib.HIT_INVALID) == (hitmap_ref.MISS, hitmap_ref.INVALID)
    assert re.search(r"typedef struct \{ uint32_t code, count; \} utree_hit_run;", hdr) and C.sizeof(lib.HitRun) == 8
    assert re.search(r"typedef struct \{ uint64_t total_runs, total_windows; uint32_t error, pad; \} utree_hitmap_meta;", hdr)
    assert C.sizeof(lib.HitmapMeta) == 24 and lib.HitmapMeta.error.offset == 16
    assert L.utree_hitmap_workspace_bytes(None, 1, 1, 0) == 0      # no handle: no size


def test_search_gg_takes_the_path():
    import inspect
    from utree_amd.search import DeviceTree, search_gg
    assert "hitmap" in inspect.signature(search_gg).parameters and callable(DeviceTree.hitmap)
