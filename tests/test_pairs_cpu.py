"""Paired-end reads, the part that needs no GPU: the committed golden files are what the CPU oracle gives on the joined inputs of
tests/pairs_ref.py (they were written by the genuine reference, tests/golden/make_golden_pairs.py), and the C-ABI carries the new names."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import orc
from utree_amd import lib
import pairs_ref
import util


@pytest.mark.parametrize("name", pairs_ref.FIXTURES)
def test_golden_files_are_the_oracle_on_the_joined_input(name, tmp_path):
    P = pairs_ref.Pairs(name)
    man = pairs_ref.manifest()["fixtures"][name]
    joined = P.joined_fasta()
    assert pairs_ref.sha256(joined) == man["joined_sha256"] and P.n == man["pairs"], "the joined input is not the one the reference ran on"
    o = orc.OracleDB.load(util.fixture_ctr(name))
    fa, out = tmp_path / "joined.fa", tmp_path / "out.txt"
    fa.write_bytes(joined)
    alone = tmp_path / "alone.fa"
    alone.write_bytes(P.reads_fasta())
    for rc in (0, 1):
        code, nr, good, err = o.search_file(str(fa), str(out), threads=1, rc=bool(rc))
        want = pairs_ref.golden(name, rc)
        assert code == 0 and nr == P.n and out.read_bytes() == want
        assert pairs_ref.sha256(want) == man["out_rc_sha256" if rc else "out_sha256"] and good == want.count(b"\n") == man["lines_rc" if rc else "lines"]
        # mate 2 matters: most pairs' lines are not the line of mate 1 searched alone
        code, nr, _, _ = o.search_file(str(alone), str(out), threads=1, rc=bool(rc))
        a, b = pairs_ref.lines_by_name(want, P.names1), pairs_ref.lines_by_name(out.read_bytes(), P.names1)
        differ = sum(1 for i in range(P.n) if a.get(i) != b.get(i))
        assert code == 0 and differ == man["differs_from_mate1"][rc] and 2 * differ > P.n


def test_golden_files_are_no_larger_than_the_fixtures_own_outputs():
    for name in pairs_ref.FIXTURES:
        cap = os.path.getsize(os.path.join(util.GOLD, name + "_out.txt.gz"))
        for rc in ("", "_rc"):
            assert os.path.getsize(os.path.join(util.GOLD, "pairs_%s_out%s.txt.gz" % (name, rc))) <= cap


def test_numpy_join_is_mate1_N_mate2():
    blob = b"ACGTTTGGA"
    out, joff, jlen = pairs_ref.numpy_join(blob, np.array([5, 0, 9]), np.array([4, 0, 0], dtype=np.uint32),
                                           blob, np.array([0, 2, 1]), np.array([2, 3, 0], dtype=np.uint32))
    assert out.tobytes() == b"TGGANAC" + b"NGTT" + b"N" and joff.tolist() == [0, 7, 11] and jlen.tolist() == [7, 4, 1]


def test_new_symbols_and_the_error_code():
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    assert re.search(r"\bUTREE_E_PAIRS\s*=\s*14\b", hdr) and lib.E_PAIRS == 14
    assert re.search(r"#define\s+UTREE_ABI_VERSION\s+4\b", hdr)
    L = lib.load()
    for name in ("utree_pairs_join", "utree_search_pairs_file"):
        assert name in lib.SYMBOLS and hasattr(L, name) and re.search(r"\b%s\(" % name, hdr)
    assert L.utree_abi_version() == 4
    assert b"pair" in L.utree_strerror(lib.E_PAIRS) and L.utree_strerror(15) == b"unknown error"
    assert C.sizeof(lib.PairsMeta) == 16 and lib.PairsMeta.max_len.offset == 8 and lib.PairsMeta.error.offset == 12
    m = re.search(r"typedef struct \{([^}]*)\} utree_pairs_meta;", hdr)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1)) == [("uint64_t", "total_bases"), ("uint32_t", "max_len"), ("uint32_t", "error")]


def test_search_gg_refuses_mates_and_interleaved_together():
    from utree_amd.search import search_gg
    with pytest.raises(ValueError):
        search_gg(None, [], "a.fa", "o.txt", mates="b.fa", interleaved=True)
