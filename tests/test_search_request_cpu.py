"""CPU-only tests of utree_search_request / utree_search_run (include/utree_amd.h): the binding mirrors the header's struct, and every
argument check comes before the first look at `ctr` or a device handle -- the handles given here are NULL or blocks of zero bytes, so a check
that came too late would run on with them and return something else than UTREE_E_ARG (or fault)."""
import ctypes as C
import os
import re

import pytest

from utree_amd import lib
import util


def header_fields():
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"typedef struct \{([^{}]*)\} utree_search_request;", hdr)
    assert m, "include/utree_amd.h declares no utree_search_request"
    names = []
    for decl in m.group(1).split(";"):
        names += [re.search(r"(\w+)\s*$", part).group(1) for part in decl.split(",") if part.strip()]
    return names


def test_binding_mirrors_the_header():
    assert header_fields() == [f[0] for f in lib.SearchRequest._fields_]
    assert header_fields()[0] == "size" and lib.SearchRequest().size == C.sizeof(lib.SearchRequest)
    assert "utree_search_run" in lib.SYMBOLS and hasattr(lib.load(), "utree_search_run")
    assert lib.load().utree_abi_version() == 4


# handles that must not be looked at
CTR = C.create_string_buffer(1 << 16)
DEV = C.create_string_buffer(1 << 16)
PRM = lib.RankParams(2, 4, 2)


def run(n_dev=1, ctr=True, devs=True, **fields):
    base = dict(reads_path=b"/nonexistent/reads.fa", out_path=b"/nonexistent/out.txt")
    base.update(fields)
    size = base.pop("size", None)
    req = lib.SearchRequest(**base)
    if size is not None:
        req.size = size
    arr = (C.c_void_p * 2)(C.addressof(DEV), C.addressof(DEV))
    st = lib.SearchStats()
    return lib.load().utree_search_run(C.addressof(CTR) if ctr else None, arr if devs else None, n_dev, C.byref(req), C.byref(st))


SIZEOF = C.sizeof(lib.SearchRequest)
RANK = dict(rank=C.pointer(PRM))
CASES = {
    "size - 4": dict(size=SIZEOF - 4),
    "size + 8": dict(size=SIZEOF + 8),
    "size 0": dict(size=0),
    "ctr NULL": dict(ctr=False),
    "devs NULL": dict(devs=False),
    "reads_path NULL": dict(reads_path=None),
    "out_path NULL": dict(out_path=None),
    "n_dev 0": dict(n_dev=0),
    "n_dev -1": dict(n_dev=-1),
    "input_format -1": dict(input_format=-1),
    "input_format 4": dict(input_format=lib.INPUT_AUTO + 1),
    "mates and interleaved": dict(mates_path=b"/nonexistent/m.fa", interleaved=1),
    "max_passes 1001, redistribute": dict(redistribute_path=b"/nonexistent/r.tsv", max_passes=1001),
    "max_passes 1001, sample_redistribute": dict(sample_redistribute_path=b"/nonexistent/r.tsv", max_passes=1001),
    "rank, two handles": dict(n_dev=2, **RANK),
    "rank, mates": dict(mates_path=b"/nonexistent/m.fa", **RANK),
    "rank, interleaved": dict(interleaved=1, **RANK),
    "rank, redistribute": dict(redistribute_path=b"/nonexistent/r.tsv", **RANK),
    "rank, hitmap": dict(hitmap_path=b"/nonexistent/h.txt", **RANK),
    "rank, sample_redistribute": dict(sample_redistribute_path=b"/nonexistent/r.tsv", **RANK),
    "rank, coverage": dict(coverage_path=b"/nonexistent/c.tsv", **RANK),
}
for _path in ("samples_path", "sample_redistribute_path"):
    for _d in (-1, 256, ord("\t"), ord(" "), ord("\r"), ord("\n")):
        CASES["sample_delim %d, %s" % (_d, _path)] = {_path: b"/nonexistent/s.tsv", "sample_delim": _d}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_check_comes_before_the_handles(case):
    assert run(**CASES[case]) == lib.E_ARG


def test_the_legacy_entry_points_check_the_same_way():
    """they are utree_search_run with some fields set: the same refusals, the handles as untouched"""
    L = lib.load()
    arr = (C.c_void_p * 1)(C.addressof(DEV))
    st = lib.SearchStats()
    ctr, r, o, m = C.addressof(CTR), b"/nonexistent/reads.fa", b"/nonexistent/out.txt", b"/nonexistent/m.fa"
    assert L.utree_search_file(ctr, arr, 0, r, o, 0, 1, C.byref(st)) == lib.E_ARG
    assert L.utree_search_file_opts(ctr, arr, 1, r, o, 0, 1, 7, C.byref(st)) == lib.E_ARG
    assert L.utree_search_file_redistribute(ctr, arr, 1, r, m, 1, o, 0, 1, 0, None, None, None, 0, C.byref(st)) == lib.E_ARG
    assert L.utree_search_file_redistribute(ctr, arr, 1, r, None, 0, o, 0, 1, 0, None, None, b"/nonexistent/r.tsv", 1001, C.byref(st)) == lib.E_ARG
    assert L.utree_search_file_samples(ctr, arr, 1, r, None, 0, o, 0, 1, 0, None, None, None, 0, None, b"/nonexistent/s.tsv", 9, C.byref(st)) == lib.E_ARG
    assert L.utree_rank_search_file(ctr, None, r, o, 0, C.byref(PRM), 1, C.byref(st)) == lib.E_ARG
    assert L.utree_rank_search_file(ctr, C.addressof(DEV), r, o, 0, None, 1, C.byref(st)) == lib.E_ARG
    assert L.utree_rank_search_file_samples(ctr, C.addressof(DEV), r, o, 0, C.byref(PRM), 1, 0, None, b"/nonexistent/s.tsv", 32, C.byref(st)) == lib.E_ARG
