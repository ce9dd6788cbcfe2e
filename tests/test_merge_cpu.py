"""The database merge without a GPU: the surface of the ABI, the argument checks (which come before any file or device is touched), the
layout sniffing (utree_merge_probe, host only), and the yardstick itself -- tests/merge_ref.py, the merge's definition in plain Python, is
pinned here to the GENUINE builder run on the imagined FASTA (oracle's restatement everywhere; oracle/_ref/utree-build* where present)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import merge_ref as M
import util
from oracle import orc
from utree_amd import ctrfile, lib, search

REF = os.path.join(util.ROOT, "oracle", "_ref")


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------------------
def test_names_are_declared_bound_and_exported():
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    L = lib.load()
    for name in ("utree_merge_files", "utree_merge_probe"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in lib.SYMBOLS and hasattr(L, name)
    for t in ("utree_merge_stats", "utree_merge_input"):
        assert "} %s;" % t in hdr
    assert C.sizeof(lib.MergeStats) == 72 and C.sizeof(lib.MergeInput) == 32
    assert lib.MERGE_GG_CLI_PATH.endswith("utree-mergeGG") and lib.MERGE_CLI_PATH.endswith("utree-merge")
    for text in ("itree.c:242-307", "itree.c:1317-1343", "only a rebuild from FASTA is BAD-exact", "sensitivity is that of the sparser one"):
        assert text in hdr, "the header states the definition and both limits"


def test_nothing_else_moved():
    L = lib.load()
    assert L.utree_abi_version() == 4
    assert C.sizeof(lib.SearchRequest) == 128 and lib.SearchRequest._fields_[-1][0] == "redistribute_reads_path"


def test_argument_checks_come_before_any_file(tmp_path):
    L = lib.load()
    out = str(tmp_path / "never.ubt")
    missing = str(tmp_path / "missing.ubt").encode()
    st = lib.MergeStats()

    def call(paths, n, ubt, I):
        arr = (C.c_char_p * max(len(paths), 1))(*paths)
        return L.utree_merge_files(arr, n, ubt, I, 1, 0, C.byref(st))
    assert call([missing], 0, out.encode(), 0) == lib.E_ARG
    assert call([missing], -1, out.encode(), 0) == lib.E_ARG
    assert call([missing, None], 2, out.encode(), 0) == lib.E_ARG
    assert call([missing], 1, None, 0) == lib.E_ARG
    for I in (1, 3, 8, 16):
        assert call([missing], 1, out.encode(), I) == lib.E_ARG              # a file that does not exist would be UTREE_E_IO
    assert L.utree_merge_files(None, 1, out.encode(), 0, 1, 0, C.byref(st)) == lib.E_ARG
    assert L.utree_merge_probe(None, C.byref(lib.MergeInput())) == lib.E_ARG and L.utree_merge_probe(missing, None) == lib.E_ARG
    assert not os.path.exists(out)


# ---- 2. merge_ref against the genuine builder --------------------------------------------------------------------------------------------
def genuine(tmp_path, inputs, gg, I):
    """the `.ubt` bytes of the builder(s) on the imagined FASTA at compression level 0: {who: bytes}"""
    W = inputs[0].W
    fa, mp = M.imagined(inputs)
    fa_p, mp_p = str(tmp_path / "im.fa"), str(tmp_path / "im.map")
    open(fa_p, "wb").write(fa)
    open(mp_p, "wb").write(mp)
    out = {}
    code, _, _, _, err = orc.build_file(fa_p, mp_p, str(tmp_path / "orc.ubt"), W=W, I=I, complevel=0, gg=gg)
    assert code == 0, err
    out["oracle"] = open(str(tmp_path / "orc.ubt"), "rb").read()
    name = M.reference_binary(W, I, gg)
    exe = os.path.join(REF, name) if name else None
    if exe and os.path.exists(exe):
        p = subprocess.run([exe, fa_p, mp_p, str(tmp_path / "ref.ubt"), "1", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stdout[-300:]
        out[name] = open(str(tmp_path / "ref.ubt"), "rb").read()
    return out


CASES = [(W, I, n) for W, I in ((8, 2),) for n in M.fold_cases()] + \
        [(W, I, n) for W, I in ((4, 2), (16, 2), (8, 4), (16, 4)) for n in ("two_way_cut", "genus_to_family", "order_021", "plain_build")]


@pytest.mark.parametrize("W,I,name", CASES)
def test_the_definition_is_the_builders(W, I, name, tmp_path):
    inputs, gg = M.fold_cases(W, I)[name]
    want, _ = M.merge(inputs, gg, I)
    for who, got in genuine(tmp_path, inputs, gg, I).items():
        assert got == want, "merge_ref differs from %s on the imagined FASTA" % who


def test_the_rules_consequences():
    """what the reference's rule does, spelled out: these are the contract, not accidents"""
    W, I = 8, 2
    one = lambda lab: M.Db(W, I, [(7, lab)])
    text = lambda ins, gg=True: M.fold(ins, gg)[0][7]
    assert text([one(M.PFX), one(M.PFX_LONG)]) == b"k__A;p__B" == text([one(M.PFX_LONG), one(M.PFX)])
    a, b, c = (one(s) for s in M.SIBLINGS)
    assert text([a, b]) == M.G and text([a, b, c]) == M.G[:M.G.rindex(b";")]            # the third sibling lifts genus to family
    L = M._labels()
    assert text([one(L["LA"]), one(L["LB"]), one(L["LX"])]) == b"k__A;p__B" and text([one(L["LA"]), one(L["LX"]), one(L["LB"])]) is M.BAD
    assert text([one(L["LA"]), one(L["LD"]), one(L["LA"])]) is M.BAD                      # BAD is absorbing
    assert text([one(L["LA"]), one(L["LB"])], gg=False) is M.BAD and text([one(L["LA"]), one(L["LA"])], gg=False) == L["LA"]


# ---- 3. the layout sniffing (host only) ---------------------------------------------------------------------------------------------------
def small_db(W=8, I=2, n=50, key=9):
    r = M.rng(W, I, n, key)
    return M.Db(W, I, [(w, b"k__S;p__L%d" % (j % 3)) for j, w in enumerate(M.random_words(r, W, n))])


def as_ctr(db: M.Db, path: str, **kw):
    labs = M.parse_labels(M.db_file(db)[32 + len(db.nodes) * (db.W + db.I):])
    ix = np.array([labs.index(l) for _, l in db.nodes], dtype=np.uint32)
    hi = np.array([w >> 64 for w, _ in db.nodes], dtype=np.uint64)
    lo = np.array([w & 0xFFFFFFFFFFFFFFFF for w, _ in db.nodes], dtype=np.uint64)
    ctrfile.write_ctr(path, db.W, db.I, hi, lo, ix, [l.decode("latin-1") for l in labs], **kw)


def probe_code(path):
    try:
        return lib.OK, search.merge_probe(path)
    except lib.UtreeError as e:
        return e.code, e.detail


@pytest.mark.parametrize("W,I", [(4, 2), (8, 2), (8, 4), (16, 2), (16, 4)])
def test_probe_tells_the_layouts_apart(W, I, tmp_path):
    db = small_db(W, I)
    u, c = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")                                # the names say nothing
    open(u, "wb").write(M.db_file(db, extra_labels=[b"k__Unused"]))
    as_ctr(db, c)
    for path, is_ctr, n_labels in ((u, 0, 4), (c, 1, 3)):
        code, info = probe_code(path)
        assert code == lib.OK and (info.W, info.I, info.is_ctr, info.n_nodes, info.n_labels) == (W, I, is_ctr, 50, n_labels)


def test_probe_refuses_what_is_neither(tmp_path):
    good = M.db_file(small_db())
    p = str(tmp_path / "x.ubt")

    def code_of(data):
        open(p, "wb").write(data)
        return probe_code(p)[0]
    assert code_of(good) == lib.OK
    assert code_of(good[:-1]) == lib.E_FORMAT                                               # the last line is not complete
    assert code_of(good[:good[:-1].rindex(b"\n") + 1]) == lib.E_FORMAT                      # a line is missing: the counts do not sum to N
    assert code_of(good + b"no tab here\n") == lib.E_FORMAT
    assert code_of(good + b"k__X\t12x\n") == lib.E_FORMAT
    assert code_of(good + b"k__X\t1\n") == lib.E_FORMAT                                     # one node too many counted
    assert code_of(good + b"k__X\t0\n") == lib.OK
    assert code_of(good[:20]) == lib.E_FORMAT
    assert code_of(np.array([8, 0, 2, 10 ** 12], dtype="<u8").tobytes() + good[32:]) == lib.E_FORMAT
    assert code_of(np.array([8, 1, 2, 50], dtype="<u8").tobytes() + good[32:]) == lib.E_FORMAT
    assert code_of(np.array([8, 0, 3, 50], dtype="<u8").tobytes() + good[32:]) == lib.E_FORMAT
    assert code_of(np.array([12, 0, 2, 50], dtype="<u8").tobytes() + good[32:]) == lib.E_UNSUPPORTED
    assert code_of(np.array([8, 0, 2, 0], dtype="<u8").tobytes()) == lib.OK                 # no node, no label: a `.ubt`
    assert probe_code(str(tmp_path / "missing"))[0] == lib.E_IO
    assert probe_code(str(tmp_path))[0] == lib.E_IO                                         # a directory


def test_probe_refuses_a_bin_table_that_is_not_monotone(tmp_path):
    db = small_db()
    p = str(tmp_path / "t.ctr")
    pref = ctrfile.word_prefix(8, np.zeros(50, dtype=np.uint64), np.array([w for w, _ in db.nodes], dtype=np.uint64))
    b = ctrfile.binix_exact(pref, 50)
    as_ctr(db, p, binix=b)
    assert probe_code(p)[0] == lib.OK
    nz = np.flatnonzero(np.diff(b.astype(np.int64)) > 0)
    b2 = b.copy()
    b2[nz[10] + 1] = b2[nz[10]]                                                             # a bin start pulled back below its predecessor's end
    b2[nz[10]] += np.uint64(1)
    as_ctr(db, p, binix=b2)
    code, why = probe_code(p)
    assert code == lib.E_UNSUPPORTED and "cannot be reconstructed" in why
