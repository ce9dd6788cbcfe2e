"""CPU-only tests of the tile contract (include/utree_amd.h, utree_tiles_*): the Python restatement against the genuine reference's bytes,
the closed-form tile count, the two host formatters against the restatement, the argument checks of utree_tiles_file in front of the
handles, and header against binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tiles_ref
import util
from oracle import orc
from utree_amd import lib
from utree_amd.search import RESULT_DTYPE, CtrDB, frame_fasta, tiles_format, tiles_segments_format

_REF = {}


def ref(name, rc):
    """the restatement's tiles of the committed contigs, computed once"""
    if (name, rc) not in _REF:
        recs = tiles_ref.parse(tiles_ref.contigs(name))
        W, S = tiles_ref.PARAMS[name]
        o = orc.OracleDB.load(util.fixture_ctr(name))
        _REF[(name, rc)] = (recs, tiles_ref.classify(o, recs, W, S, rc))
    return _REF[(name, rc)]


@pytest.mark.parametrize("name", tiles_ref.FIXTURES)
def test_the_committed_contigs_are_the_generated_ones(name):
    m = tiles_ref.manifest()["fixtures"][name]
    data = tiles_ref.contigs(name)
    assert tiles_ref.sha256(data) == m["contigs_sha256"] and data == tiles_ref.fasta(tiles_ref.make_contigs(name))
    recs = tiles_ref.parse(data)
    W, S = tiles_ref.PARAMS[name]
    assert (W, S) == (m["W"], m["S"]) and [len(s) for _, s in recs] == tiles_ref.query_lengths(name)
    assert tiles_ref.sha256(tiles_ref.fasta(tiles_ref.split_records(recs, W, S))) == m["split_sha256"]


@pytest.mark.parametrize("rc", (False, True))
@pytest.mark.parametrize("name", tiles_ref.FIXTURES)
def test_the_restatement_equals_the_reference(name, rc):
    """tiles_ref over the CPU oracle, tile by tile == what the genuine xtree-searchGG wrote for the pre-split FASTA"""
    recs, tl = ref(name, rc)
    gold = tiles_ref.golden(name, rc)
    m = tiles_ref.manifest()["fixtures"][name]
    tag = "_rc" if rc else ""
    assert tiles_ref.sha256(gold) == m["out%s_sha256" % tag]
    assert tiles_ref.tiles_tsv(tl) == gold
    assert len(tl) == m["tiles"] == m["searched%s" % tag] and gold.count(b"\n") == m["good_finds%s" % tag]
    seg = tiles_ref.segments_tsv(recs, tl)
    assert seg.count(b"\n") == m["segments%s" % tag]
    rows = [l.split(b"\t") for l in seg.split(b"\n")[:-1]]
    assert sum(int(r[3]) for r in rows) == len(tl) and {r[0] for r in rows} == {n for n, _ in recs}       # every tile once, every query a line
    assert sum(int(r[6]) for r in rows) == sum(int(x.res.found) for x in tl)


def test_the_closed_form_equals_the_enumeration():
    for W in range(1, 41):
        for S in range(1, W + 1):
            for L in range(1, 41):
                t = tiles_ref.tiles(L, W, S)
                assert len(t) == tiles_ref.n_tiles(L, W, S), (L, W, S)
                assert t[-1][1] == L and all(b - a == W for a, b in t[:-1])
                assert len(t) == 1 or W - S < t[-1][1] - t[-1][0] <= W, (L, W, S)                              # only the last is shorter, and not by S


# ---- the host formatters -------------------------------------------------------------------------------------------------------------

def framed(recs):
    data = tiles_ref.fasta(recs)
    fr = frame_fasta(data)
    return np.frombuffer(data, dtype=np.uint8), fr


def both_files(db, recs, W, S, tl, res=None):
    buf, fr = framed(recs)
    res = tiles_ref.results_array(tl) if res is None else res
    tq, ti = np.array([x.q for x in tl], dtype=np.uint32), np.array([x.t for x in tl], dtype=np.uint32)
    args = (db, buf, fr["name_off"], fr["name_len"], fr["seq_len"], W, S, tq, ti, res)
    return tiles_format(*args), tiles_segments_format(*args), args


@pytest.mark.parametrize("rc", (False, True))
@pytest.mark.parametrize("name", tiles_ref.FIXTURES)
def test_formatters_on_fixture_results(name, rc):
    recs, tl = ref(name, rc)
    W, S = tiles_ref.PARAMS[name]
    db = CtrDB.open(util.fixture_ctr(name))
    (text, lines), (seg, nseg), args = both_files(db, recs, W, S, tl)
    assert text == tiles_ref.golden(name, rc) and lines == text.count(b"\n")
    want = tiles_ref.segments_tsv(recs, tl)
    assert seg == want and nseg == want.count(b"\n")
    # the same segments from any cut of the tiles into calls: the open run is carried in the state, closed by the last call
    for step in (1, 7, len(tl)):
        st, got, n = lib.TilesRun(), b"", 0
        for a in range(0, len(tl), step):
            b = min(a + step, len(tl))
            piece = args[:7] + tuple(x[a:b] for x in args[7:])
            t, k = tiles_segments_format(*piece, flush=b == len(tl), state=st)
            got += t; n += k
        assert got == want and n == nseg and st.open == 0
    db.close()


def hand_made(db):
    """three queries whose tiles' results sit on the formatter's edges"""
    recs = [(b"first", b"A" * 95), (b"second_query", b"C" * 10), (b"q3", b"G" * 61)]
    W, S = 20, 15                                                  # 6, 1 and 4 tiles: the last of `first` is 20 long, of `q3` 16
    l0 = db.label(0)
    other = next(i for i in range(1, db.n_labels) if db.label(i)[:12] == l0[:12] and db.label(i) != l0)
    longer = next(i for i in range(1, db.n_labels) if len(db.label(i)) > 12)
    R = lambda label, cut, found, uix, sl=0, ol=0: (label, cut, found, uix, sl, ol)
    rows = [R(0, -2, 0, 0),                 # found == 0 at a query's first tile
            R(0, 12, 5, 2, 3, 2),           # two labels of equal TEXT side by side: one run
            R(other, 12, 4294967295, 3, 4294967295, 7),
            R(0, -2, 1, 1),                 # uix == 1: "*"; the whole label is another text than its first 12 bytes
            R(0, -1, 2, 2, 1, 1),           # the empty taxon: classified, a class of its own
            R(0, -2, 0, 0),                 # found == 0 at a query's last tile
            R(longer, 100000, 9, 4, 5, 4),  # a cut beyond the label prints the label; a query of one tile
            R(3, -2, 0, 5, 9, 9),           # unclassified whatever the other fields say ...
            R(7, -1, 0, 0),                 # ... and one run with the next unclassified tile
            R(0, -1, 3, 1),
            R(0, -1, 3, 1)]
    res = np.array(rows, dtype=RESULT_DTYPE)
    tl = []
    for q, (n, s) in enumerate(recs):
        for t, (a, b) in enumerate(tiles_ref.tiles(len(s), W, S)):
            x = tiles_ref.Tile()
            x.q, x.t, x.a, x.b = q, t, a, b
            r = res[len(tl)]
            x.res = orc.Result(*[int(v) for v in r])
            lab = db.label(int(r["label"]))
            tax = b"" if r["cut"] == -1 else lab if r["cut"] == -2 else lab[:int(r["cut"])]
            tail = b"1\t*" if r["uix"] == 1 else b"%d\t%d;%d" % (r["uix"], r["sl"], r["ol"])
            x.line = b"%s\t%s\t%d\t%s\n" % (tiles_ref.tile_name(n, a, b), tax, r["found"], tail) if r["found"] else b""
            x.taxon = tax if r["found"] else None
            tl.append(x)
    assert len(tl) == len(rows)
    return recs, W, S, tl, res


def test_formatters_on_hand_made_results():
    db = CtrDB.open(util.fixture_ctr("vote"))
    recs, W, S, tl, res = hand_made(db)
    (text, lines), (seg, nseg), args = both_files(db, recs, W, S, tl, res)
    assert text == tiles_ref.tiles_tsv(tl) and lines == 7
    assert text.startswith(b"first:16-35\t" + db.label(0)[:12] + b"\t5\t2\t3;2\nfirst:31-50\t" + db.label(0)[:12] + b"\t4294967295\t3\t4294967295;7\nfirst:46-65\t")
    assert b"first:61-80\t\t2\t2\t1;1\n" in text and b"second_query:1-10\t" in text and text.endswith(b"q3:46-61\t\t3\t1\t*\n")
    want = tiles_ref.segments_tsv(recs, tl)
    assert seg == want and nseg == 8
    assert seg.split(b"\n")[:2] == [b"first\t1\t20\t1\tU\t\t0", b"first\t16\t50\t2\tC\t" + db.label(0)[:12] + b"\t4294967300"]
    assert b"first\t61\t80\t1\tC\t\t2\n" in seg and b"q3\t1\t35\t2\tU\t\t0\nq3\t31\t61\t2\tC\t\t6\n" in seg
    # cap too small: (size_t)-1 from either, at every cap below the exact size, and the state is left as it was
    L = lib.load()
    bad = C.c_size_t(-1).value
    a = [x.ctypes.data if isinstance(x, np.ndarray) else x for x in args[1:]]
    for cap in list(range(0, 64)) + [len(text) - 1, len(seg) - 1]:
        out = np.zeros(cap + 1, dtype=np.uint8)
        if cap < len(text):
            assert L.utree_tiles_format(db._h, *a, len(tl), out.ctypes.data, cap, None) == bad
        if cap < len(seg):
            st = lib.TilesRun(open=1, query=2, start=5, end=9, n_tiles=3, found=1)
            assert L.utree_tiles_segments_format(db._h, *a, len(tl), 1, C.byref(st), out.ctypes.data, cap, None) == bad
            assert (st.open, st.query, st.start, st.end, st.n_tiles, st.found) == (1, 2, 5, 9, 3, 1)
        assert out[cap] == 0
    out = np.zeros(len(text), dtype=np.uint8)
    assert L.utree_tiles_format(db._h, *a, len(tl), out.ctypes.data, len(text), None) == len(text) and out.tobytes() == text
    # a label that is none of the database's
    res2 = res.copy(); res2[3]["label"] = db.n_labels
    a2 = a[:-1] + [res2.ctypes.data]
    out = np.zeros(4096, dtype=np.uint8)
    assert L.utree_tiles_format(db._h, *a2, len(tl), out.ctypes.data, 4096, None) == bad
    assert L.utree_tiles_segments_format(db._h, *a2, len(tl), 1, C.byref(lib.TilesRun()), out.ctypes.data, 4096, None) == bad
    db.close()


# ---- utree_tiles_file: every check in front of the handles --------------------------------------------------------------------------------

CTR = C.create_string_buffer(1 << 16)
DEV = C.create_string_buffer(1 << 16)


def run(ctr=True, dev=True, reads=b"/nonexistent/contigs.fa", tiles=b"/nonexistent/tiles.tsv", segments=None, params=True, stats=True,
        size=None, stats_size=None, **fields):
    base = dict(tile_bp=1000, step_bp=500)
    base.update(fields)
    prm = lib.TilesParams(**base)
    st = lib.TilesStats()
    if size is not None:
        prm.size = size
    if stats_size is not None:
        st.size = stats_size
    return lib.load().utree_tiles_file(C.addressof(CTR) if ctr else None, C.addressof(DEV) if dev else None, reads, tiles, segments,
                                       C.byref(prm) if params else None, C.byref(st) if stats else None)


CASES = {
    "S 0": dict(step_bp=0),
    "S > W": dict(tile_bp=100, step_bp=101),
    "W 0": dict(tile_bp=0, step_bp=0),
    "W above the limit": dict(tile_bp=lib.TILE_MAX_BP + 1, step_bp=1),
    "size - 4": dict(size=C.sizeof(lib.TilesParams) - 4),
    "size + 8": dict(size=C.sizeof(lib.TilesParams) + 8),
    "size 0": dict(size=0),
    "stats size 0": dict(stats_size=0),
    "stats size + 8": dict(stats_size=C.sizeof(lib.TilesStats) + 8),
    "reads_path NULL": dict(reads=None),
    "tiles_path NULL": dict(tiles=None),
    "params NULL": dict(params=False),
    "stats NULL": dict(stats=False),
    "ctr NULL": dict(ctr=False),
    "dev NULL": dict(dev=False),
    "do_rc 2": dict(do_rc=2),
    "input_format -1": dict(input_format=-1),
    "input_format 4": dict(input_format=lib.INPUT_AUTO + 1),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_check_comes_before_the_handles(case):
    assert run(**CASES[case]) == lib.E_ARG


def test_the_limits_themselves_pass_the_checks():
    """W = S = the limit and W = S = 1 are parameters like any other: the call goes on to the reads file, which is not there"""
    assert run(tile_bp=lib.TILE_MAX_BP, step_bp=lib.TILE_MAX_BP) == lib.E_IO
    assert run(tile_bp=1, step_bp=1) == lib.E_IO
    assert not os.path.exists("/nonexistent/tiles.tsv")


def test_plan_and_views_check_their_arguments():
    L = lib.load()
    dev, p = C.addressof(DEV), C.addressof(CTR)
    assert L.utree_tiles_workspace_bytes(None, 10) == 0
    assert L.utree_tiles_plan(None, p, 1, 100, 50, p, p, p, 1 << 16, None) == lib.E_ARG
    assert L.utree_tiles_plan(dev, p, 1, 100, 0, p, p, p, 1 << 16, None) == lib.E_ARG
    assert L.utree_tiles_plan(dev, p, 1, 100, 101, p, p, p, 1 << 16, None) == lib.E_ARG
    assert L.utree_tiles_plan(dev, p, 1, lib.TILE_MAX_BP + 1, 1, p, p, p, 1 << 16, None) == lib.E_ARG
    assert L.utree_tiles_plan(dev, None, 1, 100, 50, p, p, p, 1 << 16, None) == lib.E_ARG
    assert L.utree_tiles_views(dev, p, p, 1, 100, 50, p, 0, lib.TILES_MAX_BATCH + 1, p, p, p, p, p, None) == lib.E_ARG
    assert L.utree_tiles_views(dev, p, p, 1, 100, 0, p, 0, 1, p, p, p, p, p, None) == lib.E_ARG
    assert L.utree_tiles_views(dev, p, p, 1, 100, 50, p, 0, 1, None, p, p, p, p, None) == lib.E_ARG
    assert L.utree_tiles_views(None, p, p, 1, 100, 50, p, 0, 1, p, p, p, p, p, None) == lib.E_ARG


# ---- header and binding ---------------------------------------------------------------------------------------------------------------

C_TYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double, "int": C.c_int,
           "utree_fasta_error": lib.FastaError}


def header_struct(name):
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, hdr)
    assert m, "include/utree_amd.h declares no %s" % name
    out = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            out += [(n.strip(), C_TYPES[ctype]) for n in names.split(",")]
    return out


@pytest.mark.parametrize("name,cls,size", [("utree_tiles_params", lib.TilesParams, 24), ("utree_tiles_stats", lib.TilesStats, 88),
                                           ("utree_tiles_meta", lib.TilesMeta, 24), ("utree_tiles_run", lib.TilesRun, 56)])
def test_binding_mirrors_the_header(name, cls, size):
    assert header_struct(name) == [(f[0], f[1]) for f in cls._fields_]
    assert C.sizeof(cls) == size
    if name in ("utree_tiles_params", "utree_tiles_stats"):
        assert cls._fields_[0][0] == "size" and cls().size == size


def test_the_abi_did_not_move():
    assert lib.load().utree_abi_version() == 4 and C.sizeof(lib.SearchRequest) == 128
    for s in ("utree_tiles_workspace_bytes", "utree_tiles_plan", "utree_tiles_views", "utree_tiles_format", "utree_tiles_segments_format", "utree_tiles_file"):
        assert s in lib.SYMBOLS and hasattr(lib.load(), s)
    hdr = open(os.path.join(util.ROOT, "include", "utree_amd.h")).read()
    assert int(re.search(r"#define UTREE_TILE_MAX_BP (\d+)u", hdr).group(1)) == lib.TILE_MAX_BP == tiles_ref.TILE_MAX_BP
    assert "#define UTREE_TILES_MAX_BATCH (1u << 21)" in hdr and lib.TILES_MAX_BATCH == 1 << 21
    assert os.path.exists(lib.TILES_CLI_PATH)
