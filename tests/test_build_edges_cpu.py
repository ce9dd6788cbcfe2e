"""The inputs of tests/test_gpu_build_edges.py, checked without a GPU:
(a) each generated case has the property it was built for (exact total_pos, which lanes are valid, every hostile byte present, an order of
    references that matters);
(b) on the one-label cases the oracle's `.ubt` and log equal the numpy model's (build_inputs.model), byte for byte;
(c) the oracle equals what the genuine builders wrote on the same bytes (golden/reference_runs.json: exit code, SHA-256 of `.ubt` and log,
    recorded by `make_golden.py reference_runs build_edges` from oracle/_ref).
"""
import os

import numpy as np
import pytest

from oracle import orc
import build_inputs as B
import util

RUNS = B.runs()
BY_KEY = {r.key: r for r in RUNS}


def oracle_build(case, W, lv, gg, d, I=2):
    """Returns (exit code, n_nodes, n_labels, .ubt bytes or None, log bytes or None)."""
    fa, mp, ubt = os.path.join(d, "i.fa"), os.path.join(d, "i.map"), os.path.join(d, "o.ubt")
    log = ubt + (".gg.log" if gg else ".log")
    for f in (ubt, log):
        if os.path.exists(f):
            os.remove(f)
    open(fa, "wb").write(case.fa)
    open(mp, "wb").write(case.map)
    code, ns, nn, nl, err = orc.build_file(fa, mp, ubt, W=W, I=I, complevel=lv, gg=bool(gg))
    rd = lambda p: open(p, "rb").read() if os.path.exists(p) else None
    return code, nn, nl, rd(ubt), rd(log)


def log_labels(log: bytes):
    return [tuple(l.split("\t")) for l in log.decode().splitlines()]


# ---------------------------------------------------------------- (a) planted properties ----------------------------------------------------------------
@pytest.mark.parametrize("W", B.WS)
def test_bytes_case_plants_every_byte(W):
    for lv in range(5):
        c = B.bytes_case(W, lv)
        refs = B.frame(c.fa)
        assert len(refs) == 3 and c.fa.count(b"\r\n") == 2 and not c.fa.endswith(b"\n")
        body = b"".join(s for _, s in refs)
        assert b"\0" not in body and max(body) < 0x80 and b"\n" not in body
        cnt = np.bincount(np.frombuffer(body, dtype=np.uint8), minlength=128)
        assert all(cnt[b] >= 1 + lv for b in B.HOSTILE)                      # once in a k-mer, once per filter slot
        m = B.model(c.fa, W, lv)
        K = 4 * W
        assert 8 + 2 * lv <= m.n_kmers < m.total_pos                        # the planted windows survive where the byte is one of ACGTacgt, and only there
        # mixed case inside one dword of a VALID k-mer: among the valid windows, upper- and lowercase stand side by side
        seq = np.frombuffer(refs[0][1], dtype=np.uint8)
        p = int(np.flatnonzero(m.valid[0])[0]) + lv
        low = (seq[p:p + K] & 0x20) != 0
        assert low.any() and not low.all()


@pytest.mark.parametrize("W", B.WS)
def test_shape_case_total_pos_and_layout(W):
    kv = 4 * W - 1
    for t in B.SHAPE_TARGETS:
        for many in (False, True):
            c = B.shape_case(W, t, many=many)
            lens = [len(s) for _, s in B.frame(c.fa)]
            assert lens == c.planted["lens"]
            m = B.model(c.fa, W, 0)
            assert m.total_pos == t == m.n_kmers == sum(max(0, L - kv) for L in lens)
            assert lens[:3] == [1, kv - 1, kv] and lens[-3:] == [kv, kv - 1, 1]        # no position: first, last, three in a row
            one = [i for i, L in enumerate(lens) if L == kv + 1]
            assert len(one) == min(t, 3) and all(lens[i - 1] <= kv and lens[i + 1] <= kv for i in one)
    m = B.model(B.shape_case(W, 257, lv=3).fa, W, 3)
    assert m.total_pos == 257 and 0 < m.n_kmers < 30                                  # the filter leaves about 1 in 64


@pytest.mark.parametrize("W", B.WS)
def test_sparse_case_valid_lanes(W):
    c = B.sparse_case(W)
    m = B.model(c.fa, W, 0)
    assert m.total_pos == B.SPARSE_TOTAL and [len(v) for v in m.valid] == [0, 0, B.SPARSE_TOTAL, 0]
    g = np.flatnonzero(m.valid[2])
    assert tuple(g) == B.SPARSE_VALID
    assert sorted(g // 256) == [0, 1, 2, 3]                                           # one per block
    assert g[0] % 64 == 63 and g[1] % 256 == 0 and g[2] % 64 == 63 and g[3] == m.total_pos - 1


@pytest.mark.parametrize("W", B.WS)
def test_extremes_case_buckets_and_runs(W):
    c = B.extremes_case(W, 1)
    m = B.model(c.fa, W, 0)
    assert min(m.hist[0], m.hist[4095]) >= c.planted["occ"] > 256                     # one word each, a run longer than a block of fold_k
    all_t = (1 << (8 * W)) - 1
    words = [(int(h) << 64) | int(l) for h, l in zip(m.hi, m.lo)]
    assert words[0] == 0 and words[-1] == all_t
    assert B.pass_ranges(m.hist, int(m.hist.max()) - 1) is None                       # one bucket over the limit: refused
    r = B.pass_ranges(m.hist, int(m.hist.max()))
    assert B.pass_of(r, 0) != B.pass_of(r, 4095) and len(r) >= 3


@pytest.mark.parametrize("W", B.WS)
def test_clock_case_plants_the_three_situations(W, tmp_path):
    c = B.clock_case(W)
    code, nn, nl, ubt, log = oracle_build(c, W, 0, 1, str(tmp_path))
    assert code == 0
    labs = log_labels(log)
    assert [l for l, _ in labs] == c.planted["labels"]                               # C3 (cut early in c2) before C2 (cut later in c2)
    assert dict(labs)[c.planted["empty_label"]] == "0"                               # its only k-mer went BAD afterwards
    assert int(dict(labs)[B.C3]) >= 2 and int(dict(labs)[B.C2]) >= 2                 # X and c3's own word; Y and c7's
    m = B.model(c.fa, W, 0)
    bx, by, bz = (int(B.bucket_of(W, *B.positions(c.planted["words"][k], W, 0)[1:])[0]) for k in "XYZ")
    assert by == 1 and bx == 0xFFE and by < bz < bx and m.hist[4095] == 0
    r = B.pass_ranges(m.hist, int(m.hist.max()))
    assert len({B.pass_of(r, b) for b in (bx, by, bz)}) == 3                         # three different passes, X's after Y's
    # A pass always starts at a bucket that has k-mers and takes the empty buckets behind it along, so no pass is without a k-mer
    # unless the whole input is (the no-k-mer inputs); what the ranges do have is long stretches of empty buckets inside them.
    assert all(n > 0 for _, _, n in r) and max(e - b for b, e, _ in r) > 1000


def test_stability_case_ties():
    c = B.stability_case()
    M = c.planted["words"]
    assert len(set(M)) == 64 == c.planted["places"] >= 20
    assert len({w[:32] for w in M}) == 8 and len({w[32:] for w in M}) == 8          # ties in either half
    m = B.model(c.fa, 16, 0)
    assert 200 < m.n_kmers < 1000 and m.hist[4095] == 0                              # a few hundred k-mers
    r = B.pass_ranges(m.hist, int(m.hist.max()))
    assert len(r) >= 4 and all(n > 0 for _, _, n in r)


CASES_WHERE_ORDER_MATTERS = [("extremes3", W) for W in B.WS] + [("clock", W) for W in B.WS] + [("stability", 16)]


@pytest.mark.parametrize("name,W", CASES_WHERE_ORDER_MATTERS)
def test_order_of_references_matters(name, W, tmp_path):
    """Reversing the references changes what the oracle writes: the case says something about order."""
    c = BY_KEY["build_edges_%s_W%d_c0_gg" % (name, W)].make()
    fwd = oracle_build(c, W, 0, 1, str(tmp_path))
    rev = oracle_build(B.reverse_refs(c), W, 0, 1, str(tmp_path))
    assert fwd[0] == rev[0] == 0
    assert fwd[3] != rev[3] and fwd[4] != rev[4]
    if name != "clock":                                                              # forward: the planted words survive at "k__A;p__B"
        labs = dict(log_labels(fwd[4]))
        want = 2 if name == "extremes3" else 64
        assert int(labs[c.planted["survivor"]]) == want
        assert dict(log_labels(rev[4])).get(c.planted["survivor"], "0") == "0"           # reversed: the cut comes first and the next label ends them BAD


@pytest.mark.parametrize("W", B.WS)
def test_no_kmer_inputs_have_none(W):
    for which, lv in B.NO_KMERS.items():
        c = B.no_kmers_case(W, which)
        m = B.model(c.fa, W, lv)
        assert m.n_kmers == 0 and (m.total_pos == 0) == (which == "short")
        if which == "no_ag":
            assert B.model(c.fa, W, 0).n_kmers > 100 and B.model(c.fa, W, 1).n_kmers > 10     # it is the filter that leaves none


# ---------------------------------------------------------------- (b) oracle == model ----------------------------------------------------------------
@pytest.mark.parametrize("key", [r.key for r in RUNS if r.one_label])
def test_oracle_equals_model_on_one_label_cases(key, tmp_path):
    r = BY_KEY[key]
    c = r.make()
    m = B.model(c.fa, r.W, r.lv)
    for I in (2, 4):
        code, nn, nl, ubt, log = oracle_build(c, r.W, r.lv, r.gg, str(tmp_path), I=I)
        if m.n_kmers == 0:
            assert code == 2 and ubt is None and log is None
            continue
        assert code == 0 and (nn, nl) == (m.n_distinct, 1)
        assert ubt == B.ubt_bytes(m, r.W, I) and log == B.label_lines(B.ONE, m.n_distinct)


# ---------------------------------------------------------------- (c) oracle == genuine reference ----------------------------------------------------------------
@pytest.mark.parametrize("key", [r.key for r in RUNS])
def test_oracle_equals_reference(key, tmp_path):
    r = BY_KEY[key]
    c = r.make()
    want = util.reference_run(key, fa=c.fa, map=c.map)
    code, nn, nl, ubt, log = oracle_build(c, r.W, r.lv, r.gg, str(tmp_path))
    assert code == want["exit"]
    assert (util.sha256_of(ubt) if ubt is not None else None) == want["outputs"]["ubt"]
    assert (util.sha256_of(log) if log is not None else None) == want["outputs"]["log"]
    so = want["stdout"]
    if code == 0:
        assert "Total nodes in tree: %d [%d labels]" % (nn, nl) in so
        if r.one_label:                                                              # the model's count of distinct k-mers is the reference's line
            assert "Done with sequence parse: %d k-mers made" % B.model(c.fa, r.W, r.lv).n_distinct in so
    else:
        assert so[-2:] == ["Done with sequence parse: 0 k-mers made", "Error: no k-mers. Bad input/params!"]
