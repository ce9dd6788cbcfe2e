"""The merge and the compare at the two constants that no small input reaches (merge_kernels.hip): a slice of more than 256 MiB, which
decode_sort stages in two chunks with a record across their boundary, and a pass of more than 16 Mi nodes, which utk_merge_emit writes in
two chunks.  No test hook shortens a buffer here.  The inputs are numpy arrays written straight to files, the yardstick is
tests/merge_scale_ref.py (pinned to merge_ref.py and to the builder by test_merge_scale_cpu.py), and every comparison is byte for byte.
Each test prints how long its parts took."""
import os
import time

import numpy as np
import pytest

import compare_ref as CR
import merge_scale_ref as S
from utree_amd import search

pytestmark = pytest.mark.gpu
HOOKS = ("UTREE_TEST_MERGE_PASS_NODES", "UTREE_TEST_MERGE_STAGE_BYTES", "UTREE_TEST_MERGE_OUT_NODES")


class Clock:
    def __init__(self, name):
        self.name, self.t, self.parts = name, time.perf_counter(), []

    def lap(self, what):
        now = time.perf_counter()
        self.parts.append("%s %.2f s" % (what, now - self.t))
        self.t = now

    def show(self):
        print("\n[%s] %s" % (self.name, ", ".join(self.parts)), flush=True)


def same_file(path, head, rec, tail):
    """the file at `path` is head + rec + tail, compared without a Python object per node"""
    assert os.path.getsize(path) == len(head) + rec.nbytes + len(tail)
    with open(path, "rb") as f:
        assert f.read(len(head)) == head
        got = np.fromfile(f, dtype=rec.dtype, count=len(rec))
        assert np.array_equal(got.view(np.uint8), rec.view(np.uint8))
        assert f.read() == tail


def test_a_slice_of_two_staging_chunks(tmp_path, monkeypatch):
    """W = 16, I = 4: A's 13 600 000 records are 272 000 000 bytes, 2^28 = 20 x 13 421 772 + 16, so A's record 13 421 772 lies 16 bytes in
    the first staging chunk and 4 in the second.  B shares 65 536 of A's words: that record, the two at either side of it, A's first and
    last, the rest at random."""
    for v in HOOKS:
        monkeypatch.delenv(v, raising=False)
    ck = Clock("staging at 256 MiB")
    a, b, sh, keeps = S.staging_inputs()
    assert len(a.lo) * 20 > (1 << 28) and (1 << 28) // 20 == 13_421_772 and (1 << 28) % 20 == 16
    assert {0, len(a.lo) - 1, 13_421_770, 13_421_771, 13_421_772, 13_421_773, 13_421_774} <= set(sh.tolist())
    pa, pb, out = str(tmp_path / "a.ubt"), str(tmp_path / "b.ubt"), str(tmp_path / "out.ubt")
    S.write_ubt(pa, a)
    S.write_ubt(pb, b)
    ck.lap("generate")
    st = search.merge([pa, pb], out)
    ck.lap("merge")
    head, rec, tail, ws = S.merge_parts([a, b])
    ck.lap("reference")
    same_file(out, head, rec, tail)
    os.unlink(out)
    assert {k: getattr(st, k) for k in ws} == ws
    assert st.n_passes == 1 and st.n_shared == 65_536 and st.n_relabelled == 65_536 - keeps.sum() and st.n_nodes == 13_600_000 + 200_000 - 65_536
    del rec
    ck.lap("compare bytes")

    # ---- the compare of the same two files.  A word is in both exactly when it is one of the `sh`; there B's label is `lb`, A's `la`:
    # equal texts (the `keeps`) count as `same` under that text, others as `left` under A's text, `arrived` under B's and one move
    # (A's text, B's text); what a text has beyond that in A is only_a, in B only_b.  B's texts: the 20 of the tag "b", then A's 20.
    rep, mov = str(tmp_path / "report.tsv"), str(tmp_path / "moves.tsv")
    cs = search.compare(pa, pb, rep, mov)
    ck.lap("compare call")
    n = len(a.texts)
    assert b.texts[n:] == a.texts and not set(b.texts[:n]) & set(a.texts)
    la, lb = a.lab[sh], b.lab[np.searchsorted(b.hi, a.hi[sh])]
    assert np.array_equal(lb[keeps], la[keeps] + n) and (lb[~keeps] < n).all()
    count = lambda x: np.bincount(x, minlength=n)[:n]
    in_a, in_b_b, in_b_a = count(a.lab), count(b.lab[b.lab < n]), count(b.lab[b.lab >= n] - n)
    same, left, arrived = count(la[keeps]), count(la[~keeps]), count(lb[~keeps])
    want = {}
    for k in range(n):                                            # a, b, same, only_a, only_b, left, arrived
        want[a.texts[k]] = [in_a[k], in_b_a[k], same[k], in_a[k] - same[k] - left[k], in_b_a[k] - same[k], left[k], 0]
        want[b.texts[k]] = [0, in_b_b[k], 0, 0, in_b_b[k] - arrived[k], 0, arrived[k]]
    rows = [l.split(b"\t") for l in open(rep, "rb").read().split(b"\n")[:-1] if not l.startswith(b"#")]
    got = {r[0]: [int(v) for v in r[1:8]] for r in rows}
    assert {t: got[t] for t in want} == {t: [int(v) for v in f] for t, f in want.items()}
    assert all(not any(f) for t, f in got.items() if t not in want), "a row of no label text is a pure prefix"
    pairs, times = np.unique(la[~keeps] * n + lb[~keeps], return_counts=True)
    want_moves = {(a.texts[p // n], b.texts[p % n]): c for p, c in zip(pairs.tolist(), times.tolist())}
    lines = [l.split(b"\t") for l in open(mov, "rb").read().split(b"\n")[1:-1]]
    assert {(l[0], l[1]): int(l[2]) for l in lines} == want_moves and len(lines) == len(want_moves) == cs.n_moves
    assert all(l[3].decode() == CR.kind(l[0], l[1]) for l in lines)
    assert (cs.a, cs.b, cs.both, cs.same, cs.left, cs.arrived) == (13_600_000, 200_000, 65_536, keeps.sum(), 65_536 - keeps.sum(), 65_536 - keeps.sum())
    assert (cs.only_a, cs.only_b, cs.identical, cs.n_passes) == (13_600_000 - 65_536, 200_000 - 65_536, 0, 1)
    ck.lap("compare figures")
    ck.show()


@pytest.fixture(scope="module")
def output_case(tmp_path_factory):
    """the inputs' files and the reference, made once for the three runs"""
    ck = Clock("output at 16 Mi nodes")
    d = tmp_path_factory.mktemp("scale_out")
    a, b, four = S.output_inputs()
    pa, pb = str(d / "a.ubt"), str(d / "b.ubt")
    S.write_ubt(pa, a)
    S.write_ubt(pb, b)
    ck.lap("generate")
    head, rec, tail, ws = S.merge_parts([a, b])
    ck.lap("reference")
    ck.show()
    # the words the output holds at nodes 2^24 - 2 ... 2^24 + 1, the last two of the first chunk and the first two of the second, are folded ones
    at = slice((1 << 24) - 2, (1 << 24) + 2)
    assert rec["lo"][at].tolist() == four.tolist() and np.isin(four, a.lo).all() and np.isin(four, b.lo).all()
    out_texts = [l.split(b"\t")[0] for l in tail.split(b"\n")[:-1]]
    assert all(out_texts[i] not in a.texts + b.texts for i in rec["ix"][at].tolist()), "their label is a genus or the family: a cut"
    assert ws["n_nodes"] > (1 << 24) + 2 and ws["n_dropped"] == 5_000 and ws["n_relabelled"] == 50_000
    yield pa, pb, str(d / "out.ubt"), head, rec, tail, ws
    for p in (pa, pb):
        os.unlink(p)


@pytest.mark.parametrize("pass_nodes,n_passes", [(None, 1), (12_000_000, 2), (16_900_000, 2)])
def test_a_pass_of_two_output_chunks(pass_nodes, n_passes, output_case, monkeypatch):
    """W = 4, I = 2: 17 000 000 + 100 000 nodes, 5 000 of them dropped as BAD.  Unhooked: one pass, two output chunks of one emit.  Passes of
    12 000 000: two passes, two sweeps, each pass one chunk.  Passes of 16 900 000: a pass of two chunks, then a small one."""
    for v in HOOKS:
        monkeypatch.delenv(v, raising=False)
    if pass_nodes:
        monkeypatch.setenv("UTREE_TEST_MERGE_PASS_NODES", str(pass_nodes))
    pa, pb, out, head, rec, tail, ws = output_case
    ck = Clock("output at 16 Mi nodes, passes of %s" % pass_nodes)
    st = search.merge([pa, pb], out)
    ck.lap("merge")
    same_file(out, head, rec, tail)
    os.unlink(out)
    assert {k: getattr(st, k) for k in ws} == ws
    assert st.n_passes == n_passes
    ck.lap("compare bytes")
    ck.show()
