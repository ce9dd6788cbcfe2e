"""tests/merge_scale_ref.py -- the merge on numpy arrays that test_gpu_merge_scale.py holds the device to at production sizes -- pinned to
tests/merge_ref.py, the definition in plain Python, byte for byte and figure for figure; and, on one input, to the oracle's builder, as
merge_ref itself is (test_merge_cpu.py).  No GPU."""
import numpy as np
import pytest

import build_inputs as B
import merge_ref as M
import merge_scale_ref as S
from oracle import orc

Db = M.Db
LABS = [s for s in M.SIBLINGS] + [getattr(B, n).encode() for n in ("LA", "LB", "LX", "LC", "LD", "LE", "LF")]


def to_db(a: S.ADb) -> Db:
    hi = a.hi.tolist() if a.W == 16 else [0] * len(a.lo)
    return Db(a.W, a.I, [((h << 64) | l, a.texts[t]) for h, l, t in zip(hi, a.lo.tolist(), a.lab.tolist())])


def same_as_merge_ref(inputs, gg=True, I=0):
    """inputs: merge_ref.Db.  Returns merge_ref's (bytes, stats)."""
    want, ws = M.merge(inputs, gg, I)
    got, gs = S.merge([S.from_db(db) for db in inputs], gg, I)
    assert got == want
    assert gs == ws
    return want, ws


@pytest.mark.parametrize("W,I", [(8, 2), (4, 2), (16, 4)])
@pytest.mark.parametrize("name", sorted(M.fold_cases()))
def test_fold_cases(name, W, I):
    inputs, gg = M.fold_cases(W, I)[name]
    same_as_merge_ref(inputs, gg)
    same_as_merge_ref(inputs, not gg)
    same_as_merge_ref(inputs[::-1], gg, I=4)


@pytest.mark.parametrize("seed", range(20))
def test_three_random_inputs(seed):
    """300 words, a third of them in more than one input"""
    r = M.rng(4000, seed)
    W, I = [(8, 2), (4, 2), (16, 4), (16, 2)][seed % 4]
    words = M.random_words(r, W, 300)
    ins = [[], [], []]
    for j, w in enumerate(words):
        holders = r.permutation(3)[:int(r.integers(2, 4))] if j % 3 == 0 else [int(r.integers(0, 3))]
        for i in holders:
            ins[int(i)].append((w, LABS[int(r.integers(0, len(LABS)))]))
    _, ws = same_as_merge_ref([Db(W, I, sorted(n)) for n in ins], gg=seed % 5 != 4)
    assert ws["n_shared"] == 100


def test_k64_words_equal_in_one_half():
    """words equal in the high half and different in the low, and the reverse, in three inputs: the sort by the high half alone does not do"""
    r = M.rng(5)
    H = [int.from_bytes(r.bytes(8), "little") for _ in range(8)]
    Lo = [int.from_bytes(r.bytes(8), "little") for _ in range(8)]
    words = sorted((h << 64) | l for h in H for l in Lo)
    ins = [Db(16, 2, [(w, LABS[3 + i]) for w in words[i::2] + words[1 - i:8:2]]) for i in range(2)] + [Db(16, 2, [(w, LABS[5]) for w in words])]
    ins = [Db(16, 2, sorted(set(db.nodes))) for db in ins]
    _, ws = same_as_merge_ref(ins)
    assert ws["n_shared"] == 64 and ws["n_relabelled"] > 0
    same_as_merge_ref(ins[::-1])


def test_an_input_of_no_nodes_and_no_inputs_nodes():
    a = Db(8, 2, [(5, LABS[0]), (9, LABS[1])])
    same_as_merge_ref([Db(8, 2, []), a, Db(8, 4, [])])
    same_as_merge_ref([Db(8, 2, [])])


def test_label_lines_no_node_carries_get_no_index():
    a = S.ADb(8, 2, None, np.array([3, 7], dtype=np.uint64), np.array([2, 0]), [b"k__A;p__B", b"k__Never;p__Seen", b"k__A;p__C"])
    got, st = S.merge([a])
    assert (got, st) == M.merge([to_db(a)]) and st["n_labels"] == 2


def scaled_staging():
    return S.staging_inputs(n_a=13_600, n_b=200, n_shared=66, straddle=13_421, n_labels=20)


def scaled_output():
    return S.output_inputs(n_a=17_000, n_b=100, n_sib=50, n_bad=5, around=16_777, n_labels=20)


def test_staging_generator_at_a_thousandth():
    a, b, sh, keeps = scaled_staging()
    assert (a.W, a.I, len(a.lo), len(b.lo), len(sh)) == (16, 4, 13_600, 200, 66)
    assert {0, 13_599, 13_419, 13_420, 13_421, 13_422, 13_423} <= set(sh.tolist())
    da, db = to_db(a), to_db(b)
    assert [w for w, _ in da.nodes] == sorted(set(w for w, _ in da.nodes)) and [w for w, _ in db.nodes] == sorted(set(w for w, _ in db.nodes))
    held = dict(da.nodes)
    assert sorted(w for w, _ in db.nodes if w in held) == [da.nodes[i][0] for i in sh.tolist()]
    assert [held[da.nodes[i][0]] == dict(db.nodes)[da.nodes[i][0]] for i in sh.tolist()] == keeps.tolist() and 0 < keeps.sum() < 66
    _, ws = same_as_merge_ref([da, db])
    assert ws["n_shared"] == 66 and ws["n_relabelled"] == 66 - keeps.sum() and ws["n_dropped"] == 0
    same_as_merge_ref([db, da])


def test_output_generator_at_a_thousandth():
    a, b, four = scaled_output()
    assert (a.W, a.I, len(a.lo), len(b.lo)) == (4, 2, 17_000, 100) and int(a.lo[-1]) < 1 << 32
    da, db = to_db(a), to_db(b)
    assert [w for w, _ in db.nodes] == sorted(set(w for w, _ in db.nodes))
    want, ws = same_as_merge_ref([da, db])
    assert (ws["n_shared"], ws["n_relabelled"], ws["n_dropped"], ws["n_nodes"]) == (55, 50, 5, 17_000 + 45 - 5)
    rec = np.frombuffer(want[32:32 + 6 * ws["n_nodes"]], dtype=S.records(4, 2, None, a.lo[:0], a.lab[:0]).dtype)
    assert rec["lo"][16_775:16_779].tolist() == four.tolist(), "the named words stand around node `around` of the output"
    assert set(four.tolist()) <= set(a.lo.tolist()) & set(b.lo.tolist())
    same_as_merge_ref([da, db], gg=False)


@pytest.mark.parametrize("which", ["staging", "output"])
def test_against_the_builder(which, tmp_path):
    """the oracle's restatement of the genuine builder on the imagined FASTA of a scaled copy, as test_merge_cpu.py holds merge_ref to it"""
    a, b = (scaled_staging() if which == "staging" else scaled_output())[:2]
    ins = [to_db(a), to_db(b)]
    got, _ = S.merge([a, b])
    fa, mp = M.imagined(ins)
    fa_p, mp_p, out = str(tmp_path / "im.fa"), str(tmp_path / "im.map"), str(tmp_path / "orc.ubt")
    open(fa_p, "wb").write(fa)
    open(mp_p, "wb").write(mp)
    code, _, _, _, err = orc.build_file(fa_p, mp_p, out, W=a.W, I=a.I, complevel=0, gg=True)
    assert code == 0, err
    assert got == open(out, "rb").read()
