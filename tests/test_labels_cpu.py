"""The CPU oracle at the label counts tests/test_gpu_labels.py holds the kernels to: databases of 65 534 .. 2^19 - 1 labels
(tests/label_inputs.py) searched by the genuine reference once (golden/reference_runs.json, `make_golden.py reference_runs labels`: only
hashes are committed), and the oracle's output on the rebuilt inputs compared with that.  Then the conditions that give the GPU tests their
meaning, from the oracle's own records: every label count in every batch, reads whose highest label is one of the four highest ranks,
counts above one, bitmap words in every thread's stretch of classify_long_k's sweep, a read that keeps 64 hits in the rank-specific search.
No GPU.
"""
import os

import numpy as np
import pytest

from oracle import orc
from utree_amd.search import frame_fasta
import hitmap_ref
import label_inputs as li
import util


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("labels_cpu")


def seqs_of(data):
    return data.split(b"\n")[1::2]


def check_forms(built, o, data, rc):
    """forms: every label count 0 .. 5 twenty times; twenty reads of two or three labels whose highest is one of the four highest ranks,
    twenty with a count above one; of the reads planned with 2, 3 and 4 labels a third each at the top and at the bottom of the ranks."""
    fr = frame_fasta(data)
    w = o.classify_batch(np.frombuffer(data, dtype=np.uint8), fr["seq_off"], fr["seq_len"], rc=rc, threads=4)
    assert len(w) == li.N_FORMS
    for u in range(6):
        assert int((w["uix"] == u).sum()) >= 20, (built.name, rc, u, np.bincount(w["uix"]))
    two3 = (w["uix"] >= 2) & (w["uix"] <= 3)
    top = np.zeros(len(w), bool)
    low = np.zeros(len(w), bool)
    for i, s in enumerate(seqs_of(data)):
        c = hitmap_ref.codes(o, s, rc)
        ranks = built.rank_of[c[c < built.n]]
        assert len(set(ranks.tolist())) == int(w["uix"][i]) and len(ranks) == int(w["found"][i])
        if len(ranks):
            top[i] = int(ranks.max()) >= built.n - 4
            low[i] = int(ranks.min()) <= 3
    assert int((two3 & top).sum()) >= 20 and int((two3 & (w["found"] > w["uix"])).sum()) >= 20
    for u in (2, 3, 4):
        m = w["uix"] == u
        assert 3 * int((m & top).sum()) >= int(m.sum()) and 3 * int((m & low).sum()) >= int(m.sum()), (u, int(m.sum()), int((m & top).sum()))


def check_long(built, o, data):
    """long: the labels the oracle's hit map gives reach every thread's stretch of the bitmap sweep, the first and the last word included;
    the named reads hold the ranks their names say."""
    ranks = {}
    for name, s in zip(data.split(b"\n")[0::2], seqs_of(data)):
        c = hitmap_ref.codes(o, s, False)
        ranks[name[1:].decode()] = sorted(set(built.rank_of[c[c < built.n]].tolist()))
    n, w = built.n, built.sweep_per - 1
    assert ranks["r0"] == [0] and ranks["rtop"] == [n - 1] and ranks["r0top"] == [0, n - 1]
    assert len(ranks["oneword"]) == 2 and len({r >> 5 for r in ranks["oneword"]}) == 1
    assert ranks["stretch"] == [32 * w + 31, 32 * w + 32] and (ranks["stretch"][0] >> 5) // built.sweep_per == 0 \
        and (ranks["stretch"][1] >> 5) // built.sweep_per == 1
    assert ranks["spread0"] == sorted({int(round(i * (n - 1) / 59)) for i in range(60)}) and len(ranks["spread0"]) == 60
    assert len(ranks["chain70"]) == 70
    assert li.touched_words_cover(built, ranks.values())
    assert not li.touched_words_cover(built, [ranks["spread0"]]) or built.nbw <= 60         # (no single read does it)


@pytest.mark.parametrize("name", list(li.SEARCH_RUNS))
def test_oracle_equals_reference_at_these_label_counts(name, workdir):
    """Every search tests/test_gpu_labels.py compares with the oracle: the inputs rebuilt here are the ones the genuine reference ran on,
    and the oracle writes the reference's bytes -- xtree-searchGG and xtree-search, both strand modes."""
    built = li.build_named(name, workdir)
    try:
        ctr_sha = util.sha256_of(built.ctr)
        o = orc.OracleDB.load(built.ctr)
        assert o.n_labels == built.n and o.label(built.edge[0]) == built.by_rank[0].encode() and o.label(built.edge[built.n - 1]) == built.by_rank[-1].encode()
        fa, out = workdir / "r.fa", workdir / "o.txt"
        for rank, kinds in ((False, li.SEARCH_RUNS[name]), (True, li.RANK_RUNS.get(name, ()))):
            for kind in kinds:
                data = li.reads_data(built, kind)
                fa.write_bytes(data)
                for rc in (False, True):
                    want = util.reference_run(li.run_key(name, kind, rc, rank), fa=data)
                    assert want["inputs"]["ctr"] == ctr_sha, "the database is not the one the reference was run on"
                    assert want["exit"] == 0
                    if out.exists():
                        out.unlink()
                    if rank:
                        code, nr, good, err = orc.rank_search_file(o, str(fa), str(out), rc=rc)
                    else:
                        code, nr, good, err = o.search_file(str(fa), str(out), threads=4, rc=rc)
                    assert code == 0 and nr == data.count(b">") and good > 0, err
                    assert util.sha256_of(str(out)) == want["outputs"]["out"], (name, kind, rc, rank)
                    if kind == "forms" and name in ("top19", "max16"):
                        check_forms(built, o, data, rc)
                if kind == "long":
                    check_long(built, o, data)
                if rank:                                                            # a read that keeps 64 hits or more: rank_vote_k<true>
                    fr = frame_fasta(data)
                    rs = orc.RankSearch(o)
                    r = rs.read_batch(np.frombuffer(data, dtype=np.uint8), fr["seq_off"], fr["seq_len"])
                    assert int(r["found"].max()) >= 64
                    rs.close()
        o.close()
    finally:
        os.remove(built.ctr)


def test_label_sets_are_what_the_module_says():
    """Distinct texts, seven ranks at most, a genus with its species, an empty last rank, tokens ending in '_'; the vote table's shape limits."""
    t = li.label_texts(65537)
    assert len(set(t)) == 65537 and max(s.count(";") for s in t) == 6
    assert t[0] + ";s__" == t[1] and t[2].startswith(t[0] + ";") and t[4].endswith("_") and t[6].startswith(t[3])
    for longest in (255, 256):
        s = li.shape_label_texts(300, np.random.default_rng(li.SHAPE_DATABASES["vt255"][3]), longest)
        ends = [[i for i, ch in enumerate(x) if ch == ";"] + [len(x)] for x in s]
        assert all(len(e) == 8 for e in ends) and max(e[-1] for e in ends) == longest and sum(1 for e in ends if e[3] > 127) > 250
