"""The search above 65 535 labels and at the lane pass's 2^19 - 1 limit (tests/label_inputs.py: databases by label count, reads by rank)
against the CPU oracle, which tests/test_labels_cpu.py holds to the genuine reference on these very inputs.

What depends on the label count and is reached here: utk_lanes_image_ok and the 19 rank bits of a tally slot (top19 / over19), the vote's
13 / 19 split of packed records, classify_long_k's touched-label bitmap in LDS and in HBM and its hist / touch rows left zero (lds, hbm,
top19), the rank-specific vote's histogram rows under the 512 MiB clamp, the vote table's 16-bit ids and 8-bit ends (max16, vt255, vt256),
the u16 rank fields with 0xFFFF as "none" (max16, max16k64, max16k16), and the reports' counters beyond their dense part (hbm).

Every comparison is byte equality with the oracle's text, or equality of all six record words.  Each test uploads one database.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import lib
from utree_amd.search import CtrDB, DeviceTree, classify_fasta_bytes, frame_fasta, search_gg
import coverage_ref
import hitmap_ref
import label_inputs as li
import profile_ref
import redist_ref
import samples_ref
from test_gpu_tally_inline import assert_records, records


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_CASES = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("labels")
    yield d
    for c in _CASES.values():                                   # up to 100 MB each
        c.o.close()
        if os.path.exists(c.built.ctr):
            os.remove(c.built.ctr)
    _CASES.clear()


class Case:
    """One database, made once per module and never changed; its reads and the oracle's answers, made when first asked for."""

    def __init__(self, name, workdir):
        self.built = li.build_named(name, workdir)
        self.o = orc.OracleDB.load(self.built.ctr)
        self.dir = workdir
        self._data, self._text, self._rec, self._rank = {}, {}, {}, {}

    def data(self, kind):
        if kind not in self._data:
            self._data[kind] = li.reads_data(self.built, kind)
        return self._data[kind]

    def fasta(self, kind):
        p = self.dir / ("%s_%s.fa" % (self.built.name, kind.replace("+", "")))
        if not p.exists():
            p.write_bytes(self.data(kind))
        return str(p)

    def text(self, kind, rc, rank=False):
        key = (kind, rc, rank)
        if key not in self._text:
            out = self.dir / "oracle.txt"
            if rank:
                code, nr, good, err = orc.rank_search_file(self.o, self.fasta(kind), str(out), rc=rc)
            else:
                code, nr, good, err = self.o.search_file(self.fasta(kind), str(out), threads=8, rc=rc)
            assert code == 0 and good > 0, err
            self._text[key] = out.read_bytes()
        return self._text[key]

    def records(self, kind, rc):
        if (kind, rc) not in self._rec:
            data = self.data(kind)
            fr = frame_fasta(data)
            self._rec[(kind, rc)] = (fr, self.o.classify_batch(np.frombuffer(data, dtype=np.uint8), fr["seq_off"], fr["seq_len"], rc=rc, threads=8))
        return self._rec[(kind, rc)]


def case(name, workdir):
    if name not in _CASES:
        _CASES[name] = Case(name, workdir)
    return _CASES[name]


def upload(c, monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    db = CtrDB.open(c.built.ctr)
    tree = DeviceTree.upload(db, 0)
    assert tree.info.irregular_bins == 0 and not tree.info.generic_mode
    return db, tree


def check(c, db, tree, kinds, monkeypatch, lane_passes=("1", "0"), words=True):
    """The kinds through the lane pass (where the handle takes it) and through the wave-per-read kernels, both strands: the text, and with
    `words` all six record words; kernel_name() says which family ran."""
    for lane_pass in lane_passes:
        monkeypatch.setenv("UTREE_LANE_PASS", lane_pass)
        for kind in kinds:
            for rc in (False, True):
                got = classify_fasta_bytes(db, tree, c.data(kind), rc=rc)
                name = tree.kernel_name()
                if lane_pass == "1" and tree.info.lane_pass:
                    assert name.startswith("classify_lanes_"), name
                else:
                    assert not name.startswith("classify_lanes_"), name
                assert got == c.text(kind, rc), (c.built.name, kind, rc, lane_pass)
                if words:
                    import torch
                    fr, want = c.records(kind, rc)
                    assert_records(records(torch, tree, c.data(kind), fr, rc), want, (c.built.name, kind, rc, lane_pass))
    monkeypatch.delenv("UTREE_LANE_PASS")


def check_files(c, db, tree, kinds, tmp_path):
    """The same reads through search_gg's device text pipeline: fmt_len_k / fmt_write_k print the labels."""
    for kind in kinds:
        for rc in (False, True):
            out = tmp_path / "o.txt"
            code, st = search_gg(db, [tree], c.fasta(kind), str(out), rc=rc)
            assert code == lib.OK and st.pipeline == 1
            assert out.read_bytes() == c.text(kind, rc), (c.built.name, kind, rc)


# ---- the databases themselves ----------------------------------------------------------------------------------------------------------------
# name: (lane_pass, vote_table) the handle must report
EXPECT = {"top19": (1, 0), "over19": (0, 0), "lds": (1, 0), "hbm": (1, 0), "hbm64": (0, 0), "max16": (1, 1), "max16k64": (1, 1),
          "max16k16": (None, None), "vt255": (1, 1), "vt256": (1, 0)}


@pytest.mark.parametrize("name", list(EXPECT))
def test_database_uploads_regular(torch_cuda, workdir, monkeypatch, name):
    """Each database is written here, once (a .ctr of 2^19 labels takes the host a second); every bin is regular, and the handle says which
    passes it takes: the lane pass up to 2^19 - 2 labels and not from 2^19 - 1, the vote table up to 65 534 labels of at most 255 bytes."""
    c = case(name, workdir)
    db, tree = upload(c, monkeypatch)
    lane_pass, vote_table = EXPECT[name]
    if lane_pass is not None:
        assert (tree.info.lane_pass, tree.info.vote_table) == (lane_pass, vote_table)
    tree.close()
    db.close()


# ---- 1, 2: the lane pass's limit of 2^19 - 1 labels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["forms", "lanes"])
@pytest.mark.parametrize("inline", [None, "0"], ids=["packed", "listed"])
def test_last_label_count_the_lane_pass_takes(torch_cuda, workdir, monkeypatch, inline, kind):
    """2^19 - 2 labels, u32 indices: the lane pass takes the image, the highest rank's tally slot lies just under the all-ones empty marker,
    and the vote unpacks two- and three-label records with 19 bits of rank -- packed (default) and listed (UTREE_TALLY_INLINE=0)."""
    c = case("top19", workdir)
    db, tree = upload(c, monkeypatch)
    assert tree.info.lane_pass == 1 and tree.info.vote_table == 0
    if inline is None:
        monkeypatch.delenv("UTREE_TALLY_INLINE", raising=False)
    else:
        monkeypatch.setenv("UTREE_TALLY_INLINE", inline)
    check(c, db, tree, (kind,), monkeypatch)
    tree.close()
    db.close()


@pytest.mark.parametrize("name,kind", [("top19", "forms"), ("top19", "lanes"), ("max16", "forms")])
def test_device_text_prints_19_bit_label_indices(torch_cuda, workdir, tmp_path, monkeypatch, name, kind):
    """The same reads through search_gg's device text pipeline: fmt_len_k / fmt_write_k print labels whose index needs 19 bits (and 0xFFFD)."""
    c = case(name, workdir)
    db, tree = upload(c, monkeypatch)
    check_files(c, db, tree, (kind,), tmp_path)
    tree.close()
    db.close()


@pytest.mark.parametrize("kind", ["forms", "lanes"])
def test_first_label_count_the_lane_pass_leaves(torch_cuda, workdir, monkeypatch, kind):
    """2^19 - 1 labels: rank 2^19 - 2 with a full count would be the empty marker, so the handle falls back to the wave-per-read kernels."""
    c = case("over19", workdir)
    db, tree = upload(c, monkeypatch)
    assert tree.info.lane_pass == 0
    check(c, db, tree, (kind,), monkeypatch, lane_passes=("1",))
    if kind == "forms":
        assert "classify_short_k" in tree.kernel_name(), tree.kernel_name()
    tree.close()
    db.close()


# ---- 3: classify_long_k's bitmap -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds", "hbm", "top19"])
def test_long_read_bitmap_in_lds_and_in_hbm(torch_cuda, workdir, monkeypatch, name):
    """65 536 labels: 2048 bitmap words, still in LDS; 65 537: 2049 words in HBM, nine to a thread; 2^19 - 2: 64 to a thread.  Reads of rank 0,
    of the highest rank, of two ranks in one word, of the two ranks either side of thread 0's last word, and 300 ranks that reach every
    thread's stretch.  Without the lane pass every read goes to classify_long_k; with it they are taken in pieces."""
    c = case(name, workdir)
    db, tree = upload(c, monkeypatch)
    assert tree.info.lane_pass == 1
    check(c, db, tree, ("long",), monkeypatch, lane_passes=("0", "1"))
    monkeypatch.setenv("UTREE_LANE_PASS", "0")
    classify_fasta_bytes(db, tree, c.data("long"), rc=False)
    assert "classify_long_k" in tree.kernel_name(), tree.kernel_name()
    tree.close()
    db.close()


@pytest.mark.parametrize("name", ["hbm", "top19"])
def test_long_read_rows_are_left_zero(torch_cuda, workdir, monkeypatch, name):
    """2500 long reads are more than classify_long_k has workgroups: some workgroup takes a second read on its hist / touch rows; the batch
    again on the same handle finds the rows every workgroup left."""
    c = case(name, workdir)
    db, tree = upload(c, monkeypatch, UTREE_LANE_PASS="0")
    fr, want = c.records("many_long", False)
    assert len(want) == li.N_MANY > 2048 and int(fr["seq_len"].min()) >= li.LONG_MIN
    for turn in (1, 2):
        got = records(torch_cuda, tree, c.data("many_long"), fr, False)
        assert "classify_long_k" in tree.kernel_name(), tree.kernel_name()
        assert_records(got, want, (name, turn))
    assert classify_fasta_bytes(db, tree, c.data("many_long"), rc=True) == c.text("many_long", True)
    tree.close()
    db.close()


def test_wave_per_read_kernels_alone_with_u32_labels(torch_cuda, workdir, monkeypatch):
    """k = 64 with u32 labels has no lane pass: classify_short_k / the mid pass / classify_long_k at 65 537 labels."""
    c = case("hbm64", workdir)
    db, tree = upload(c, monkeypatch)
    assert tree.info.lane_pass == 0
    check(c, db, tree, ("forms", "long"), monkeypatch, lane_passes=("1",))
    tree.close()
    db.close()


# ---- 4: the I = 2 maximum ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [("max16", {}), ("max16", {"UTREE_VOTE_BYTES": "1"}), ("max16", {"UTREE_OVF_CHAINS": "1"}),
                                      ("max16", {"UTREE_BUCKET_BYTES": "128"}), ("max16k64", {}), ("max16k16", {})],
                         ids=["max16", "max16-vote_bytes", "max16-chains", "max16-bucket128", "max16k64", "max16k16"])
def test_most_labels_u16_indices_hold(torch_cuda, workdir, monkeypatch, name, env):
    """65 534 labels: the highest rank is 0xFFFD, 0xFFFF means "none" in a record's, a chain's and the direct table's rank field, and the vote
    table's prefix ids reach 65 533 with 0xFFFF for "no token"."""
    c = case(name, workdir)
    db, tree = upload(c, monkeypatch, **env)
    if name == "max16":
        assert tree.info.vote_table == (0 if "UTREE_VOTE_BYTES" in env else 1) and tree.info.lane_pass == 1
        assert tree.info.overflow_chains == (1 if "UTREE_OVF_CHAINS" in env else 0) and tree.info.bucket_bytes == int(env.get("UTREE_BUCKET_BYTES", 64))
    check(c, db, tree, ("forms", "long"), monkeypatch)
    tree.close()
    db.close()


# ---- 5: the vote table's shape limits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,table", [("vt255", 1), ("vt256", 0)])
def test_vote_table_shape_limits(torch_cuda, workdir, monkeypatch, name, table):
    """Labels of exactly eight tokens and 200 .. 255 bytes keep the table (tok_end and len reach 255); one label of 256 bytes drops it.  Both
    votes give the oracle's lines."""
    c = case(name, workdir)
    assert max(len(s) for s in c.built.labels) == (255 if table else 256) and all(s.count(";") == 7 for s in c.built.labels)
    for vote_bytes in (False, True):
        db, tree = upload(c, monkeypatch, **({"UTREE_VOTE_BYTES": "1"} if vote_bytes else {}))
        assert tree.info.vote_table == (table if not vote_bytes else 0)
        check(c, db, tree, ("forms",), monkeypatch)
        tree.close()
        db.close()
        monkeypatch.delenv("UTREE_VOTE_BYTES", raising=False)


# ---- 6: the rank-specific search ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("name", ["top19", "hbm"])
def test_rank_search_above_16_bits(torch_cuda, workdir, tmp_path, name, rc):
    """xtree-search on 2^19 - 2 and 65 537 labels: the read of 70 k-mers keeps more than 64 hits and takes rank_vote_k<true>, whose histogram
    rows the 512 MiB clamp counts (256 and 2047 waves, not n_cu * 8)."""
    c = case(name, workdir)
    for rc in (rc,):
        out = tmp_path / ("rank%d.txt" % rc)
        r = subprocess.run([lib.RANK_CLI_PATH, c.built.ctr, c.fasta("forms+long"), str(out), "4"] + (["RC"] if rc else []),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        assert out.read_bytes() == c.text("forms+long", rc, rank=True), (name, rc)


# ---- 7: the reports ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True])
def test_reports_above_16_bits(torch_cuda, workdir, tmp_path, monkeypatch, rc):
    """Profile, coverage, redistribution, hit map and sample table in one search of 65 537 labels (the request fields UTREE_PROFILE, UTREE_COVERAGE,
    UTREE_REDISTRIBUTE, UTREE_HITMAP and UTREE_SAMPLE_TABLE fill): 3000 single-k-mer reads on random labels over three samples give every
    workgroup far more distinct labels than its dense counters and LDS hash slots hold."""
    c = case("hbm", workdir)
    kind = "forms+long+singles"
    data = c.data(kind)
    names = profile_ref.fasta_names(data)
    seqs = data.split(b"\n")[1::2]
    db, tree = upload(c, monkeypatch)
    for rc in (rc,):
        want = c.text(kind, rc)
        p = {k: str(tmp_path / ("%s%d" % (k, rc))) for k in ("profile", "coverage", "redistribute", "hitmap", "samples")}
        out = tmp_path / ("o%d.txt" % rc)
        code, st = search_gg(db, [tree], c.fasta(kind), str(out), rc=rc, **p)
        assert code == lib.OK and st.n_reads == len(names)
        assert out.read_bytes() == want
        assert open(p["profile"], "rb").read() == profile_ref.profile_ref(want, names, len(names))
        assert open(p["samples"], "rb").read() == samples_ref.samples_ref(want, names, len(names))
        dbk, cov, hits, texts = coverage_ref.coverage_counts(c.built.ctr, seqs, rc)
        assert int((hits > 0).sum()) > 3000
        assert open(p["coverage"], "rb").read() == coverage_ref.coverage_file(dbk, cov, hits, texts, len(names))
        assert open(p["redistribute"], "rb").read() == redist_ref.reference_file(c.built.ctr, seqs, rc)
        maps = hitmap_ref.hitmap(c.built.ctr, seqs, rc, o=c.o)
        assert open(p["hitmap"], "rb").read() == hitmap_ref.file_bytes(names, maps)
        if not rc:
            assert open(p["hitmap"] + ".labels", "rb").read() == hitmap_ref.labels_bytes(c.built.ctr, o=c.o)
    tree.close()
    db.close()
