"""Two- and three-label tallies kept in the pending result record (csrc/lanes_core.hpp phase C: CUT_INLINE; csrc/kernels.hip: the vote's
list accessor) against the CPU oracle, with UTREE_TALLY_INLINE=0 (every list in the workspace, as before) beside the default on the same
handle: reads of every label count in one wavefront, both label widths, k = 32 and 64, both strands, the table vote and the byte vote;
reads of two lanes; the committed vote multisets; and the proof that a packed read takes no list space (UTREE_TEST_TALLY_CAP=1).

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import orc
from utree_amd import ctrfile, lib
from utree_amd.search import CtrDB, DeviceTree, frame_fasta, search_gg
import util
from test_gpu_lanes import OwnDB, oracle_text
from test_gpu_parity import fasta_bytes, random_reads, tree_for

FIELDS = ("label", "cut", "found", "uix", "sl", "ol")
N_FORMS = 64 * 5 + 37                     # five full grabs and a ragged one; one full 256-read vote block and a ragged one


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def rnd(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


class RunsDB:
    """OwnDB's shape -- 60 000 k-mers under its four-rank label tree, every bin regular -- with the k-mers in 12 000 runs of five consecutive
    windows of one sequence, each run labelled with one to five labels: a read of 150 bases can then carry five labels at k = 64 too, and
    repeated labels come by themselves.  A piece is what a read is built from: the bases of c consecutive k-mers of a run, with their labels."""
    S = 5

    def __init__(self, tmp_path, k, seed):
        self.k = k
        rng = np.random.default_rng(seed)
        self.labels = ["k__A;p__P%d;c__C%d;o__O%d" % (a, b, c) for a in range(3) for b in range(3) for c in range(4)]
        self.labels += ["k__A;p__P%d;c__C%d" % (a, b) for a in range(3) for b in range(3)] + ["k__A;p__P%d" % a for a in range(3)]
        n = 12_000
        self.seq = rng.integers(0, 4, (n, k + self.S - 1)).astype(np.uint64)
        self.lab = np.zeros((n, self.S), np.uint32)
        for s in range(n):
            pal = rng.choice(len(self.labels), int(rng.integers(1, self.S + 1)), replace=False)
            self.lab[s] = pal[rng.integers(0, len(pal), self.S)]
        hi = np.zeros((n, self.S), np.uint64)
        lo = np.zeros((n, self.S), np.uint64)
        for j in range(self.S):
            w = self.seq[:, j:j + k]
            for i in range(k):
                if k == 64 and i < 32:
                    hi[:, j] = (hi[:, j] << np.uint64(2)) | w[:, i]
                else:
                    lo[:, j] = (lo[:, j] << np.uint64(2)) | w[:, i]
        hi, lo, ix = hi.ravel(), lo.ravel(), self.lab.ravel()
        order = np.lexsort((lo, hi))
        keep = np.ones(len(order), bool)
        keep[1:] = (hi[order][1:] != hi[order][:-1]) | (lo[order][1:] != lo[order][:-1])
        assert keep.all()                                                               # (random sequence: no k-mer twice)
        self.ctr = str(tmp_path / ("runs%d.ctr" % k))
        ctrfile.write_ctr(self.ctr, k // 4, 2, hi[order], lo[order], ix[order], self.labels)
        self.by_label = [np.argwhere(self.lab == l) for l in range(len(self.labels))]

    def piece(self, rng, have=()):
        s, c = int(rng.integers(0, len(self.seq))), int(rng.integers(1, self.S + 1))
        j = int(rng.integers(0, self.S - c + 1))
        return "".join("ACGT"[int(x)] for x in self.seq[s, j:j + self.k + c - 1]), [int(x) for x in self.lab[s, j:j + c]]

    def kmer_of(self, rng, label):
        s, j = self.by_label[label][int(rng.integers(0, len(self.by_label[label])))]
        return "".join("ACGT"[int(x)] for x in self.seq[s, j:j + self.k]), [label]


class FixtureKmers:
    """A committed database (ix32: u32 labels) as a source of pieces: single k-mers with their labels."""

    def __init__(self, name):
        d = util.load_db_fixture(name)
        self.k = d.k
        self.hi, self.lo = d.words()
        self.ix = d.ix()
        self.labels = d.labels()
        self.ctr = util.fixture_ctr(name)
        self.by_label = {int(l): np.flatnonzero(self.ix == l) for l in np.unique(self.ix)}

    def piece(self, rng, have=()):
        """... every other one with a label the read has already: counts above one"""
        j = int(rng.integers(0, len(self.lo)))
        if have and rng.random() < 0.5:
            same = self.by_label[have[int(rng.integers(0, len(have)))]]
            j = int(same[int(rng.integers(0, len(same)))])
        return ctrfile.decode_kmer(int(self.hi[j]), int(self.lo[j]), self.k), [int(self.ix[j])]


def build_read(rng, src, n_labels, L):
    """A read of L bases whose pieces carry exactly n_labels distinct labels.  (What the oracle then says is what counts: behind a piece that
    ends inside its run, the window one base on is the run's next k-mer whenever the base that follows happens to fit.)"""
    for _ in range(4000):
        parts, labs, used = [], [], 0
        for _ in range(12):
            b, l = src.piece(rng, labs)
            if used + len(b) > L or len(set(labs + l)) > n_labels:
                continue
            parts.append(b); labs += l; used += len(b)
            if len(set(labs)) == n_labels and rng.random() < 0.4:
                break
        if len(set(labs)) == n_labels:
            front = int(rng.integers(0, L - used + 1))
            return rnd(rng, front) + "".join(parts) + rnd(rng, L - used - front)
    raise AssertionError("no read of %d labels in %d bases" % (n_labels, L))


def with_one_n(rng, s):
    p = int(rng.integers(0, len(s)))
    return s[:p] + "N" + s[p + 1:]


def form_reads(rng, src, special):
    """N_FORMS shuffled reads: none to five labels each (five: 160 bases), a sixth of them with one N; `special`: reads of chosen labels."""
    reads = list(special)
    i = 0
    while len(reads) < N_FORMS:
        nl = i % 6
        s = build_read(rng, src, nl, 160 if nl == 5 else 150)
        reads.append(("f%d_%d" % (nl, i), with_one_n(rng, s) if i % 6 == i // 6 % 6 else s))
        i += 1
    return [reads[j] for j in rng.permutation(len(reads))]


def special_reads(rng, src):
    """A leaf with its own ancestor (the vote's "less specific" branch), with counts above one, and two siblings."""
    L = src.labels
    leaf = [i for i, l in enumerate(L) if l.count(";") == 3]
    out = []
    n_k = 150 // src.k                                                                   # single k-mers a read holds
    for i in range(12):
        a = leaf[int(rng.integers(0, len(leaf)))]
        anc = L.index(L[a].rsplit(";", 1 + i % 2)[0])                                  # its class, or its phylum
        sib = L.index(L[a][:-1] + str((int(L[a][-1]) + 1 + i % 3) % 4))                 # another order of the same class
        for tag, pair in (("anc", (a, anc)), ("sib", (a, sib))):
            picks = [pair[j % 2] for j in range(n_k)] if i % 3 else [pair[0]] + [pair[1]] * (n_k - 1)
            s = "".join(src.kmer_of(rng, l)[0] for l in picks)
            out.append(("%s%d" % (tag, i), s + rnd(rng, 150 - len(s))))
    return out


def records(torch, tree, data, fr, rc):
    buf = np.frombuffer(data, dtype=np.uint8)
    res = tree.classify(torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(fr["seq_off"].astype(np.int64)).cuda(),
                        torch.from_numpy(fr["seq_len"].astype(np.int32)).cuda(), rc=rc)
    torch.cuda.synchronize()
    tree.poll()
    return res.cpu().numpy()


def assert_records(got, want, what):
    g = got.view(np.uint32)
    for j, f in enumerate(FIELDS):
        w = want[f].view(np.uint32) if want[f].dtype != np.uint32 else want[f]
        bad = np.flatnonzero(g[:, j] != w)
        assert len(bad) == 0, (what, f, bad[:5], g[bad[:5]], [want[x][bad[:5]] for x in FIELDS])


_CASES = {}


def forms_case(name, tmp_path_factory):
    """The database, its reads and the oracle's answers, once per database."""
    if name not in _CASES:
        tmp = tmp_path_factory.mktemp("forms_" + name)
        rng = np.random.default_rng({"own": 11, "own64": 12, "ix32": 13}[name])
        if name == "ix32":
            src = FixtureKmers("ix32")
            special = []
        else:
            src = RunsDB(tmp, 64 if name == "own64" else 32, seed=5)
            special = special_reads(rng, src)
        data = fasta_bytes(form_reads(rng, src, special))
        fr = frame_fasta(data)
        assert len(fr["seq_off"]) == N_FORMS
        o = orc.OracleDB.load(src.ctr)
        buf = np.frombuffer(data, dtype=np.uint8)
        want, text = {}, {}
        for rc in (False, True):
            want[rc] = o.classify_batch(buf, fr["seq_off"], fr["seq_len"], rc=rc, threads=8)
            text[rc] = oracle_text(o, data, tmp, rc=rc)
            # every form is there, in every quarter of the batch (a grab of 64 mixes them), and some labels were hit more than once
            for u in range(6):
                assert int((want[rc]["uix"] == u).sum()) >= 20, (name, rc, u, np.bincount(want[rc]["uix"]))
                assert all(int((want[rc]["uix"][q:q + 96] == u).sum()) >= 1 for q in range(0, N_FORMS - 95, 87)), (name, rc, u)
            assert int(((want[rc]["uix"] >= 2) & (want[rc]["uix"] <= 3) & (want[rc]["found"] > want[rc]["uix"])).sum()) >= 20
        _CASES[name] = (src, data, fr, want, text, tmp)
    return _CASES[name]


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("vote_bytes", [False, True])
@pytest.mark.parametrize("name", ["own", "own64", "ix32"])
def test_every_form_in_one_wavefront(torch_cuda, name, vote_bytes, rc, tmp_path, tmp_path_factory, monkeypatch):
    """Reads of no, one, two, three, four and five labels, repeated labels, a leaf with its ancestor, siblings, an N -- shuffled, so that every
    grab of 64 packs some records and lists others: all six result words and the file pipeline's text against the oracle, packed and listed."""
    src, data, fr, want, text, tmp = forms_case(name, tmp_path_factory)
    if vote_bytes:
        monkeypatch.setenv("UTREE_VOTE_BYTES", "1")                                      # (read when the image is built)
    db = CtrDB.open(src.ctr)
    tree = DeviceTree.upload(db, 0)
    # (u32 label indices do not fit the label table's 16-bit ids: ix32 votes from the label bytes either way)
    assert tree.info.vote_table == int(not vote_bytes and name != "ix32") and tree.info.lane_pass == 1
    fa = tmp_path / "r.fa"
    fa.write_bytes(data)
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("UTREE_TALLY_INLINE", raising=False)
        else:
            monkeypatch.setenv("UTREE_TALLY_INLINE", switch)
        got = records(torch_cuda, tree, data, fr, rc)
        assert tree.kernel_name().startswith("classify_lanes_k<%d, %d, 1," % (src.k // 4, 4 if name == "ix32" else 2)), tree.kernel_name()
        if rc and name != "ix32":
            assert tree.kernel_name().endswith("true>"), tree.kernel_name()              # both strands from one pass
        assert_records(got, want[rc], (name, vote_bytes, rc, switch))
        out = tmp_path / ("o%s.txt" % switch)
        code, stats = search_gg(db, [tree], str(fa), str(out), rc=rc)
        assert code == 0 and out.read_bytes() == text[rc]
    tree.close()


def test_reads_of_two_lanes_among_reads_of_one(torch_cuda, tmp_path, tmp_path_factory, monkeypatch):
    """Reads of 161 to 300 bases take two lanes and 24 tally slots (classify_lanes_mixed_k: the listed classes); their two and three labels are
    packed like a one-lane read's, their four listed."""
    src = forms_case("own", tmp_path_factory)[0]
    rng = np.random.default_rng(31)
    reads = [("s%d" % i, build_read(rng, src, i % 5, 150)) for i in range(150)]
    reads += [("l%d" % i, build_read(rng, src, 2 + i % 3, int(rng.integers(161, 301)))) for i in range(120)]
    reads = [reads[j] for j in rng.permutation(len(reads))]
    data = fasta_bytes(reads)
    fr = frame_fasta(data)
    o = orc.OracleDB.load(src.ctr)
    want = o.classify_batch(np.frombuffer(data, dtype=np.uint8), fr["seq_off"], fr["seq_len"], rc=False, threads=8)
    long_ = fr["seq_len"] > 160
    for u in (2, 3, 4):
        assert int((want["uix"][long_] == u).sum()) >= 12 and int((want["uix"][~long_] == u).sum()) >= 12
    db = CtrDB.open(src.ctr)
    tree = DeviceTree.upload(db, 0)
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("UTREE_TALLY_INLINE", raising=False)
        else:
            monkeypatch.setenv("UTREE_TALLY_INLINE", switch)
        got = records(torch_cuda, tree, data, fr, False)
        assert tree.kernel_name().startswith("classify_lanes_mixed_k<8, 2,"), tree.kernel_name()
        assert_records(got, want, switch)
    tree.close()


def test_committed_vote_multisets_packed_and_listed(torch_cuda, monkeypatch):
    """The `vote` fixture's reads (the reference's own output is committed): the records with the switch on and off are the same, and the text
    formatted from them is the golden."""
    db, tree = tree_for("vote")
    data = util.fixture_bytes("vote_reads.fa.gz")
    fr = frame_fasta(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    got = {}
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("UTREE_TALLY_INLINE", raising=False)
        else:
            monkeypatch.setenv("UTREE_TALLY_INLINE", switch)
        got[switch] = records(torch_cuda, tree, data, fr, False)
        assert tree.kernel_name().startswith("classify_lanes_"), tree.kernel_name()
        assert db.format(buf, fr["name_off"], fr["name_len"], got[switch]) == util.fixture_bytes("vote_out.txt.gz")
    assert np.array_equal(got[None], got["0"])
    uix = got[None][:, 3]
    assert int(((uix == 2) | (uix == 3)).sum()) >= 100 and int((uix >= 4).sum()) >= 100        # both forms were there to compare


def test_packed_reads_take_no_list_space(torch_cuda, tmp_path, monkeypatch):
    """Every read of the batch has three labels at most.  With room for ONE list entry (the test hook) the batch is clean and right: nothing was
    reserved.  The same batch with every list in the workspace raises the error word -- the kernels write into the first chunk, nothing
    faults -- and the next batch, hook off, is fine."""
    d = OwnDB(tmp_path, seed=4)
    rng = np.random.default_rng(41)
    hi, lo = d.words()
    reads = []
    for i in range(20_000):                                                              # three database k-mers at most: three labels at most
        ks = [ctrfile.decode_kmer(int(hi[j]), int(lo[j]), 32) for j in rng.integers(0, len(lo), i % 4)]
        s = "".join(k_ + rnd(rng, int(rng.integers(0, 9))) for k_ in ks)
        reads.append(("p%d" % i, (s + rnd(rng, 150))[:150]))
    data = fasta_bytes(reads)
    fr = frame_fasta(data)
    o = orc.OracleDB.load(d.ctr)
    want = o.classify_batch(np.frombuffer(data, dtype=np.uint8), fr["seq_off"], fr["seq_len"], rc=False, threads=8)
    assert int(want["uix"].max()) == 3 and int((want["uix"] == 2).sum()) > 3000 and int((want["uix"] == 3).sum()) > 3000   # else the first half proves nothing
    db = CtrDB.open(d.ctr)
    tree = DeviceTree.upload(db, 0)
    monkeypatch.setenv("UTREE_LANE_PASS", "1")
    monkeypatch.delenv("UTREE_TALLY_INLINE", raising=False)
    monkeypatch.setenv("UTREE_TEST_TALLY_CAP", "1")
    assert_records(records(torch_cuda, tree, data, fr, False), want, "packed, no list space")
    assert tree.kernel_name().startswith("classify_lanes_k<8, 2, 1,")
    monkeypatch.setenv("UTREE_TALLY_INLINE", "0")
    with pytest.raises(lib.UtreeError) as ei:
        records(torch_cuda, tree, data, fr, False)
    assert ei.value.code == lib.E_DEVICE
    monkeypatch.delenv("UTREE_TEST_TALLY_CAP")
    assert_records(records(torch_cuda, tree, data, fr, False), want, "listed, hook off")
    monkeypatch.delenv("UTREE_TALLY_INLINE")
    assert_records(records(torch_cuda, tree, data, fr, False), want, "packed, hook off")
    tree.close()
