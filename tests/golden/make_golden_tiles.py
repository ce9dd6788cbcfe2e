#!/usr/bin/env python3
"""Generate golden/tiles_{vote,k64,ix32}_contigs.fa.gz, golden/tiles_{...}_out{,_rc}.txt.gz and golden/tiles_manifest.json: the contigs of
tests/tiles_ref.py, and what the genuine reference prints for their PRE-SPLIT FASTA -- one two-line record ><name>:<start>-<end> per tile
of the fixture's (W, S) -- which is what utree-tiles must write into tiles.tsv byte for byte.

    make -C oracle liboracle.so ref          # oracle/_ref/: xtree-searchGG, xtree-searchGG-k64, xtree-searchGG-ix32
    python tests/golden/make_golden_tiles.py

Every run uses 1 thread (the reference writes in input order then).  Before a file is written the Python restatement (tiles_ref.classify
over the CPU oracle) must equal the reference's output byte for byte.  The manifest records, per fixture, W and S, the SHA-256 of the contigs
and of the split FASTA, the tile count, and the reference's own "Good finds" and "Searched N queries" figures.  Data only: contigs, outputs
and hashes.  Under "scale" the manifest also holds, as hashes and counts alone, the reference's answers for the larger contigs the tests
generate themselves (scale() below), and its message for a broken header in the committed contigs."""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
import tiles_ref  # noqa: E402
import util  # noqa: E402
from oracle import orc  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def put_gz(path, data):
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=9, mtime=0, filename="") as g:
        g.write(data)


def scale(td):
    """The contigs that tests/test_gpu_tiles_scale.py generates at test time (tiles_ref.pass_contigs / file_contigs, fixture vote), at the
    widths the restatement is held to there: the reference on their pre-split FASTA, both strands.  Hashes and counts only -- neither the
    FASTA nor the outputs are kept.  And the reference's own message for the committed vote contigs with one header broken."""
    name = "vote"
    exe = os.path.join(REF, tiles_ref.REF_BINARY[name])
    ctr = util.fixture_ctr(name)
    o = orc.OracleDB.load(ctr)
    sp, out = os.path.join(td, "scale_split.fa"), os.path.join(td, "scale_out.txt")
    sets = {"pass": (tiles_ref.pass_contigs(), tiles_ref.pass_params(o.k)), "file": (tiles_ref.file_contigs(), {"file": tiles_ref.FILE_WS})}
    man = {}
    for key, (recs, params) in sets.items():
        buf, names, off, ln = tiles_ref.framed_arrays(recs)
        rec = {"contigs_sha256": tiles_ref.sha256(tiles_ref.fasta(recs)), "lengths": [len(s) for _, s in recs], "runs": {}}
        for pk, (W, S) in params.items():
            split = tiles_ref.fasta(tiles_ref.split_records(recs, W, S))
            open(sp, "wb").write(split)
            first = tiles_ref.plan_np(ln, W, S)
            n_tiles = int(first[-1])
            toff, tlen, tq, ti = tiles_ref.views_range(off, ln, W, S, 0, n_tiles, first)
            run = {"W": W, "S": S, "tiles": n_tiles, "split_sha256": tiles_ref.sha256(split)}
            for rc in (0, 1):
                if os.path.exists(out):
                    os.remove(out)
                r = subprocess.run([exe, ctr, sp, out, "1"] + (["RC"] if rc else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                assert r.returncode == 0, (key, pk, rc, r.returncode, r.stderr[-300:])
                got = open(out, "rb").read()
                res = tiles_ref.classify_views(o, buf, toff, tlen, bool(rc))
                text, seg, lines, nseg = tiles_ref.view_files(o, names, ln, W, S, tq, ti, res)
                assert text == got, "%s %s rc=%d: the restatement over the views differs from the reference" % (key, pk, rc)
                good = int(re.search(rb"Good finds: (\d+)", r.stdout).group(1))
                searched = int(re.search(rb"Searched (\d+) queries", r.stdout).group(1))
                assert searched == n_tiles and good == lines == got.count(b"\n")
                tag = "_rc" if rc else ""
                run["out%s_sha256" % tag] = tiles_ref.sha256(got)
                run["good_finds%s" % tag] = good
                run["searched%s" % tag] = searched
                run["segments%s" % tag] = nseg
                print("scale", key, pk, "rc=%d" % rc, "W", W, "S", S, "tiles", n_tiles, "lines", good, "segments", nseg, "bytes", len(got), flush=True)
            rec["runs"][pk] = run
        man[key] = rec
    # a framing error: what the reference says to the whole contigs with the '>' of one record broken
    bad = tiles_ref.broken_header(tiles_ref.contigs(name), tiles_ref.FRAMING_RECORD)
    open(sp, "wb").write(bad)
    r = subprocess.run([exe, ctr, sp, out, "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    m = re.search(rb"ERROR: no header '>' \[L (\d+)", r.stderr)
    assert r.returncode == 2 and m, (r.returncode, r.stderr[-300:])
    man["framing"] = {"record": tiles_ref.FRAMING_RECORD, "input_sha256": tiles_ref.sha256(bad), "exit": r.returncode, "index": int(m.group(1)),
                      "message": "ERROR: no header '>' [L %d]" % int(m.group(1))}
    print("scale framing: record", tiles_ref.FRAMING_RECORD, "->", man["framing"]["message"], flush=True)
    return man


def main():
    man = {"recipe": "oracle/Makefile ref; <binary> <fixture>.ctr split.fa out.txt 1 [RC]", "threads": 1, "fixtures": {}}
    with tempfile.TemporaryDirectory() as td:
        for name in tiles_ref.FIXTURES:
            exe = os.path.join(REF, tiles_ref.REF_BINARY[name])
            if not os.path.exists(exe):
                sys.exit("missing reference binary %s (make -C oracle ref)" % exe)
            W, S = tiles_ref.PARAMS[name]
            recs = tiles_ref.make_contigs(name)
            contigs = tiles_ref.fasta(recs)
            split = tiles_ref.fasta(tiles_ref.split_records(recs, W, S))
            ctr = util.fixture_ctr(name)
            o = orc.OracleDB.load(ctr)
            sp, out = os.path.join(td, "split.fa"), os.path.join(td, "out.txt")
            open(sp, "wb").write(split)
            n_tiles = sum(tiles_ref.n_tiles(len(s), W, S) for _, s in recs)
            rec = {"binary": tiles_ref.REF_BINARY[name], "W": W, "S": S, "queries": len(recs), "tiles": n_tiles,
                   "contigs_sha256": tiles_ref.sha256(contigs), "split_sha256": tiles_ref.sha256(split)}
            put_gz(os.path.join(HERE, "tiles_%s_contigs.fa.gz" % name), contigs)
            for rc in (0, 1):
                if os.path.exists(out):
                    os.remove(out)
                r = subprocess.run([exe, ctr, sp, out, "1"] + (["RC"] if rc else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                assert r.returncode == 0, (name, rc, r.returncode, r.stderr[-300:])
                got = open(out, "rb").read()
                tl = tiles_ref.classify(o, recs, W, S, bool(rc))
                assert tiles_ref.tiles_tsv(tl) == got, "%s rc=%d: the restatement differs from the reference" % (name, rc)
                good = int(re.search(rb"Good finds: (\d+)", r.stdout).group(1))
                searched = int(re.search(rb"Searched (\d+) queries", r.stdout).group(1))
                assert searched == n_tiles and good == got.count(b"\n")
                tag = "_rc" if rc else ""
                dst = os.path.join(HERE, "tiles_%s_out%s.txt.gz" % (name, tag))
                put_gz(dst, got)
                rec["out%s_sha256" % tag] = tiles_ref.sha256(got)
                rec["good_finds%s" % tag] = good
                rec["searched%s" % tag] = searched
                rec["segments%s" % tag] = tiles_ref.segments_tsv(recs, tl).count(b"\n")
                print(name, "rc=%d" % rc, "W", W, "S", S, "tiles", n_tiles, "lines", good, "segments", rec["segments%s" % tag], "bytes",
                      os.path.getsize(dst), flush=True)
            man["fixtures"][name] = rec
        man["scale"] = scale(td)
    json.dump(man, open(os.path.join(HERE, "tiles_manifest.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
