#!/usr/bin/env python3
"""Generate golden/pairs_{toy,vote,k64}_out{,_rc}.txt.gz and golden/pairs_manifest.json: what the genuine reference prints for the pairs
of tests/pairs_ref.py, each searched as ONE query mate 1 + "N" + mate 2 under mate 1's name (with RC the reference itself appends
'N' + the reverse complement, itree.c:891-898).

    make -C oracle liboracle.so ref          # oracle/_ref/: xtree-searchGG, xtree-searchGG-k64
    python tests/golden/make_golden_pairs.py

Every run uses 1 thread (the reference writes in input order then).  Before a file is written the CPU oracle's search_file on the same
joined input must equal the reference's output byte for byte.  The manifest records, per fixture, the SHA-256 of the joined input, the
pair count, and for how many pairs the line differs from the line of mate 1 searched alone (forward, RC): an implementation that ignores
or mangles mate 2 cannot reproduce the files.  Only outputs and hashes are committed; the inputs are rebuilt by the tests."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
import pairs_ref  # noqa: E402
import util  # noqa: E402
from oracle import orc  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    man = {"recipe": "oracle/Makefile ref; <binary> <fixture>.ctr joined.fa out.txt 1 [RC]", "threads": 1, "fixtures": {}}
    with tempfile.TemporaryDirectory() as td:
        for name in pairs_ref.FIXTURES:
            exe = os.path.join(REF, pairs_ref.REF_BINARY[name])
            if not os.path.exists(exe):
                sys.exit("missing reference binary %s (make -C oracle ref)" % exe)
            P = pairs_ref.Pairs(name)
            ctr = util.fixture_ctr(name)
            o = orc.OracleDB.load(ctr)
            joined, alone = P.joined_fasta(), P.reads_fasta()
            jp, ap, out, want = (os.path.join(td, f) for f in ("joined.fa", "alone.fa", "out.txt", "oracle.txt"))
            open(jp, "wb").write(joined)
            open(ap, "wb").write(alone)
            rec = {"binary": pairs_ref.REF_BINARY[name], "pairs": P.n, "joined_sha256": pairs_ref.sha256(joined), "differs_from_mate1": []}
            for rc in (0, 1):
                if os.path.exists(out):
                    os.remove(out)
                r = subprocess.run([exe, ctr, jp, out, "1"] + (["RC"] if rc else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                assert r.returncode == 0, (name, rc, r.returncode, r.stderr[-300:])
                got = open(out, "rb").read()
                code, nr, good, err = o.search_file(jp, want, threads=1, rc=bool(rc))
                assert code == 0 and nr == P.n and open(want, "rb").read() == got, "%s rc=%d: the CPU oracle differs from the reference" % (name, rc)
                code, nr, good, err = o.search_file(ap, want, threads=1, rc=bool(rc))
                assert code == 0 and nr == P.n
                a, b = pairs_ref.lines_by_name(got, P.names1), pairs_ref.lines_by_name(open(want, "rb").read(), P.names1)
                rec["differs_from_mate1"].append(sum(1 for i in range(P.n) if a.get(i) != b.get(i)))
                dst = os.path.join(HERE, "pairs_%s_out%s.txt.gz" % (name, "_rc" if rc else ""))
                with open(dst, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=9, mtime=0, filename="") as g:
                    g.write(got)
                rec["out%s_sha256" % ("_rc" if rc else "")] = pairs_ref.sha256(got)
                rec["lines%s" % ("_rc" if rc else "")] = got.count(b"\n")
                print(name, "rc=%d" % rc, "pairs", P.n, "lines", got.count(b"\n"), "differ from mate 1 alone", rec["differs_from_mate1"][-1],
                      "bytes", os.path.getsize(dst), flush=True)
            man["fixtures"][name] = rec
    json.dump(man, open(os.path.join(HERE, "pairs_manifest.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
