#!/usr/bin/env python3
"""Writes tests/golden/vote_out_rc.txt.gz: what the GENUINE reference prints for the committed `vote` fixture with RC
(`xtree-searchGG vote.ctr vote_reads.fa out.txt 1 RC`, the binary `make -C oracle ref` builds into oracle/_ref/).  make_golden.py's gen_vote
writes the forward output only; tests/test_hitmap_cpu.py pins this file's SHA-256.  Run from the repository root, where oracle/_ref exists."""
import gzip
import hashlib
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import util  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "xtree-searchGG")


def main():
    ctr, fa = util.fixture_ctr("vote"), util.fixture_reads_path("vote")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "out.txt")
        # the same binary must reproduce the committed forward output first
        subprocess.run([REF, ctr, fa, out, "1"], check=True, stdout=subprocess.DEVNULL)
        assert open(out, "rb").read() == util.fixture_bytes("vote_out.txt.gz"), "this reference build does not reproduce vote_out.txt.gz"
        subprocess.run([REF, ctr, fa, out, "1", "RC"], check=True, stdout=subprocess.DEVNULL)
        data = open(out, "rb").read()
    with gzip.GzipFile(os.path.join(HERE, "vote_out_rc.txt.gz"), "wb", mtime=0) as f:
        f.write(data)
    print("vote_out_rc.txt.gz: %d lines, sha256 %s" % (data.count(b"\n"), hashlib.sha256(data).hexdigest()))


if __name__ == "__main__":
    main()
