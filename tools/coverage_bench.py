#!/usr/bin/env python3
"""coverage_bench.py -- what the k-mer coverage report (UTREE_COVERAGE, utree_coverage_*) costs on one GPU, on bench.py's synthetic
database (default: config 2, 1.217e9 32-mers = 8 GB) and launches of 16 M x 150 bp reads:

  coverage_create   seconds, from the raw pieces in HBM (a device-to-device copy) and from the .ctr file (the dump streamed again)
  coverage_add      reads/s forward and with RC, HIP events around warmed-up launches
  coverage_count    seconds of one read-back (the streaming pass over dump and bitmap)
  file -> file      reads/s of the whole search with and without the coverage file, the two alternating

Prints one JSON line; --out also writes it to a file (profiles/coverage_bench.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_217_000_000)
    ap.add_argument("--batch-reads", type=int, default=16_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--e2e-reads", type=int, default=16_000_000, help="reads of the file -> file leg (0: skip it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from utree_amd import lib as ulib
    from utree_amd import synth
    from utree_amd.search import Coverage, CtrDB, search_gg
    assert torch.cuda.is_available(), "coverage_bench.py needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"nodes": args.nodes, "batch_reads": args.batch_reads, "read_len": args.read_len, "gpu": torch.cuda.get_device_name(0)}
    sdb = synth.make_db(dev, args.nodes, W=8, keep_raw=True)
    res["coverage_bytes"] = Coverage.bytes_needed(sdb.ctr)
    res["image_bytes"] = int(sdb.tree.info.image_bytes)

    def say(what):
        print("[coverage_bench] " + what, file=sys.stderr, flush=True)

    say("database built (%d nodes)" % sdb.n_nodes)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return time.time() - t0, out

    res["create_from_device_seconds"], cov = timed(lambda: sdb.tree.coverage(sdb.binix.view(torch.uint8), sdb.records))
    reads = synth.make_reads(sdb, args.batch_reads, args.read_len)
    for rc in (False, True):
        cov.add(reads.bases, reads.off, reads.length, rc=rc)                    # warm-up: code objects, the bitmap's first touches
        torch.cuda.synchronize()
        ms = []
        for rep in range(args.repeats):
            cov.reset()                                                          # every timed launch sets its bits anew
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            cov.add(reads.bases, reads.off, reads.length, rc=rc)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        again = []
        for rep in range(args.repeats):                                          # the same reads once more: every bit is there already
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            cov.add(reads.bases, reads.off, reads.length, rc=rc)
            b.record()
            torch.cuda.synchronize()
            again.append(a.elapsed_time(b))
        key = "add_rc" if rc else "add_forward"
        say("%s: %s ms, bits already set: %s ms" % (key, ms, again))
        res[key] = {"ms": ms, "reads_per_second": [args.batch_reads / (m * 1e-3) for m in ms],
                    "ms_bits_already_set": again, "reads_per_second_bits_already_set": [args.batch_reads / (m * 1e-3) for m in again]}
    counts = []
    for rep in range(args.repeats):
        s, (e, nr, nh) = timed(cov.entries)
        counts.append(s)
    res["count_seconds"] = counts
    say("count: %s s" % counts)
    res["covered_after_adds"] = int(e["covered"].sum())
    res["hits_after_adds"] = int(nh)
    # what the search itself does on these reads, for scale
    out = sdb.tree.classify(reads.bases, reads.off, reads.length, rc=False)
    torch.cuda.synchronize()
    cl = []
    for rep in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sdb.tree.classify(reads.bases, reads.off, reads.length, rc=False, out=out)
        b.record()
        torch.cuda.synchronize()
        cl.append(a.elapsed_time(b))
    res["classify_forward_ms"] = cl
    cov.close()
    del out

    if args.e2e_reads:
        need = 12 * 2**30 + 200 * args.e2e_reads
        base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * need else None
        d = tempfile.mkdtemp(prefix="utree_covbench_", dir=base)
        try:
            ctr_path, fa = os.path.join(d, "db.ctr"), os.path.join(d, "reads.fa")
            records = sdb.records.cpu().numpy()
            with open(ctr_path, "wb") as f:
                f.write(np.array([sdb.W, 0, 2, sdb.n_nodes], dtype="<u8").tobytes())
                f.write(sdb.binix.cpu().numpy().view(np.uint32).tobytes())
                for lo in range(0, records.size, 1 << 30):
                    f.write(records[lo:lo + (1 << 30)].tobytes())
                f.write(sdb.label_text)
            del records
            say(".ctr written")
            with open(fa, "wb") as f:
                done, b = 0, 0
                while done < args.e2e_reads:
                    n = min(args.batch_reads, args.e2e_reads - done)
                    r = synth.make_reads(sdb, args.batch_reads, args.read_len, seed=synth.READ_SEED + b)
                    if n < args.batch_reads:
                        r = synth.SynthReads(bases=r.bases[: n * args.read_len], off=r.off[:n], length=r.length[:n], n=n, read_len=args.read_len)
                    synth.fasta_tensor(r, done).cpu().numpy().tofile(f)
                    done += n
                    b += 1
                    del r
            del reads
            torch.cuda.empty_cache()
            db = CtrDB.open(ctr_path)                                            # the file: what a coverage handle streams the dump from
            import ctypes as C

            def create_from_file():
                h = C.c_void_p()
                ulib.check(ulib.load().utree_coverage_create(db._h, sdb.tree._h, None, None, C.byref(h)), "utree_coverage_create")
                return h
            res["create_from_file_seconds"], h = timed(create_from_file)
            ulib.load().utree_coverage_free(h)
            say("coverage handle from the file: %.2f s" % res["create_from_file_seconds"])
            arr = (C.c_void_p * 1)(sdb.tree._h)
            ulib.check(ulib.load().utree_search_prepare(db._h, arr, 1, 0), "utree_search_prepare")
            code, st = search_gg(db, [sdb.tree], fa, os.path.join(d, "warm.txt"))             # warm-up
            ulib.check(code, "utree_search_file")
            plain, withc = [], []
            for rep in range(args.repeats):
                for lst, covp in ((plain, None), (withc, os.path.join(d, "cov.tsv"))):
                    outp = os.path.join(d, "out.txt")
                    t0 = time.time()
                    code, st = search_gg(db, [sdb.tree], fa, outp, threads=16, coverage=covp)
                    wall = time.time() - t0
                    ulib.check(code, "utree_search_file_coverage" if covp else "utree_search_file")
                    lst.append({"wall_seconds": wall, "reads_per_second": st.n_reads / wall})
                    say("file -> file %s: %.3f s" % ("with coverage" if covp else "plain", wall))
                    os.unlink(outp)
            res["file_to_file"] = {"reads": args.e2e_reads, "plain": plain, "with_coverage": withc,
                                   "note": "with_coverage includes creating the handle (the node dump streamed from the .ctr) and the read-back"}
        finally:
            shutil.rmtree(d, ignore_errors=True)
    sdb.tree.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
