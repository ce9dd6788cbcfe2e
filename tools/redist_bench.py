#!/usr/bin/env python3
"""redist_bench.py -- what the redistribution of ambiguous reads (UTREE_REDISTRIBUTE, utree_redist_*) costs on one GPU, on bench.py's
synthetic database (default: config 2, 1.217e9 32-mers = 8 GB) and launches of 16 M x 150 bp reads:

  batch step        classify + vote of one launch, HIP events around warmed-up launches: utree_classify_batch (the code path of a search
                    without the variable) against utree_redist_classify_batch, the two alternating; the first add into an empty handle
                    (every set is inserted) apart from the later ones (every set is found)
  solve             seconds of the passes over the sets of all the batches added, and how many sets and passes those were
  file -> file      reads/s of the whole search with and without the redistribution file, the two alternating

Prints one JSON line; --out also writes it to a file (profiles/redist_bench.json).  Needs the GPU: there is no fallback.
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solve-batches", type=int, default=3, help="distinct batches whose sets the timed solve iterates over")
    ap.add_argument("--e2e-reads", type=int, default=16_000_000, help="reads of the file -> file leg (0: skip it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from utree_amd import lib as ulib
    from utree_amd import synth
    from utree_amd.search import CtrDB, search_gg
    assert torch.cuda.is_available(), "redist_bench.py needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"nodes": args.nodes, "batch_reads": args.batch_reads, "read_len": args.read_len, "gpu": torch.cuda.get_device_name(0)}
    sdb = synth.make_db(dev, args.nodes, W=8, keep_raw=bool(args.e2e_reads))

    def say(what):
        print("[redist_bench] " + what, file=sys.stderr, flush=True)

    say("database built (%d nodes)" % sdb.n_nodes)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return time.time() - t0, out

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    reads = synth.make_reads(sdb, args.batch_reads, args.read_len)
    total, mx = args.batch_reads * args.read_len, args.read_len
    # one workspace for every launch (sized for both strands), so that no timed call allocates
    ws = torch.empty(sdb.tree.workspace_bytes(args.batch_reads, total, mx, True), dtype=torch.uint8, device=dev)
    out = torch.empty((args.batch_reads, 6), dtype=torch.int32, device=dev)
    kw = dict(total_bases=total, max_len=mx, out=out, workspace=ws)
    res["create_seconds"], rd = timed(lambda: sdb.tree.redistribution())
    for rc in (False, True):
        sdb.tree.classify(reads.bases, reads.off, reads.length, rc=rc, **kw)                  # warm-up: code objects
        torch.cuda.synchronize()
        rd.reset()
        first = event_ms(lambda: rd.classify(reads.bases, reads.off, reads.length, rc=rc, **kw))
        plain, withr = [], []
        for rep in range(args.repeats):
            plain.append(event_ms(lambda: sdb.tree.classify(reads.bases, reads.off, reads.length, rc=rc, **kw)))
            withr.append(event_ms(lambda: rd.classify(reads.bases, reads.off, reads.length, rc=rc, **kw)))
        sdb.tree.poll()
        key = "batch_step_rc" if rc else "batch_step_forward"
        mp, mw = float(np.median(plain)), float(np.median(withr))
        res[key] = {"plain_ms": plain, "with_handle_ms": withr, "first_add_into_empty_handle_ms": first,
                    "median_plain_ms": mp, "median_with_handle_ms": mw, "ratio": mw / mp}
        say("%s: plain %s ms, with a handle %s ms (first %0.2f ms): x%.4f" % (key, plain, withr, first, mw / mp))
    # the sets of a run of distinct batches, solved
    rd.reset()
    for b in range(args.solve_batches):
        r = reads if b == 0 else synth.make_reads(sdb, args.batch_reads, args.read_len, seed=synth.READ_SEED + b)
        rd.classify(r.bases, r.off, r.length, rc=False, **kw)
        torch.cuda.synchronize()
        del r
    read_s, (ms, n_reads, n_classified) = timed(rd.sets)
    solves = []
    for rep in range(3):
        s, (e, passes, ambiguous) = timed(lambda: rd.solve(100))
        solves.append(s)
    one_pass, _ = timed(lambda: rd.solve(1))
    res["solve"] = {"reads": n_reads, "classified": n_classified, "ambiguous": ambiguous, "distinct_sets": len(ms),
                    "distinct_multi_label_sets": sum(1 for k in ms if len(k) > 1), "largest_set": max(map(len, ms)) if ms else 0,
                    "passes": passes, "seconds": solves, "seconds_one_pass": one_pass, "read_back_seconds": read_s,
                    "labels_assigned": int((e["assigned"] > 0).sum())}
    say("solve: %s" % res["solve"])
    del ms
    rd.close()
    del out, ws, kw

    if args.e2e_reads:
        need = 12 * 2**30 + 200 * args.e2e_reads
        base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * need else None
        d = tempfile.mkdtemp(prefix="utree_redbench_", dir=base)
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
            db = CtrDB.open(ctr_path)
            import ctypes as C
            arr = (C.c_void_p * 1)(sdb.tree._h)
            ulib.check(ulib.load().utree_search_prepare(db._h, arr, 1, 0), "utree_search_prepare")
            code, st = search_gg(db, [sdb.tree], fa, os.path.join(d, "warm.txt"))             # warm-up
            ulib.check(code, "utree_search_file")
            plain, withr = [], []
            for rep in range(3):
                for lst, redp in ((plain, None), (withr, os.path.join(d, "redist.tsv"))):
                    outp = os.path.join(d, "out.txt")
                    t0 = time.time()
                    code, st = search_gg(db, [sdb.tree], fa, outp, threads=16, redistribute=redp)
                    wall = time.time() - t0
                    ulib.check(code, "utree_search_file_redistribute" if redp else "utree_search_file")
                    lst.append({"wall_seconds": wall, "reads_per_second": st.n_reads / wall})
                    say("file -> file %s: %.3f s" % ("with redistribution" if redp else "plain", wall))
                    os.unlink(outp)
            with open(os.path.join(d, "redist.tsv"), "rb") as f:
                res["file_header"] = f.readline().decode().strip()
            res["file_to_file"] = {"reads": args.e2e_reads, "plain": plain, "with_redistribution": withr,
                                   "note": "with_redistribution includes creating the handle, the passes and writing the file"}
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
