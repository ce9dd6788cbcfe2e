#!/usr/bin/env python3
"""hitmap_bench.py -- what the per-query k-mer hit map (UTREE_HITMAP, utree_hitmap_batch) costs on one GPU, on bench.py's synthetic
database (default: config 2, 1.217e9 32-mers = 8 GB) and launches of 16 M x 150 bp reads:

  hitmap_batch      ms forward and with RC, HIP events around warmed-up launches; runs per read; the workspace
  classify / coverage_add   the same batch in the same process, for scale
  file -> file      wall seconds of the whole search with and without the hit-map file, the two alternating

Prints one JSON line; --out also writes it to a file (profiles/hitmap_bench.json).  Needs the GPU: there is no fallback.
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
    from utree_amd.search import CtrDB, search_gg
    assert torch.cuda.is_available(), "hitmap_bench.py needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"nodes": args.nodes, "batch_reads": args.batch_reads, "read_len": args.read_len, "gpu": torch.cuda.get_device_name(0)}
    sdb = synth.make_db(dev, args.nodes, W=8, keep_raw=True)
    res["image_bytes"] = int(sdb.tree.info.image_bytes)
    res["bucket_bytes"] = int(sdb.tree.info.bucket_bytes)

    def say(what):
        print("[hitmap_bench] " + what, file=sys.stderr, flush=True)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    say("database built (%d nodes)" % sdb.n_nodes)
    reads = synth.make_reads(sdb, args.batch_reads, args.read_len)
    total = args.batch_reads * args.read_len
    t = (reads.bases, reads.off, reads.length)
    for rc in (False, True):
        key = "rc" if rc else "forward"
        need = ulib.load().utree_hitmap_workspace_bytes(sdb.tree._h, args.batch_reads, total, int(rc))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        # the first call sizes the runs (capacity 0: offsets and meta are complete, no run is written), and warms the code objects up
        _, _, meta = sdb.tree.hitmap(*t, rc=rc, capacity=0, total_bases=total, workspace=ws, runs=torch.empty((1, 2), dtype=torch.int32, device=dev))
        assert meta["error"] == 1 or meta["total_runs"] == 0
        cap = meta["total_runs"]
        runs = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev)
        ms = []
        for rep in range(args.repeats):
            ms.append(events(lambda: sdb.tree.hitmap(*t, rc=rc, capacity=cap, total_bases=total, workspace=ws, runs=runs, sync=False)))
        run_off, _, meta = sdb.tree.hitmap(*t, rc=rc, capacity=cap, total_bases=total, workspace=ws, runs=runs)
        assert meta["error"] == 0 and int(run_off[-1].item()) == cap
        hit_windows = int(runs[:, 1][(runs[:, 0] >= 0)].to(torch.int64).sum().item()) if cap else 0       # (miss / invalid read as -1 / -2)
        res["hitmap_" + key] = {"ms": ms, "reads_per_second": [args.batch_reads / (m * 1e-3) for m in ms], "workspace_bytes": need,
                                "total_windows": meta["total_windows"], "total_runs": cap, "runs_per_read": cap / args.batch_reads,
                                "hit_windows": hit_windows}
        say("hitmap %s: %s ms, %.2f runs per read, workspace %.2f GB" % (key, ms, cap / args.batch_reads, need / 1e9))
        del ws, runs, run_off
        torch.cuda.empty_cache()
        out = sdb.tree.classify(*t, rc=rc)
        torch.cuda.synchronize()
        res["classify_" + key + "_ms"] = [events(lambda: sdb.tree.classify(*t, rc=rc, out=out)) for rep in range(args.repeats)]
        say("classify %s: %s ms" % (key, res["classify_" + key + "_ms"]))
        del out
    cov = sdb.tree.coverage(sdb.binix.view(torch.uint8), sdb.records)
    for rc in (False, True):
        cov.add(*t, rc=rc)
        torch.cuda.synchronize()
        res["coverage_add_" + ("rc" if rc else "forward") + "_ms"] = [events(lambda: cov.add(*t, rc=rc)) for rep in range(args.repeats)]
    say("coverage_add: %s / %s ms" % (res["coverage_add_forward_ms"], res["coverage_add_rc_ms"]))
    cov.close()

    if args.e2e_reads:
        need = 12 * 2**30 + 400 * args.e2e_reads
        base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * need else None
        d = tempfile.mkdtemp(prefix="utree_hmbench_", dir=base)
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
            del reads, t
            torch.cuda.empty_cache()
            db = CtrDB.open(ctr_path)
            import ctypes as C
            arr = (C.c_void_p * 1)(sdb.tree._h)
            ulib.check(ulib.load().utree_search_prepare(db._h, arr, 1, 0), "utree_search_prepare")
            code, st = search_gg(db, [sdb.tree], fa, os.path.join(d, "warm.txt"))             # warm-up
            ulib.check(code, "utree_search_file")
            plain, withm = [], []
            for rep in range(args.repeats):
                for lst, hm in ((plain, None), (withm, os.path.join(d, "map.tsv"))):
                    outp = os.path.join(d, "out.txt")
                    t0 = time.time()
                    code, st = search_gg(db, [sdb.tree], fa, outp, threads=16, hitmap=hm)
                    wall = time.time() - t0
                    ulib.check(code, "utree_search_file_hitmap" if hm else "utree_search_file")
                    lst.append({"wall_seconds": wall, "reads_per_second": st.n_reads / wall, "pipeline": int(st.pipeline)})
                    if hm:
                        lst[-1]["hitmap_file_bytes"] = os.path.getsize(hm)
                        os.unlink(hm)
                    say("file -> file %s: %.3f s" % ("with the hit map" if hm else "plain", wall))
                    os.unlink(outp)
            res["file_to_file"] = {"reads": args.e2e_reads, "plain": plain, "with_hitmap": withm,
                                   "note": "plain runs on the device text pipeline, with_hitmap on the host-framing pipeline (pipeline 0) and writes one line per read"}
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
