#!/usr/bin/env python3
"""samples_bench.py -- what the per-sample taxon table (UTREE_SAMPLE_TABLE, utree_samples_*) costs on one GPU, on bench.py's synthetic
database (bench.py's default, configs[1]: 1.217e9 32-mers = 8 GB) and launches of 16 M x 150 bp reads named <sample>_<n>:

  add               utree_samples_add against utree_profile_add on the same records in the same process, and against the classify step, HIP
                    events around one warm-up and three timed launches each; names of 96 samples in blocks (a combined file is a
                    concatenation), 96 shuffled and 10 000 shuffled (what the predecessor shortcut is worth)
  file -> file      reads/s of the whole search with and without the table file, the two alternating, three runs each, outputs compared

Prints one JSON line; --out also writes it to a file (profiles/samples_bench.json).  Needs the GPU: there is no fallback.
"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAME_W = 15                                      # S%05d_%08d


def names_tensor(torch, sample, dev):
    """[n, NAME_W] uint8: read i of sample[i] is named S<sample, 5 digits>_<i, 8 digits>"""
    n = sample.numel()
    t = torch.empty((n, NAME_W), dtype=torch.uint8, device=dev)
    t[:, 0] = ord("S")
    t[:, 6] = ord("_")
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    for d in range(5):
        t[:, 5 - d] = ((sample // (10 ** d)) % 10 + ord("0")).to(torch.uint8)
    for d in range(8):
        t[:, 14 - d] = ((idx // (10 ** d)) % 10 + ord("0")).to(torch.uint8)
    return t


def sample_of(torch, n, n_samples, shuffled, dev):
    if shuffled:
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        return torch.randint(0, n_samples, (n,), generator=g, device=dev, dtype=torch.int64)
    return torch.arange(n, dtype=torch.int64, device=dev) * n_samples // n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_217_000_000, help="nodes of the synthetic database (bench.py's default, configs[1])")
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
    assert torch.cuda.is_available(), "samples_bench.py needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"nodes": args.nodes, "batch_reads": args.batch_reads, "read_len": args.read_len, "gpu": torch.cuda.get_device_name(0)}
    sdb = synth.make_db(dev, args.nodes, W=8, keep_raw=bool(args.e2e_reads))

    def say(what):
        print("[samples_bench] " + what, file=sys.stderr, flush=True)

    say("database built (%d nodes)" % sdb.n_nodes)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    n = args.batch_reads
    reads = synth.make_reads(sdb, n, args.read_len)
    total, mx = n * args.read_len, args.read_len
    ws = torch.empty(sdb.tree.workspace_bytes(n, total, mx, False), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 6), dtype=torch.int32, device=dev)
    kw = dict(total_bases=total, max_len=mx, out=out, workspace=ws)
    sdb.tree.classify(reads.bases, reads.off, reads.length, rc=False, **kw)                      # warm-up
    torch.cuda.synchronize()
    classify = [event_ms(lambda: sdb.tree.classify(reads.bases, reads.off, reads.length, rc=False, **kw)) for _ in range(args.repeats)]
    sdb.tree.poll()
    prof = sdb.tree.profile()
    prof.add(out)
    torch.cuda.synchronize()
    profile = [event_ms(lambda: prof.add(out)) for _ in range(args.repeats)]
    prof.close()
    res["classify_ms"], res["profile_add_ms"] = classify, profile
    say("classify %s ms, profile add %s ms" % (classify, profile))
    name_off = (torch.arange(n, dtype=torch.int64, device=dev) * NAME_W).to(torch.int32)
    name_len = torch.full((n,), NAME_W, dtype=torch.int32, device=dev)
    res["samples_add"] = {}
    for tag, n_samples, shuffled in (("96_blocks", 96, False), ("96_shuffled", 96, True), ("10000_shuffled", 10000, True)):
        text = names_tensor(torch, sample_of(torch, n, n_samples, shuffled, dev), dev).view(-1)
        smp = sdb.tree.samples(1 << 16, 1 << 25)                                                  # (10 000 samples: millions of cells)
        first = event_ms(lambda: smp.add(text, name_off, name_len, out))                          # into an empty handle: every id is claimed
        ms = [event_ms(lambda: smp.add(text, name_off, name_len, out)) for _ in range(args.repeats)]
        rb = smp.read()
        assert rb.n_reads == (1 + args.repeats) * n and len(rb.ids) == n_samples and int(rb.reads.sum()) == rb.n_reads
        res["samples_add"][tag] = {"first_add_into_empty_handle_ms": first, "ms": ms, "median_ms": float(np.median(ms)),
                                   "over_profile_add": float(np.median(ms) / np.median(profile)),
                                   "share_of_classify": float(np.median(ms) / np.median(classify)), "cells": int(len(rb.cells))}
        say("%s: first %.3f ms, then %s ms" % (tag, first, ms))
        smp.close()
        del text
    del out, ws, kw, name_off, name_len

    if args.e2e_reads:
        need = 12 * 2**30 + 200 * args.e2e_reads
        base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * need else None
        d = tempfile.mkdtemp(prefix="utree_smpbench_", dir=base)
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
            L = args.read_len
            with open(fa, "wb") as f:                                                           # 96 samples in blocks: a concatenation of samples
                m = min(args.e2e_reads, n)
                assert m == args.e2e_reads, "the file -> file leg takes at most one batch of reads"
                rec = torch.empty((m, 1 + NAME_W + 1 + L + 1), dtype=torch.uint8, device=dev)
                rec[:, 0] = ord(">")
                rec[:, 1:1 + NAME_W] = names_tensor(torch, sample_of(torch, m, 96, False, dev), dev)
                rec[:, 1 + NAME_W] = ord("\n")
                rec[:, 2 + NAME_W:2 + NAME_W + L] = reads.bases.view(n, L)[:m]
                rec[:, 2 + NAME_W + L] = ord("\n")
                rec.view(-1).cpu().numpy().tofile(f)
                del rec
            del reads
            torch.cuda.empty_cache()
            db = CtrDB.open(ctr_path)
            import ctypes as C
            arr = (C.c_void_p * 1)(sdb.tree._h)
            ulib.check(ulib.load().utree_search_prepare(db._h, arr, 1, 0), "utree_search_prepare")
            code, st = search_gg(db, [sdb.tree], fa, os.path.join(d, "warm.txt"))             # warm-up
            ulib.check(code, "utree_search_file")
            plain, withs, sums = [], [], set()
            for rep in range(3):
                for lst, tab in ((plain, None), (withs, os.path.join(d, "samples.tsv"))):
                    outp = os.path.join(d, "out.txt")
                    t0 = time.time()
                    code, st = search_gg(db, [sdb.tree], fa, outp, threads=16, samples=tab)
                    wall = time.time() - t0
                    ulib.check(code, "utree_search_file_samples" if tab else "utree_search_file")
                    lst.append({"wall_seconds": wall, "reads_per_second": st.n_reads / wall, "pipeline": st.pipeline})
                    say("file -> file %s: %.3f s" % ("with the table" if tab else "plain", wall))
                    h = hashlib.sha256()
                    with open(outp, "rb") as f:
                        for blk in iter(lambda: f.read(1 << 24), b""):
                            h.update(blk)
                    sums.add(h.hexdigest())
                    os.unlink(outp)
            with open(os.path.join(d, "samples.tsv"), "rb") as f:
                res["file_header"] = f.readline().decode().strip()
            res["file_to_file"] = {"reads": args.e2e_reads, "plain": plain, "with_table": withs, "outputs_identical": len(sums) == 1,
                                   "note": "with_table includes creating the handle, the read-back and writing the file"}
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
