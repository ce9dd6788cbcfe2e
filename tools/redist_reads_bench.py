#!/usr/bin/env python3
"""redist_reads_bench.py -- what each read's redistributed label (UTREE_REDISTRIBUTE_READS, utree_redist_classify_batch_keys /
utree_redist_assign) costs on one GPU, on bench.py's synthetic database (default: config 2, 1.217e9 32-mers = 8 GB) and launches of
16 M x 150 bp reads.  Four figures:

  1 unchanged path    utree_redist_classify_batch of this library against the PARENT commit's library (--parent-so: its libutree_amd.so, built
                      in a sibling directory), each in processes of its own on the same box, the two alternating, HIP events around one
                      warm-up and --repeats timed launches per process.  Gate: this library's median is not above the parent's median by more
                      than the parent's own min-max spread over its runs (the tool exits with 1 otherwise).  Without --parent-so: skipped
  2 key stores        utree_redist_classify_batch_keys against utree_redist_classify_batch in this process, alternating (no gate)
  3 assignment        the first utree_redist_assign after a solve (T_P in place, redist_winner_k over the table, the gather) and the later
                      ones (the gather alone), per 16 M keys
  4 file -> file      reads/s of the whole search with UTREE_REDISTRIBUTE alone (device text pipeline), with it under UTREE_HOST_TEXT=1 (the
                      host pipeline without the report: the middle figure) and with UTREE_REDISTRIBUTE_READS as well (host pipeline, spool,
                      second pass), the three alternating, three runs each, outputs and tables compared

Prints one JSON line; --out also writes it to a file (profiles/redist_reads_bench.json), after every figure.  Needs the GPU: there is no
fallback.
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("utree_redist_classify_batch_keys", "utree_redist_assign", "utree_redist_reads_format")


def say(what):
    print("[redist_reads_bench] " + what, file=sys.stderr, flush=True)


def sha_of(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def classify_leg(args):
    """a process of its own: warm-up and timed launches of utree_redist_classify_batch with whatever library UTREE_AMD_SO names"""
    import ctypes as C
    import torch
    from utree_amd import lib as ulib
    probe = C.CDLL(ulib.SO_PATH)
    for name in NEW_SYMBOLS:                         # the parent's library does not have them; this leg does not call them
        if not hasattr(probe, name):
            ulib.SYMBOLS.pop(name, None)
    from utree_amd import synth
    dev = torch.device("cuda:0")
    sdb = synth.make_db(dev, args.nodes, W=8, keep_raw=False)
    n = args.batch_reads
    reads = synth.make_reads(sdb, n, args.read_len)
    total, mx = n * args.read_len, args.read_len
    ws = torch.empty(sdb.tree.workspace_bytes(n, total, mx, False), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 6), dtype=torch.int32, device=dev)
    rd = sdb.tree.redistribution()
    ms = []
    for rep in range(1 + args.repeats):              # the first: warm-up, and every set is inserted; then every set is found
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rd.classify(reads.bases, reads.off, reads.length, rc=False, total_bases=total, max_len=mx, out=out, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    sdb.tree.poll()
    rd.close()
    sdb.tree.close()
    print(json.dumps({"so": ulib.SO_PATH, "warm_up_ms": ms[0], "ms": ms[1:]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_217_000_000)
    ap.add_argument("--batch-reads", type=int, default=16_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-so", default="", help="the parent commit's libutree_amd.so (figure 1; empty: skip it)")
    ap.add_argument("--rounds", type=int, default=2, help="processes per library in figure 1, alternating")
    ap.add_argument("--e2e-reads", type=int, default=16_000_000, help="reads of the file -> file leg (0: skip it)")
    ap.add_argument("--leg", default="", help="internal: 'classify' runs figure 1's measurement in this process")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.leg == "classify":
        return classify_leg(args)
    import numpy as np
    import torch
    from utree_amd import lib as ulib
    from utree_amd import synth
    from utree_amd.search import CtrDB, search_gg
    assert torch.cuda.is_available(), "redist_reads_bench.py needs the MI355X"
    res = {"nodes": args.nodes, "batch_reads": args.batch_reads, "read_len": args.read_len, "gpu": torch.cuda.get_device_name(0)}
    failed = False

    def keep():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    # ---- 1. the path without keys, against the parent commit's library: processes of their own, before this one holds the card's memory ----
    if args.parent_so:
        legs = {"parent": [], "this": []}
        for rnd in range(args.rounds):
            for who, so in (("parent", os.path.abspath(args.parent_so)), ("this", ulib.SO_PATH)):
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", "classify", "--nodes", str(args.nodes), "--batch-reads", str(args.batch_reads),
                       "--read-len", str(args.read_len), "--repeats", str(args.repeats)]
                p = subprocess.run(cmd, env=dict(os.environ, UTREE_AMD_SO=so), capture_output=True, timeout=900)
                if p.returncode:
                    sys.stderr.write(p.stderr.decode(errors="replace")[-2000:])
                    raise SystemExit("figure 1: the %s leg failed with %d" % (who, p.returncode))
                legs[who].append(json.loads(p.stdout.decode().strip().split("\n")[-1]))
                say("classify_batch, %s library: %s ms" % (who, legs[who][-1]["ms"]))
        pm = [x for leg in legs["parent"] for x in leg["ms"]]
        tm = [x for leg in legs["this"] for x in leg["ms"]]
        spread = max(pm) - min(pm)
        ok = float(np.median(tm)) <= float(np.median(pm)) + spread
        res["classify_batch_vs_parent"] = {"parent_ms": pm, "this_ms": tm, "parent_median_ms": float(np.median(pm)), "this_median_ms": float(np.median(tm)),
                                           "parent_min_max_spread_ms": spread, "within_parent_spread": ok,
                                           "note": "utree_redist_classify_batch, %d processes per library alternating, one warm-up and %d timed launches each" % (args.rounds, args.repeats)}
        failed |= not ok
        keep()

    dev = torch.device("cuda:0")
    sdb = synth.make_db(dev, args.nodes, W=8, keep_raw=bool(args.e2e_reads))
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
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    kw = dict(total_bases=total, max_len=mx, out=out, workspace=ws)

    # ---- 2. the key stores ----
    rd = sdb.tree.redistribution()
    rd.classify(reads.bases, reads.off, reads.length, rc=False, keys=keys, **kw)                 # warm-up; every set is inserted
    rd.classify(reads.bases, reads.off, reads.length, rc=False, **kw)
    torch.cuda.synchronize()
    plain, withk = [], []
    for rep in range(args.repeats):
        plain.append(event_ms(lambda: rd.classify(reads.bases, reads.off, reads.length, rc=False, **kw)))
        withk.append(event_ms(lambda: rd.classify(reads.bases, reads.off, reads.length, rc=False, keys=keys, **kw)))
    sdb.tree.poll()
    mp, mk = float(np.median(plain)), float(np.median(withk))
    res["keys_vs_no_keys"] = {"classify_batch_ms": plain, "classify_batch_keys_ms": withk, "median_classify_batch_ms": mp,
                              "median_classify_batch_keys_ms": mk, "key_stores_ms": mk - mp, "ratio": mk / mp}
    say("keys: without %s ms, with %s ms: x%.4f" % (plain, withk, mk / mp))
    keep()

    # ---- 3. the assignment of one launch's keys ----
    firsts, later = [], []
    for rep in range(3):
        e, passes, ambiguous = rd.solve(100)
        torch.cuda.synchronize()
        t0 = time.time()
        label, ncand = rd.assign(keys)                                                         # T_P in place, the slots' winners, the gather
        torch.cuda.synchronize()
        firsts.append(1e3 * (time.time() - t0))
    for rep in range(args.repeats):
        later.append(event_ms(lambda: rd.assign(keys)))
    ms_sets, n_reads, n_classified = rd.sets()
    hist = torch.bincount(label[label != -1].long())
    assert int(hist.sum().item()) * (2 + 2 * args.repeats) == int(e["assigned"].sum()), "the assigned reads are not the solve's"
    res["assign"] = {"keys": n, "first_after_a_solve_wall_ms": firsts, "later_ms": later, "median_first_ms": float(np.median(firsts)),
                     "median_later_ms": float(np.median(later)), "winner_pass_and_tally_ms": float(np.median(firsts) - np.median(later)),
                     "table_slots": 1 << 22, "distinct_multi_label_sets": sum(1 for k in ms_sets if len(k) > 1), "passes": passes,
                     "reads_with_a_label": int(hist.sum().item()), "reads_with_several_candidates": int((ncand > 1).sum().item())}
    say("assign: first after a solve %s ms (wall), later %s ms" % (firsts, later))
    del ms_sets, label, ncand, hist
    rd.close()
    del out, ws, kw, keys
    keep()

    # ---- 4. file -> file ----
    if args.e2e_reads:
        need = 12 * 2**30 + 400 * args.e2e_reads
        base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * need else None
        d = tempfile.mkdtemp(prefix="utree_rrbench_", dir=base)
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
                    m = min(args.batch_reads, args.e2e_reads - done)
                    r = reads if b == 0 else synth.make_reads(sdb, args.batch_reads, args.read_len, seed=synth.READ_SEED + b)
                    if m < args.batch_reads:
                        r = synth.SynthReads(bases=r.bases[: m * args.read_len], off=r.off[:m], length=r.length[:m], n=m, read_len=args.read_len)
                    synth.fasta_tensor(r, done).cpu().numpy().tofile(f)
                    done += m
                    b += 1
                    del r
            del reads
            torch.cuda.empty_cache()
            db = CtrDB.open(ctr_path)
            import ctypes as C
            arr = (C.c_void_p * 1)(sdb.tree._h)
            ulib.check(ulib.load().utree_search_prepare(db._h, arr, 1, 0), "utree_search_prepare")
            code, st = search_gg(db, [sdb.tree], fa, os.path.join(d, "warm.txt"))             # warm-up
            ulib.check(code, "utree_search_run")
            os.unlink(os.path.join(d, "warm.txt"))
            modes = (("redistribute_device_pipeline", False, False), ("redistribute_host_pipeline", True, False), ("redistribute_and_reads", False, True))
            runs = {m[0]: [] for m in modes}
            outs, tables = set(), set()
            q = os.path.join(d, "reads.tsv")
            for rep in range(3):
                for tag, host, with_reads in modes:
                    outp, redp = os.path.join(d, "out.txt"), os.path.join(d, "redist.tsv")
                    if host:
                        os.environ["UTREE_HOST_TEXT"] = "1"
                    t0 = time.time()
                    code, st = search_gg(db, [sdb.tree], fa, outp, threads=16, redistribute=redp, redistribute_reads=q if with_reads else None)
                    wall = time.time() - t0
                    os.environ.pop("UTREE_HOST_TEXT", None)
                    ulib.check(code, "utree_search_run (%s)" % tag)
                    runs[tag].append({"wall_seconds": wall, "reads_per_second": st.n_reads / wall, "pipeline": st.pipeline, "search_seconds": st.seconds_total})
                    say("file -> file %s: %.3f s (search %.3f s)" % (tag, wall, st.seconds_total))
                    outs.add(sha_of(outp)); tables.add(sha_of(redp))
                    os.unlink(outp); os.unlink(redp)
            med = {tag: float(np.median([r["reads_per_second"] for r in runs[tag]])) for tag in runs}
            wall = {tag: float(np.median([r["wall_seconds"] for r in runs[tag]])) for tag in runs}
            with open(q, "rb") as f:
                first_line = f.readline().decode(errors="replace").rstrip("\n")
            res["file_to_file"] = {"reads": args.e2e_reads, "runs": runs, "median_reads_per_second": med, "median_wall_seconds": wall,
                                   "pipeline_change_seconds": wall["redistribute_host_pipeline"] - wall["redistribute_device_pipeline"],
                                   "report_itself_seconds": wall["redistribute_and_reads"] - wall["redistribute_host_pipeline"],
                                   "outputs_identical": len(outs) == 1, "tables_identical": len(tables) == 1,
                                   "reads_file_bytes": os.path.getsize(q), "reads_file_first_line": first_line,
                                   "spool_removed": not os.path.exists(q + ".spool"),
                                   "note": "every run writes the redistribution's table; redistribute_and_reads also spools the keys, assigns them after the "
                                           "solve and writes the reads file"}
            failed |= len(outs) != 1 or len(tables) != 1
        finally:
            shutil.rmtree(d, ignore_errors=True)
    sdb.tree.close()
    print(json.dumps(res))
    keep()
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
