#!/usr/bin/env python3
"""pairs_bench.py -- what paired-end reads cost on one GPU, on bench.py's synthetic database (default: config 2, 1.217e9 32-mers) and
16 M pairs of 150 + 150 bp:

  join            utree_pairs_join, HIP events around warmed-up launches; next to it, in the same run, a device-to-device hipMemcpyAsync
                  (torch's copy_ of a contiguous tensor) of the same byte count (the yardstick: the join reads and writes every byte once, as the copy does) and
                  utree_classify_batch on the joined batch (what the join sits in front of); the join as a share of each
  join_tiny       the same launch over pairs of two 1-byte mates: ns per joined byte against the 150 bp figure
  file -> file    the paired search over two files against the host pipeline (UTREE_HOST_TEXT=1) on the pre-joined single file of the same
                  pairs, the two alternating, each in a worker process of its own that keeps the database resident.  --baseline-root names
                  a built checkout whose library runs the baseline (the parent commit); without it this checkout's does

Prints one JSON line; --out also writes it to a file (profiles/pairs_bench.json).  Needs the GPU: there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def say(what):
    print("[pairs_bench] " + what, file=sys.stderr, flush=True)


def worker(root):
    """one line of JSON in, one out: {"reads", "mates" (or null), "out"} -> wall seconds and the search's stats.  The first line names the .ctr."""
    sys.path.insert(0, root)
    from utree_amd import lib as ulib
    from utree_amd.search import CtrDB, DeviceTree, search_gg
    ctr = json.loads(sys.stdin.readline())["ctr"]
    db = CtrDB.open(ctr)
    tree = DeviceTree.upload(db, 0)
    arr = (C.c_void_p * 1)(tree._h)
    ulib.check(ulib.load().utree_search_prepare(db._h, arr, 1, 0), "utree_search_prepare")
    print(json.dumps({"ready": True, "library": ulib.SO_PATH}), flush=True)
    for line in sys.stdin:
        job = json.loads(line)
        kw = {"mates": job["mates"]} if job.get("mates") else {}
        t0 = time.time()
        code, st = search_gg(db, [tree], job["reads"], job["out"], threads=16, **kw)
        wall = time.time() - t0
        ulib.check(code, "search")
        print(json.dumps({"wall_seconds": wall, "n_reads": int(st.n_reads), "good_finds": int(st.good_finds), "pipeline": int(st.pipeline),
                          "seconds_read": st.seconds_read, "seconds_frame": st.seconds_frame, "seconds_gpu": st.seconds_classify_format,
                          "seconds_format": st.seconds_d2h, "seconds_write": st.seconds_write}), flush=True)
    tree.close()


class Worker:
    def __init__(self, root, ctr, env):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--root", root], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, env=env, text=True)
        self.p.stdin.write(json.dumps({"ctr": ctr}) + "\n")
        self.p.stdin.flush()
        self.hello = self._read()

    def _read(self):
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError("a worker ended (exit %s)" % self.p.wait())
            if line.startswith("{"):                                              # (the search's own progress lines go to stdout too)
                return json.loads(line)

    def run(self, **job):
        self.p.stdin.write(json.dumps(job) + "\n")
        self.p.stdin.flush()
        return self._read()

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def med_spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_217_000_000)
    ap.add_argument("--pairs", type=int, default=16_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--e2e-pairs", type=int, default=16_000_000, help="pairs of the file -> file leg (0: skip it)")
    ap.add_argument("--baseline-root", default="", help="a built checkout of the parent commit: its library runs the file leg's baseline")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE_ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.root)
    sys.path.insert(0, HERE_ROOT)
    import numpy as np
    import torch
    from utree_amd import lib as ulib
    from utree_amd import synth
    assert torch.cuda.is_available(), "pairs_bench.py needs the MI355X"
    assert args.repeats >= 3
    dev = torch.device("cuda:0")
    n, L = args.pairs, args.read_len
    res = {"nodes": args.nodes, "pairs": n, "read_len": L, "gpu": torch.cuda.get_device_name(0)}
    sdb = synth.make_db(dev, args.nodes, W=8, keep_raw=True)
    say("database built (%d nodes)" % sdb.n_nodes)
    lib = ulib.load()
    stream = torch.cuda.current_stream()

    def events(fn, repeats):
        fn()                                                                       # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    def join_fn(b1, o1, l1, b2, o2, l2, joined, joff, jlen, meta):
        k = o1.numel()
        return lambda: ulib.check(lib.utree_pairs_join(sdb.tree._h, b1.data_ptr(), o1.data_ptr(), l1.data_ptr(), b2.data_ptr(), o2.data_ptr(),
                                                       l2.data_ptr(), k, joined.data_ptr(), joined.numel(), joff.data_ptr(), jlen.data_ptr(),
                                                       meta.data_ptr(), stream.cuda_stream), "utree_pairs_join")

    m1 = synth.make_reads(sdb, n, L)
    m2 = synth.make_reads(sdb, n, L, seed=synth.READ_SEED + 1)
    total = 2 * n * L + n
    joined = torch.empty(total, dtype=torch.uint8, device=dev)
    joff = torch.empty(n, dtype=torch.int64, device=dev)
    jlen = torch.empty(n, dtype=torch.int32, device=dev)
    meta = torch.zeros(2, dtype=torch.int64, device=dev)
    ms_join = events(join_fn(m1.bases, m1.off, m1.length, m2.bases, m2.off, m2.length, joined, joff, jlen, meta), args.repeats)
    pm = ulib.PairsMeta.from_buffer_copy(meta.cpu().numpy().tobytes())
    assert pm.error == 0 and pm.total_bases == total and pm.max_len == 2 * L + 1
    v = joined.view(n, 2 * L + 1)
    assert torch.equal(v[:, :L], m1.bases.view(n, L)) and torch.equal(v[:, L + 1:], m2.bases.view(n, L)) and bool((v[:, L] == 0x4E).all())
    del v
    src = torch.empty(total, dtype=torch.uint8, device=dev)
    ms_copy = events(lambda: joined.copy_(src), args.repeats)     # contiguous uint8 on one device: torch issues hipMemcpyAsync, device to device
    del src
    ms_join2 = events(join_fn(m1.bases, m1.off, m1.length, m2.bases, m2.off, m2.length, joined, joff, jlen, meta), args.repeats)   # (the copy overwrote it)
    res["join"] = {"joined_bytes": total, "ms": med_spread(ms_join + ms_join2), "memcpy_d2d_ms": med_spread(ms_copy)}
    say("join %s ms, memcpy of %d bytes %s ms" % (ms_join + ms_join2, total, ms_copy))
    out = None
    for rc in (False, True):
        out = sdb.tree.classify(joined, joff, jlen, rc=rc, total_bases=total, max_len=2 * L + 1, out=out)
        ms_cl = events(lambda: sdb.tree.classify(joined, joff, jlen, rc=rc, total_bases=total, max_len=2 * L + 1, out=out), args.repeats)
        sdb.tree.poll()
        res["classify_joined_rc" if rc else "classify_joined_forward"] = {"ms": med_spread(ms_cl), "kernel": sdb.tree.kernel_name(),
                                                                            "classified": int((out[:, 2] != 0).sum())}
        say("classify on the joined batch, rc=%d: %s ms (%s)" % (rc, ms_cl, sdb.tree.kernel_name()))
    j = res["join"]["ms"]["median"]
    res["join_share"] = {"of_memcpy_d2d": j / res["join"]["memcpy_d2d_ms"]["median"],
                         "of_classify_forward": j / res["classify_joined_forward"]["ms"]["median"],
                         "of_classify_rc": j / res["classify_joined_rc"]["ms"]["median"],
                         "ns_per_joined_byte": 1e6 * j / total,
                         "effective_GBps_read_plus_write": 2 * total / (j * 1e-3) / 1e9}
    del out
    # pairs of two one-byte mates: three joined bytes, 24 bytes of offsets and lengths read and 12 written per pair
    nt = n
    one = torch.ones(nt, dtype=torch.int32, device=dev)
    o1 = torch.arange(nt, dtype=torch.int64, device=dev)
    tj, toff, tlen = torch.empty(3 * nt, dtype=torch.uint8, device=dev), torch.empty(nt, dtype=torch.int64, device=dev), torch.empty(nt, dtype=torch.int32, device=dev)
    ms_tiny = events(join_fn(m1.bases, o1, one, m2.bases, o1, one, tj, toff, tlen, meta), args.repeats)
    res["join_tiny"] = {"pairs": nt, "joined_bytes": 3 * nt, "ms": med_spread(ms_tiny), "ns_per_joined_byte": 1e6 * statistics.median(ms_tiny) / (3 * nt)}
    say("join of %d pairs of 1 + 1 bytes: %s ms" % (nt, ms_tiny))
    del tj, toff, tlen, one, o1, joined, joff, jlen

    if args.e2e_pairs:
        ne = args.e2e_pairs
        need = 12 * 2**30 + 1300 * ne
        base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * need else None
        d = tempfile.mkdtemp(prefix="utree_pairsbench_", dir=base)
        workers = []
        try:
            ctr_path = os.path.join(d, "db.ctr")
            records = sdb.records.cpu().numpy()
            with open(ctr_path, "wb") as f:
                f.write(np.array([sdb.W, 0, 2, sdb.n_nodes], dtype="<u8").tobytes())
                f.write(sdb.binix.cpu().numpy().view(np.uint32).tobytes())
                for lo in range(0, records.size, 1 << 30):
                    f.write(records[lo:lo + (1 << 30)].tobytes())
                f.write(sdb.label_text)
            del records
            r1, r2, jf = (os.path.join(d, x) for x in ("r1.fa", "r2.fa", "joined.fa"))
            step = 4_000_000
            with open(r1, "wb") as f1, open(r2, "wb") as f2, open(jf, "wb") as fj:
                for lo in range(0, ne, step):
                    k = min(step, ne - lo)
                    a = synth.make_reads(sdb, k, L, seed=synth.READ_SEED + 10 + lo // step)
                    b = synth.make_reads(sdb, k, L, seed=synth.READ_SEED + 5000 + lo // step)
                    both = torch.cat([a.bases.view(k, L), torch.full((k, 1), 0x4E, dtype=torch.uint8, device=dev), b.bases.view(k, L)], dim=1).contiguous()
                    jr = synth.SynthReads(bases=both.view(-1), off=torch.arange(k, dtype=torch.int64, device=dev) * (2 * L + 1),
                                          length=torch.full((k,), 2 * L + 1, dtype=torch.int32, device=dev), n=k, read_len=2 * L + 1)
                    synth.fasta_tensor(a, lo).cpu().numpy().tofile(f1)
                    synth.fasta_tensor(b, lo).cpu().numpy().tofile(f2)
                    synth.fasta_tensor(jr, lo).cpu().numpy().tofile(fj)
                    del a, b, both, jr
            sizes = {os.path.basename(p): os.path.getsize(p) for p in (r1, r2, jf)}
            say("files written: %s" % sizes)
            del m1, m2
            sdb.tree.close()
            torch.cuda.empty_cache()
            env = dict(os.environ)
            for v in ("UTREE_HOST_TEXT", "UTREE_CHUNK_BYTES", "UTREE_MATES", "UTREE_INTERLEAVED"):
                env.pop(v, None)
            broot = os.path.abspath(args.baseline_root) if args.baseline_root else HERE_ROOT
            wp = Worker(HERE_ROOT, ctr_path, env)
            wb = Worker(broot, ctr_path, dict(env, UTREE_HOST_TEXT="1"))
            workers = [wp, wb]
            legs = {"paired": [], "joined_host_pipeline": []}
            for rep in range(args.repeats + 1):                                   # the first round warms both up
                for key, w, job in (("paired", wp, dict(reads=r1, mates=r2)), ("joined_host_pipeline", wb, dict(reads=jf, mates=None))):
                    outp = os.path.join(d, key + ".txt")
                    r = w.run(out=outp, **job)
                    r["out_bytes"] = os.path.getsize(outp)
                    assert r["n_reads"] == ne and r["pipeline"] == 0
                    if rep:
                        legs[key].append(r)
                    say("file -> file %s%s: %.3f s (read %.2f frame %.2f gpu %.2f format %.2f write %.2f)" % (
                        key, "" if rep else " (warm-up)", r["wall_seconds"], r["seconds_read"], r["seconds_frame"], r["seconds_gpu"],
                        r["seconds_format"], r["seconds_write"]))
            same = open(os.path.join(d, "paired.txt"), "rb").read() == open(os.path.join(d, "joined_host_pipeline.txt"), "rb").read()
            assert same, "the paired search and the search of the joined file wrote different outputs"
            med = {k: statistics.median(x["wall_seconds"] for x in v) for k, v in legs.items()}
            stage = {k: {s: statistics.median(x[s] for x in v) for s in ("seconds_read", "seconds_frame", "seconds_gpu", "seconds_format", "seconds_write")}
                     for k, v in legs.items()}
            res["file_to_file"] = {"pairs": ne, "input_bytes": sizes, "baseline_library": wb.hello["library"], "paired_library": wp.hello["library"],
                                   "runs": legs, "median_wall_seconds": med, "median_stage_seconds": stage,
                                   "paired_over_joined": med["paired"] / med["joined_host_pipeline"], "outputs_identical": same,
                                   "pairs_per_second": {k: ne / s for k, s in med.items()}}
        finally:
            for w in workers:
                w.close()
            shutil.rmtree(d, ignore_errors=True)
    else:
        sdb.tree.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
