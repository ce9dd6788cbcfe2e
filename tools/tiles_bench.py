#!/usr/bin/env python3
"""tiles_bench.py -- utree-tiles against what a user does today, on one GPU, file to file, on bench.py's synthetic database:

  tiles        utree_tiles_file on contigs.fa (default 2 000 x 1 Mb drawn from the database), W = 1000, S = 500
  pre-split    this same library's GG search (utree_search_run, what xtree-searchGG calls) on split.fa, the FASTA of the same tiles cut
               by a script: one two-line record ><name>:<start>-<end> per tile, W/S times the bases

Both run in this process on the same resident image, alternating, --repeats times each after un-timed warm-ups of both (a small file, then the timed files themselves); wall
seconds around the call, which returns with its files written.  The two per-tile outputs must be byte-identical (SHA-256).  The
expectation under test: tiles is not slower than pre-split by more than the spread (max - min) of pre-split's own runs.  Prints one JSON
line with every time, the medians, tiles/s and the verdict -- "holds" or "refuted"; --out also writes it to a file
(profiles/tiles_bench.json).  Needs the GPU: there is no fallback.
"""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_217_000_000)
    ap.add_argument("--contigs", type=int, default=2000)
    ap.add_argument("--contig-len", type=int, default=1_000_000)
    ap.add_argument("--tile", type=int, default=1000)
    ap.add_argument("--step", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rc", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from utree_amd import lib as ulib
    from utree_amd import synth
    from utree_amd.search import search_gg, tiles_file
    assert torch.cuda.is_available(), "tiles_bench.py needs the MI355X"
    dev = torch.device("cuda:0")
    W, S, L = args.tile, args.step, args.contig_len
    assert 1 <= S <= W <= L
    per = 1 + -(-(L - W) // S)
    res = {"nodes": args.nodes, "contigs": args.contigs, "contig_len": L, "tile_bp": W, "step_bp": S, "rc": args.rc, "tiles": per * args.contigs,
           "gpu": torch.cuda.get_device_name(0)}

    def say(what):
        print("[tiles_bench] " + what, file=sys.stderr, flush=True)

    sdb = synth.make_db(dev, args.nodes, W=8)
    say("database built (%d nodes)" % sdb.n_nodes)
    need = args.contigs * L * (2 + W // S) + (1 << 30)
    base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * need else None
    d = tempfile.mkdtemp(prefix="utree_tilesbench_", dir=base)
    try:
        # contigs.fa, split.fa and, for the warm-ups, the same of the first two contigs
        paths = {k: os.path.join(d, k) for k in ("contigs.fa", "split.fa", "warm_contigs.fa", "warm_split.fa")}
        starts = list(range(0, (per - 1) * S + 1, S))
        files = {k: open(p, "wb") for k, p in paths.items()}
        done, b = 0, 0
        while done < args.contigs:
            n = min(64, args.contigs - done)
            r = synth.make_reads(sdb, n, L, seed=synth.READ_SEED + 7 + b)
            seqs = r.bases.view(n, L).cpu().numpy()
            for i in range(n):
                name, seq = b"r%d" % (done + i), seqs[i].tobytes()
                rec = b">%s\n%s\n" % (name, seq)
                split = b"".join(b">%s:%d-%d\n%s\n" % (name, a + 1, min(a + W, L), seq[a:a + W]) for a in starts)
                files["contigs.fa"].write(rec); files["split.fa"].write(split)
                if done + i < 2:
                    files["warm_contigs.fa"].write(rec); files["warm_split.fa"].write(split)
            done += n
            b += 1
            del r, seqs
        for f in files.values():
            f.close()
        torch.cuda.empty_cache()
        res["contigs_bytes"], res["split_bytes"] = os.path.getsize(paths["contigs.fa"]), os.path.getsize(paths["split.fa"])
        say("files written: contigs %.2f GB, split %.2f GB, %d tiles" % (res["contigs_bytes"] / 1e9, res["split_bytes"] / 1e9, res["tiles"]))

        def run_split(src, out):
            t0 = time.time()
            code, st = search_gg(sdb.ctr, [sdb.tree], src, out, rc=bool(args.rc), threads=16)
            wall = time.time() - t0
            ulib.check(code, "utree_search_run")
            return wall, int(st.n_reads), int(st.good_finds), int(st.pipeline)

        def run_tiles(src, out):
            t0 = time.time()
            code, st = tiles_file(sdb.ctr, sdb.tree, src, out, None, tile_bp=W, step_bp=S, rc=bool(args.rc), threads=16)
            wall = time.time() - t0
            ulib.check(code, "utree_tiles_file")
            return wall, int(st.n_tiles), int(st.classified), float(st.seconds_device), int(st.n_batches)

        o_split, o_tiles = os.path.join(d, "split.txt"), os.path.join(d, "tiles.tsv")
        for src_s, src_t in ((paths["warm_split.fa"], paths["warm_contigs.fa"]), (paths["split.fa"], paths["contigs.fa"])):   # code objects; then the shapes that are timed
            run_split(src_s, o_split)
            run_tiles(src_t, o_tiles)
            assert sha256_file(o_split) == sha256_file(o_tiles), "warm-up: the two per-tile outputs differ"
        split_runs, tiles_runs, hashes = [], [], set()
        for rep in range(args.repeats):
            wall, n, good, pipeline = run_split(paths["split.fa"], o_split)
            assert n == res["tiles"]
            split_runs.append({"wall_seconds": wall, "tiles_per_second": n / wall, "lines": good, "pipeline": pipeline})
            hashes.add(sha256_file(o_split)); os.unlink(o_split)
            say("pre-split %.3f s" % wall)
            wall, n, good, t_dev, nb = run_tiles(paths["contigs.fa"], o_tiles)
            assert n == res["tiles"]
            tiles_runs.append({"wall_seconds": wall, "tiles_per_second": n / wall, "lines": good, "seconds_device": t_dev, "batches": nb})
            hashes.add(sha256_file(o_tiles)); os.unlink(o_tiles)
            say("tiles     %.3f s (device %.3f s)" % (wall, t_dev))
        res["outputs_identical"] = len(hashes) == 1
        res["output_sha256"] = sorted(hashes)
        assert res["outputs_identical"], "the two per-tile outputs differ"
        sw, tw = [r["wall_seconds"] for r in split_runs], [r["wall_seconds"] for r in tiles_runs]
        res["pre_split"], res["tiles_runs"] = split_runs, tiles_runs
        res["pre_split_median_seconds"], res["tiles_median_seconds"] = statistics.median(sw), statistics.median(tw)
        res["pre_split_spread_seconds"] = max(sw) - min(sw)
        res["tiles_per_second_median"] = res["tiles"] / res["tiles_median_seconds"]
        res["pre_split_tiles_per_second_median"] = res["tiles"] / res["pre_split_median_seconds"]
        res["speedup_over_pre_split"] = res["pre_split_median_seconds"] / res["tiles_median_seconds"]
        res["tiles_minus_pre_split_median_seconds"] = res["tiles_median_seconds"] - res["pre_split_median_seconds"]
        res["expectation"] = "tiles_median_seconds <= pre_split_median_seconds + pre_split_spread_seconds"
        res["verdict"] = "holds" if res["tiles_median_seconds"] <= res["pre_split_median_seconds"] + res["pre_split_spread_seconds"] else "refuted"
    finally:
        shutil.rmtree(d, ignore_errors=True)
    sdb.tree.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
