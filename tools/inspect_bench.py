#!/usr/bin/env python3
"""Time utree_inspect_file next to utree_compare_files of the same file against itself (GPU).  A record, not a gate: writes
profiles/inspect_bench.json.

    python tools/inspect_bench.py [--nodes 600000000] [--planted 0.10] [--labels 2000] [--runs 3] [--dir DIR] [--keep] [--out profiles/inspect_bench.json]

The input is one of tools/merge_bench.py's synthetic k = 32 `.ubt` files (W = 8, I = 2, uniformly random words, `--labels` labels) in which
a share `--planted` of the nodes is a copy of another node with one base substituted at a uniformly random position, under a label of
its own draw.  The inspection and the compare of the file against itself -- which spends its time in the same decode-and-sort front --
run alternately, `--runs` times each, in one session.  Reported: the total seconds, the neighbour pass alone (what UTREE_TIMING prints:
the stats' seconds_neighbours), and lookups per second = nodes x 96 / neighbour pass.  The HBM bytes moved per lookup come from counters
taken in a run of their own on the kept file (--keep --dir DIR):

    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d OUT -- utree_amd/utree-inspect DIR/db.ubt OUT/report.tsv OUT/pairs.tsv

and `--counters FETCH_KB` adds what that run read for neighbours_k to the record as bytes per lookup."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from merge_bench import sorted_unique_words, write_ubt
from utree_amd import search


def generate(d, nodes, planted, n_labels, dev):
    """the input file in directory d: (its path, its nodes)"""
    n_pl = int(nodes * planted)
    base = sorted_unique_words(nodes - n_pl, 1, dev)
    g = torch.Generator(device=dev).manual_seed(5)
    pick = base[torch.randperm(len(base), device=dev, generator=g)[:n_pl]]
    pos = torch.randint(0, 32, (n_pl,), generator=g, device=dev, dtype=torch.int64)
    sub = torch.randint(1, 4, (n_pl,), generator=g, device=dev, dtype=torch.int64)
    sub = torch.where(pos == 31, torch.ones_like(sub), sub)        # the top bit stays clear (merge_bench: signed order = unsigned order)
    mut = pick ^ (sub << (2 * pos))
    words = torch.unique(torch.cat([base, mut]))
    del base, pick, pos, sub, mut
    labels = [b"k__Bac;p__P%d;c__C%d;o__O%d;f__F%d;g__G%d;s__S%d" % (j % 7, j % 31, j % 101, j % 499, j % 997, j) for j in range(n_labels)]
    ix = torch.randint(0, n_labels, (len(words),), generator=g, device=dev, dtype=torch.int16)
    p = os.path.join(d, "db.ubt")
    write_ubt(p, words, ix, labels)
    n = len(words)
    del words, ix
    torch.cuda.empty_cache()
    return p, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=600_000_000)
    ap.add_argument("--planted", type=float, default=0.10)
    ap.add_argument("--labels", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--keep", action="store_true", help="leave the generated file in --dir")
    ap.add_argument("--counters", type=float, default=None, metavar="FETCH_KB", help="FETCH_SIZE of neighbours_k from a counter run of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inspect_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d = a.dir or tempfile.mkdtemp(prefix="inspect_bench_")
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    try:
        path, n = generate(d, a.nodes, a.planted, a.labels, dev)
        t_gen = time.time() - t0
        report, pairs, creport = os.path.join(d, "report.tsv"), os.path.join(d, "pairs.tsv"), os.path.join(d, "compare.tsv")
        ins_s, nb_s, cmp_s, st, cs = [], [], [], None, None
        for _ in range(a.runs):                                       # alternating, so that both see the same page cache and device state
            st = search.inspect(path, report, pairs)
            ins_s.append(st.seconds)
            nb_s.append(st.seconds_neighbours)
            cs = search.compare(path, path, creport)
            cmp_s.append(cs.seconds)
        lookups = st.kmers * 96
        figures = lambda s: {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "spread": max(s) - min(s)}
        rec = {
            "what": "utree_inspect_file on a synthetic k = 32 .ubt file (W = 8, I = 2) with planted neighbours, alternating with utree_compare_files of the file against itself in one session",
            "device": torch.cuda.get_device_name(0), "nodes": n, "labels": a.labels, "planted_share_asked": a.planted, "runs": a.runs,
            "GB_in": os.path.getsize(path) / 1e9,
            "inspect": dict(figures(ins_s), kmers=st.kmers, isolated=st.isolated, same=st.same, lineage=st.lineage, conflict=st.conflict,
                            pair_events=st.pair_events, distinct_pairs=st.distinct_pairs, passes=st.n_passes,
                            report_bytes=os.path.getsize(report), pairs_bytes=os.path.getsize(pairs)),
            "neighbour_pass": dict(figures(nb_s), lookups=lookups, lookups_per_s=lookups / statistics.median(nb_s)),
            "compare_self": dict(figures(cmp_s), same=cs.same, passes=cs.n_passes),
            "inspect_over_compare_median": statistics.median(ins_s) / statistics.median(cmp_s),
            "hbm_bytes_per_lookup": None if a.counters is None else {"FETCH_SIZE_KB_neighbours_k": a.counters, "bytes_per_lookup": a.counters * 1024 / lookups,
                                                                      "note": "FETCH_SIZE as rocprofv3 reports it; coalesced streams of such a run (decode_k, inspect_append_k) report half their bytes, "
                                                                              "per-lane gathers are uncalibrated: the true figure lies between this one and twice it"},
            "generate_seconds": t_gen,
        }
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps(rec))
    finally:
        if not a.dir or not a.keep:
            for f in ("db.ubt", "report.tsv", "pairs.tsv", "compare.tsv"):
                if os.path.exists(os.path.join(d, f)):
                    os.unlink(os.path.join(d, f))
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
