#!/usr/bin/env python3
"""Time utree_compare_files next to utree_merge_files on the same inputs (GPU).  A record, not a gate: writes profiles/compare_bench.json.

    python tools/compare_bench.py [--nodes 600000000] [--shared 0.10] [--labels 2000] [--runs 3] [--dir DIR] [--out profiles/compare_bench.json]

The inputs are tools/merge_bench.py's: two `.ubt` files of `--nodes` nodes each (W = 8, I = 2) with uniformly random words, a share
`--shared` of each file's words also in the other under a sibling label.  The compare and the merge run alternately, `--runs` times each,
in one session: the compare reads the same bytes and writes a few kilobytes where the merge writes a database, so the expectation this
records is that the compare is not slower than the merge by more than the runs' spread."""
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

from merge_bench import generate
from utree_amd import search


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=600_000_000)
    ap.add_argument("--shared", type=float, default=0.10)
    ap.add_argument("--labels", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d = a.dir or tempfile.mkdtemp(prefix="compare_bench_")
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    try:
        paths, n_in = generate(d, a.nodes, a.shared, a.labels, dev)
        t_gen = time.time() - t0
        report, moves, out = os.path.join(d, "report.tsv"), os.path.join(d, "moves.tsv"), os.path.join(d, "merged.ubt")
        cmp_s, mrg_s, cs, ms = [], [], None, None
        for _ in range(a.runs):                                       # alternating, so that both see the same page cache and device state
            cs = search.compare(paths[0], paths[1], report, moves)
            cmp_s.append(cs.seconds)
            ms = search.merge(paths, out)
            mrg_s.append(ms.seconds)
        bytes_in = sum(os.path.getsize(p) for p in paths)
        figures = lambda s: {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "spread": max(s) - min(s)}
        rec = {
            "what": "utree_compare_files and utree_merge_files on the same two synthetic k = 32 .ubt files (W = 8, I = 2), alternating in one session",
            "device": torch.cuda.get_device_name(0), "nodes_per_input": n_in, "labels_per_input": a.labels, "shared_share_asked": a.shared,
            "runs": a.runs, "GB_in": bytes_in / 1e9,
            "compare": dict(figures(cmp_s), words=cs.words, both=cs.both, same=cs.same, changed=cs.left, only_a=cs.only_a, only_b=cs.only_b,
                            distinct_moves=cs.n_moves, passes=cs.n_passes, GB_per_s_in=bytes_in / 1e9 / statistics.median(cmp_s),
                            report_bytes=os.path.getsize(report), moves_bytes=os.path.getsize(moves)),
            "merge": dict(figures(mrg_s), nodes_out=ms.n_nodes, shared=ms.n_shared, passes=ms.n_passes, GB_out=os.path.getsize(out) / 1e9,
                          GB_per_s_in=bytes_in / 1e9 / statistics.median(mrg_s)),
            "compare_over_merge_median": statistics.median(cmp_s) / statistics.median(mrg_s),
            "generate_seconds": t_gen,
        }
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps(rec))
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
