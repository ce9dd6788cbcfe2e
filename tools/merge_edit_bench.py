#!/usr/bin/env python3
"""Time the merge with and without an edit (GPU).  A record, not a gate: writes profiles/merge_edit_bench.json.

    python tools/merge_edit_bench.py --parent-so PARENT/libutree_amd.so [--nodes 600000000] [--minus-nodes 100000000] [--runs 3]
                                     [--dir DIR] [--out profiles/merge_edit_bench.json]

(a) the UNEDITED merge on tools/merge_bench.py's inputs, this tree's library against the parent commit's (--parent-so: a library built
    from the parent commit), alternating, --runs each, every run a process of its own: both series, each series' spread (max - min) and
    whether this tree's median is within the larger spread of the parent's median;
(b) the EDITED merge on the same inputs: ranks = 7, 1 % of the labels dropped, a MINUS `.ubt` of --minus-nodes nodes (a tenth of its words
    drawn from the first input): seconds, nodes/s, GB/s in and out, and what an edit costs over (a)."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
NEW_SYMBOLS = ("utree_merge_files_edit", "utree_merge_edit_preview")


def leg(a):
    """one merge in this process; prints its figures as one JSON line"""
    from utree_amd import lib, search
    if a.leg == "plain":
        for name in NEW_SYMBOLS:                     # the parent's library does not have them; this leg does not call them
            lib.SYMBOLS.pop(name, None)
        st = search.merge([os.path.join(a.dir, "in0.ubt"), os.path.join(a.dir, "in1.ubt")], os.path.join(a.dir, "out.ubt"))
        rec = {}
    else:
        st, es = search.merge_edit([os.path.join(a.dir, "in0.ubt"), os.path.join(a.dir, "in1.ubt")], os.path.join(a.dir, "out.ubt"), ranks=7,
                                   drop=os.path.join(a.dir, "drop.rules"), minus=[os.path.join(a.dir, "minus.ubt")])
        rec = {f: getattr(es, f) for f, _ in lib.MergeEditStats._fields_}
    rec.update({f: getattr(st, f) for f, _ in lib.MergeStats._fields_})
    rec["bytes_out"] = os.path.getsize(os.path.join(a.dir, "out.ubt"))
    print(json.dumps(rec))


def run_leg(which, d, so=None):
    env = dict(os.environ)
    if so:
        env["UTREE_AMD_SO"] = so
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--dir", d], stdout=subprocess.PIPE, env=env, timeout=600)
    if p.returncode:
        raise SystemExit("leg %s failed with exit code %d" % (which, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def generate(a, d):
    import torch
    import merge_bench as MB
    dev = torch.device("cuda:0")
    n, n_sh = a.nodes, int(a.nodes * a.shared)
    own_a = MB.sorted_unique_words(n, 1, dev)
    own_b = MB.sorted_unique_words(n - n_sh, 2, dev)
    pick = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(3))[:n_sh]
    words_b = torch.unique(torch.cat([own_b, own_a[pick]]))
    del own_b, pick
    labels = [[b"k__Bac;p__P%d;c__C%d;o__O%d;f__F%d;g__G%d;s__S%d_%s;t__T%d" % (j % 7, j % 31, j % 101, j % 499, j % 997, j % 50, t, j)
               for j in range(a.labels)] for t in (b"a", b"b")]                              # eight ranks: ranks = 7 cuts every one of them
    g = torch.Generator(device=dev).manual_seed(4)
    for k, w in enumerate((own_a, words_b)):
        ix = torch.randint(0, a.labels, (len(w),), generator=g, device=dev, dtype=torch.int16)
        MB.write_ubt(os.path.join(d, "in%d.ubt" % k), w, ix, labels[k])
        del ix
    m_own = MB.sorted_unique_words(a.minus_nodes - a.minus_nodes // 10, 5, dev)
    pick = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(6))[:a.minus_nodes // 10]
    minus = torch.unique(torch.cat([m_own, own_a[pick]]))
    MB.write_ubt(os.path.join(d, "minus.ubt"), minus, torch.zeros(len(minus), dtype=torch.int16, device=dev), [b"k__Host"])
    with open(os.path.join(d, "drop.rules"), "wb") as f:                                      # 1 % of the labels of each input
        f.write(b"".join(l + b"\n" for ls in labels for l in ls[::100]))
    sizes = {"nodes_per_input": [len(own_a), len(words_b)], "minus_nodes": len(minus)}
    del own_a, words_b, minus, m_own
    torch.cuda.empty_cache()
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--nodes", type=int, default=600_000_000)
    ap.add_argument("--minus-nodes", type=int, default=100_000_000)
    ap.add_argument("--shared", type=float, default=0.10)
    ap.add_argument("--labels", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_edit_bench.json"))
    ap.add_argument("--leg", choices=("plain", "edit"), default=None)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    if not a.parent_so or not os.path.exists(a.parent_so):
        raise SystemExit("--parent-so: the parent commit's libutree_amd.so is needed for (a)")
    d = a.dir or tempfile.mkdtemp(prefix="merge_edit_bench_")
    os.makedirs(d, exist_ok=True)
    try:
        sizes = generate(a, d)
        import torch
        device = torch.cuda.get_device_name(0)
        bytes_in = [os.path.getsize(os.path.join(d, f)) for f in ("in0.ubt", "in1.ubt", "minus.ubt")]
        run_leg("plain", d)                                                                  # once unrecorded: the files enter the page cache
        series = {"parent": [], "this": []}
        last = None
        for _ in range(a.runs):
            series["parent"].append(run_leg("plain", d, os.path.abspath(a.parent_so))["seconds"])
            last = run_leg("plain", d)
            series["this"].append(last["seconds"])
        spread = {k: max(v) - min(v) for k, v in series.items()}
        med = {k: statistics.median(v) for k, v in series.items()}
        edits = [run_leg("edit", d) for _ in range(a.runs)]
        e = sorted(edits, key=lambda r: r["seconds"])[len(edits) // 2]
        rec = {
            "what": "utree_merge_files without an edit, this tree against the parent commit's library (alternating, one process per run), "
                    "and utree_merge_files_edit (ranks = 7, 1 % of the labels dropped, one MINUS .ubt) on the same inputs; W = 8, I = 2",
            "device": device, **sizes, "labels_per_input": a.labels, "shared_share_asked": a.shared,
            "unedited": {"seconds_parent": series["parent"], "seconds_this": series["this"], "spread_parent": spread["parent"], "spread_this": spread["this"],
                         "median_parent": med["parent"], "median_this": med["this"],
                         "this_within_spread_of_parent": med["this"] - med["parent"] <= max(spread.values()),
                         "nodes_in": last["n_in_nodes"], "nodes_out": last["n_nodes"], "GB_in": sum(bytes_in[:2]) / 1e9},
            "edited": {"seconds": [r["seconds"] for r in edits], "median_seconds": e["seconds"], "nodes_read": e["n_in_nodes"] + e["n_minus_nodes"],
                       "nodes_read_per_s": (e["n_in_nodes"] + e["n_minus_nodes"]) / e["seconds"], "GB_in": sum(bytes_in) / 1e9,
                       "GB_out": e["bytes_out"] / 1e9, "GB_per_s_in": sum(bytes_in) / 1e9 / e["seconds"], "GB_per_s_out": e["bytes_out"] / 1e9 / e["seconds"],
                       "seconds_over_unedited": e["seconds"] - med["this"], "stats": e},
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
