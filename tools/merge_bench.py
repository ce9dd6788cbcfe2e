#!/usr/bin/env python3
"""Time utree_merge_files on two synthetic k = 32 `.ubt` files (GPU).  A record, not a gate: writes profiles/merge_bench.json.

    python tools/merge_bench.py [--nodes 600000000] [--shared 0.10] [--labels 2000] [--dir DIR] [--out profiles/merge_bench.json]

Two files of `--nodes` nodes each (W = 8, I = 2: 10-byte records) with uniformly random words; a share `--shared` of each file's words
also stands in the other, under a sibling label, so that many runs are cut to their common prefix.  The files are generated on the GPU
(torch) and written to --dir (default: a temporary directory, removed afterwards).  The same file also records the time xtree-compress
takes on the merged file: the yardstick for "one streaming pass over this many bytes on this host"."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from utree_amd import search


def sorted_unique_words(n, seed, dev):
    """n distinct 63-bit words, ascending (int64 on the device; the top bit stays clear so that signed order = unsigned order)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    w = torch.randint(0, 2 ** 63 - 1, (int(n * 1.001) + 16,), generator=g, device=dev, dtype=torch.int64)
    w = torch.unique(w)                                              # sorted
    assert len(w) >= n
    return w[:n]


def write_ubt(path, words, ix, labels, chunk=1 << 26):
    """words: int64 ascending on the device, ix: int16 on the device"""
    n = len(words)
    counts = torch.bincount(ix.to(torch.int64), minlength=len(labels)).cpu().numpy()
    with open(path, "wb") as f:
        f.write(np.array([8, 0, 2, n], dtype="<u8").tobytes())
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            rec = torch.empty((b - a, 10), dtype=torch.uint8, device=words.device)
            rec[:, :8] = words[a:b].contiguous().view(torch.uint8).view(-1, 8)
            rec[:, 8:] = ix[a:b].contiguous().view(torch.uint8).view(-1, 2)
            f.write(rec.cpu().numpy().tobytes())
        f.write(b"".join(l + b"\t%d\n" % c for l, c in zip(labels, counts)))


def generate(d, nodes, shared, n_labels, dev):
    """the two input files in directory d: (their paths, their node counts)"""
    n, n_sh = nodes, int(nodes * shared)
    own_a = sorted_unique_words(n, 1, dev)
    own_b = sorted_unique_words(n - n_sh, 2, dev)
    pick = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(3))[:n_sh]
    words_b = torch.unique(torch.cat([own_b, own_a[pick]]))       # a word both generators drew (about n^2 / 2^63 of them) counts as shared
    del own_b, pick
    labels = [[b"k__Bac;p__P%d;c__C%d;o__O%d;f__F%d;g__G%d;s__S%d_%s" % (j % 7, j % 31, j % 101, j % 499, j % 997, j, t) for j in range(n_labels)]
              for t in (b"a", b"b")]
    g = torch.Generator(device=dev).manual_seed(4)
    paths = []
    for k, w in enumerate((own_a, words_b)):
        ix = torch.randint(0, n_labels, (len(w),), generator=g, device=dev, dtype=torch.int16)
        p = os.path.join(d, "in%d.ubt" % k)
        write_ubt(p, w, ix, labels[k])
        paths.append(p)
        del ix
    n_in = [len(own_a), len(words_b)]
    del own_a, words_b
    torch.cuda.empty_cache()
    return paths, n_in


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=600_000_000)
    ap.add_argument("--shared", type=float, default=0.10)
    ap.add_argument("--labels", type=int, default=2000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d = a.dir or tempfile.mkdtemp(prefix="merge_bench_")
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    try:
        paths, n_in = generate(d, a.nodes, a.shared, a.labels, dev)
        t_gen = time.time() - t0
        out, ctr = os.path.join(d, "merged.ubt"), os.path.join(d, "merged.ctr")
        st = search.merge(paths, out)
        bytes_in, bytes_out = sum(os.path.getsize(p) for p in paths), os.path.getsize(out)
        code, cs = search.compress(out, ctr)
        assert code == 0, code
        rec = {
            "what": "utree_merge_files on two synthetic k = 32 .ubt files (W = 8, I = 2), and xtree-compress on the merged file",
            "device": torch.cuda.get_device_name(0), "nodes_per_input": n_in, "labels_per_input": a.labels, "shared_share_asked": a.shared,
            "merge": {"seconds": st.seconds, "nodes_in": st.n_in_nodes, "nodes_out": st.n_nodes, "shared": st.n_shared, "relabelled": st.n_relabelled,
                      "dropped": st.n_dropped, "labels_out": st.n_labels, "passes": st.n_passes, "nodes_in_per_s": st.n_in_nodes / st.seconds,
                      "GB_in": bytes_in / 1e9, "GB_out": bytes_out / 1e9, "GB_per_s_in": bytes_in / 1e9 / st.seconds, "GB_per_s_out": bytes_out / 1e9 / st.seconds},
            "compress_of_merged": {"seconds": cs.seconds, "nodes": cs.n_nodes, "GB_in": bytes_out / 1e9, "GB_out": os.path.getsize(ctr) / 1e9,
                                   "GB_per_s_in": bytes_out / 1e9 / cs.seconds},
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
