#!/usr/bin/env python3
"""The anchor index timed against kmu_anchor_match, the route without it.

Device-resident anchors of ONT-shaped reads (kmerutils_amd.synth; the batch of scripts/bench_anchor_match.py: k = 21, nbkmer 16,
window 500 / overlap 250, the reference's hashes), group = read, min_common 1.
  (a) reuse   the rows as one database, cut into eight query batches: one ctx.anchor_index plus eight index.match calls, against
              eight ctx.anchor_match calls (each builds and sorts the database's entries, twice); n_keys 1 and 4
  (b) single  create + match + close against one ctx.anchor_match, the whole batch against itself: the price of the directory
  (c) mask    the same reads with 600 bases of a tenth of them overwritten by A: an index of the batch, its occupancy histogram,
              max_occ = max_occ_for_fraction(hist, 2e-4); match with max_occ = 0 against match with that max_occ: time and pairs
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max.  The pairs of the
two routes of (a) and (b) are compared once.  One JSON line.

  scripts/bench_anchor_index.py [--reads 20000] [--mean-len 5000] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--mean-len", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import anchor, lib, synth
    dev = torch.device("cuda", 0)
    k, nbkmer, window, overlap = 21, 16, 500, 250
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    p = A.SketchParams(A.ALGO_BOTTOMK, A.KMER64BIT, k, nbkmer, A.SIG_U64, A.HASHER_INT64HASH, A.FHASH_VALUE_MASKED, 0,
                       A.MODE_PER_SEQ, A.INPUT_ASCII, A.MEM_DEVICE, 0)

    def anchors_of(b):
        hashes, _, _, row_off = ctx.read_anchors(b, off, p, window, overlap, want_counts=False)
        h_group = np.repeat(np.arange(args.reads, dtype=np.uint32), np.diff(row_off.astype(np.int64)))
        return hashes.contiguous(), torch.from_numpy(h_group.view(np.int32)).to(dev)

    hashes, group = anchors_of(bases)
    rows = int(hashes.shape[0])
    res = {"reads": args.reads, "bases": int(off[-1].item()), "rows": rows, "k": k, "nbkmer": nbkmer, "window": window,
           "overlap": overlap, "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "reuse": [], "single": [], "mask": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def alternate(routes):
        for fn in routes.values():
            timed(fn)
        t = {name: [] for name in routes}
        for _ in range(args.repeats):
            for name, fn in routes.items():
                t[name].append(timed(fn)[0])
        return {name: stat(v) for name, v in t.items()}

    def same(x, y):
        return bool(all(torch.equal(a, b) for a, b in zip(x, y)))

    cuts = [rows * i // 8 for i in range(9)]
    batches = [(hashes[cuts[i]:cuts[i + 1]].contiguous(), group[cuts[i]:cuts[i + 1]].contiguous()) for i in range(8)]
    for n_keys in (1, 4):
        def with_index():
            with ctx.anchor_index(hashes, n_keys=n_keys, group_db=group) as index:
                return [index.match(q, group_q=g, min_common=1) for q, g in batches]

        def without():
            return [ctx.anchor_match(q, hashes, n_keys=n_keys, min_common=1, group_q=g, group_db=group) for q, g in batches]

        ms = alternate({"index": with_index, "anchor_match": without})
        x, y = with_index(), without()
        res["reuse"].append({"n_keys": n_keys, "pairs": int(sum(a[0].shape[0] for a in x)), "ms": ms,
                             "pairs_equal": all(same(a, b) for a, b in zip(x, y)),
                             "index_over_anchor_match": ms["index"]["median"] / ms["anchor_match"]["median"]})

        def single_index():
            with ctx.anchor_index(hashes, n_keys=n_keys, group_db=group) as index:
                return index.match(hashes, group_q=group, min_common=1)

        def single_plain():
            return ctx.anchor_match(hashes, hashes, n_keys=n_keys, min_common=1, group_q=group, group_db=group)

        ms = alternate({"index": single_index, "anchor_match": single_plain})
        x, y = single_index(), single_plain()
        res["single"].append({"n_keys": n_keys, "pairs": int(x[0].shape[0]), "ms": ms, "pairs_equal": same(x, y),
                              "index_over_anchor_match": ms["index"]["median"] / ms["anchor_match"]["median"]})

    # (c) a low-complexity stretch in a tenth of the reads
    h_off = off.cpu().numpy().astype(np.int64)
    dirty = bases.clone()
    n_dirty = 0
    for i in range(0, args.reads, 10):
        if h_off[i + 1] - h_off[i] >= 1200:
            dirty[h_off[i] + 300:h_off[i] + 900] = ord("A")
            n_dirty += 1
    dhashes, dgroup = anchors_of(dirty)
    for n_keys in (1, 4):
        with ctx.anchor_index(dhashes, n_keys=n_keys, group_db=dgroup) as index:
            info = index.info()
            hist = index.occupancy(info["max_occupancy"] + 1)
            max_occ = anchor.max_occ_for_fraction(hist, 2e-4)
            ms = alternate({"unmasked": lambda: index.match(dhashes, group_q=dgroup, min_common=1, max_occ=0),
                            "masked": lambda: index.match(dhashes, group_q=dgroup, min_common=1, max_occ=max_occ)})
            res["mask"].append({"n_keys": n_keys, "reads_with_insert": n_dirty, "n_distinct": info["n_distinct"],
                                "max_occupancy": info["max_occupancy"], "max_occ": max_occ, "ms": ms,
                                "pairs_unmasked": int(index.match(dhashes, group_q=dgroup, min_common=1, max_occ=0)[0].shape[0]),
                                "pairs_masked": int(index.match(dhashes, group_q=dgroup, min_common=1, max_occ=max_occ)[0].shape[0])})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
