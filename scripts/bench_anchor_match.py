#!/usr/bin/env python3
"""kmu_anchor_match timed against what a caller had without it.

Device-resident anchors of ONT-shaped reads (kmerutils_amd.synth; the setup of scripts/bench_anchors.py: k = 21, nbkmer 16, window
500 / overlap 250, the reference's hashes), self-join with group = read, min_common 1, n_keys 1 and 4.  Per n_keys:
  match      ctx.anchor_match on the resident rows (its count-only call and its exact-capacity call), pairs left on the device
  baseline   the rows copied to the host, the inverse index built the way anchor.anchors_by_minhash builds it (a Python loop over
             rows into a dict, here over the first n_keys hashes of a row), the pairs of every bucket whose rows belong to
             different reads listed once, then ONE kmu_minhash_distance_pairs call on the host arrays and the common >= 1 filter
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max, and the device
time of the kernels of one match call (kmu_profile_get).  The pair sets of the two routes are compared once.  One JSON line.

  scripts/bench_anchor_match.py [--reads 20000] [--mean-len 5000] [--repeats 7] [--out FILE]
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
    from kmerutils_amd import lib, synth
    dev = torch.device("cuda", 0)
    k, nbkmer, window, overlap = 21, 16, 500, 250
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    p = A.SketchParams(A.ALGO_BOTTOMK, A.KMER64BIT, k, nbkmer, A.SIG_U64, A.HASHER_INT64HASH, A.FHASH_VALUE_MASKED, 0,
                       A.MODE_PER_SEQ, A.INPUT_ASCII, A.MEM_DEVICE, 0)
    hashes, _, n, row_off = ctx.read_anchors(bases, off, p, window, overlap, want_counts=False)
    hashes = hashes.contiguous()
    rows = int(row_off[-1])
    h_group = np.repeat(np.arange(args.reads, dtype=np.uint32), np.diff(row_off.astype(np.int64)))
    group = torch.from_numpy(h_group.view(np.int32)).to(dev)
    res = {"reads": args.reads, "bases": int(off[-1].item()), "rows": rows, "k": k, "nbkmer": nbkmer, "window": window,
           "overlap": overlap, "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "cases": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for n_keys in (1, 4):
        def match():
            return ctx.anchor_match(hashes, hashes, n_keys=n_keys, min_common=1, group_q=group, group_db=group)

        def baseline():
            h = hashes.cpu().numpy().view(np.uint64)
            hn = n.cpu().numpy().view(np.uint32)
            index = {}
            for r in range(rows):
                for key in h[r, :min(n_keys, int(hn[r]))].tolist():
                    index.setdefault(key, []).append(r)
            found = set()
            for bucket in index.values():
                if len(bucket) > 1:
                    for a in bucket:
                        for b in bucket:
                            if h_group[a] != h_group[b]:
                                found.add((a, b))
            pairs = np.array(sorted(found), np.uint32).reshape(-1, 2)
            d = ctx.minhash_distance_pairs(h, h, np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1]))
            keep = d[:, 0] >= 1
            return pairs[keep], d[keep]

        timed(match)
        timed(baseline)
        t = {"match": [], "baseline": []}
        for _ in range(args.repeats):
            t["match"].append(timed(match)[0])
            t["baseline"].append(timed(baseline)[0])
        gp, gd = match()
        wp, wd = baseline()
        gp = gp.cpu().numpy().view(np.uint32)
        gd = gd.cpu().numpy().view(np.uint32)
        o = np.lexsort((gp[:, 1], gp[:, 0]))  # the baseline lists its pairs by (a, b)
        same = bool(np.array_equal(gp[o], wp) and np.array_equal(gd[o], wd))
        ctx.profile_enable(True)
        ctx.profile_reset()
        match()
        ctx.synchronize()
        prof = {name: round(v[1], 4) for name, v in ctx.profile_get().items() if v[0]}
        ctx.profile_enable(False)
        res["cases"].append({"n_keys": n_keys, "pairs": int(gp.shape[0]), "ms": {name: stat(v) for name, v in t.items()},
                             "pairs_equal": same, "match_over_baseline": stat(t["match"])["median"] / stat(t["baseline"])["median"],
                             "kernels_ms": prof})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
