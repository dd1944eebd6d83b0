#!/usr/bin/env python3
"""kmu_anchor_overlaps timed against what a caller had without it.

The batch of scripts/bench_anchor_match.py: device-resident anchors of ONT-shaped reads (k = 21, nbkmer 16, window 500 / overlap
250, the reference's hashes).  From those rows to read pairs (each once, band 1, min_score 2), by two routes:
  device     ctx.anchor_match as a self-join on the resident rows, then ctx.anchor_overlaps on its device output (KMU_OVL_UPPER):
             four library calls (each counts, then writes); only the records would leave the device
  host       today's route: anchor.match_read_anchors (the same join, its pairs copied to the host and turned into records),
             then a numpy group-by over those records that applies the rules of include/kmu.h (sort, run sums with reduceat, band
             sums by shifted adds, first-of-the-largest per read pair)
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max, and the device
time of the kernels of one device route (kmu_profile_get).  The records of the two routes are compared once.  One JSON line.

  scripts/bench_anchor_overlaps.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--out FILE]
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


def group_by(np, rec, stride, strands, band, min_score):
    """records [n, 6] of match_read_anchors -> records of kmu_anchor_overlaps with KMU_OVL_UPPER, read numbers as read indices"""
    rec = rec[rec[:, 0] < rec[:, 2]]
    ra, rb, w = rec[:, 0], rec[:, 2], rec[:, 4]
    sa, sb = rec[:, 1] // stride, rec[:, 3] // stride
    ra, rb, w, sa = (np.tile(x, strands) for x in (ra, rb, w, sa))
    s = np.repeat(np.arange(strands), rec.shape[0])
    d = np.concatenate([rec[:, 1] // stride - sb, rec[:, 1] // stride + sb][:strands])
    order = np.lexsort((d, s, rb, ra))
    ra, rb, s, d, w, sa = (x[order] for x in (ra, rb, s, d, w, sa))
    if ra.size == 0:
        return np.zeros((0, 8), np.int64)
    head = np.ones(ra.size, bool)
    head[1:] = (ra[1:] != ra[:-1]) | (rb[1:] != rb[:-1]) | (s[1:] != s[:-1]) | (d[1:] != d[:-1])
    at = np.nonzero(head)[0]
    ra, rb, s, d = ra[at], rb[at], s[at], d[at]  # per run
    W, V = np.add.reduceat(w, at), np.diff(np.append(at, sa.size))
    lo, hi = np.minimum.reduceat(sa, at), np.maximum.reduceat(sa, at)
    S, votes, blo, bhi = W.copy(), V.copy(), lo.copy(), hi.copy()
    n = ra.size
    for t in range(1, band + 1):
        ok = np.zeros(n, bool)
        ok[:n - t] = (ra[t:] == ra[:n - t]) & (rb[t:] == rb[:n - t]) & (s[t:] == s[:n - t]) & (d[t:] - d[:n - t] <= band)
        i = np.nonzero(ok)[0]
        S[i] += W[i + t]
        votes[i] += V[i + t]
        blo[i] = np.minimum(blo[i], lo[i + t])
        bhi[i] = np.maximum(bhi[i], hi[i + t])
    phead = np.ones(n, bool)
    phead[1:] = (ra[1:] != ra[:-1]) | (rb[1:] != rb[:-1])
    pat = np.nonzero(phead)[0]
    best = np.maximum.reduceat(S, pat)
    seg = np.cumsum(phead) - 1
    first = np.minimum.reduceat(np.where(S == best[seg], np.arange(n), n), pat)  # runs are in (strand, d) order: the tie rule
    first = first[best >= min_score]
    return np.stack([ra[first], rb[first], s[first], d[first], np.minimum(S[first], 0xFFFFFFFF), votes[first], blo[first], bhi[first]],
                    axis=1).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--mean-len", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
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
    params = anchor.AnchorsGeneratorParameters("bench", window, nbkmer, k, overlap)
    p = params.sketch_params()
    p.mem = A.MEM_DEVICE
    hashes, _, n, row_off = ctx.read_anchors(bases, off, p, window, overlap, want_counts=False)
    hashes = hashes.contiguous()
    rows = int(row_off[-1])
    h_group = np.repeat(np.arange(args.reads, dtype=np.uint32), np.diff(row_off.astype(np.int64)))
    group = torch.from_numpy(h_group.view(np.int32)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(row_off.astype(np.uint64)).view(np.int64)).to(dev)
    res = {"reads": args.reads, "bases": int(off[-1].item()), "rows": rows, "k": k, "nbkmer": nbkmer, "window": window,
           "overlap": overlap, "band": 1, "min_score": 2, "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "cases": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for n_keys, strands in ((1, 1), (4, 1), (4, 2)):
        def device():
            pairs, dist = ctx.anchor_match(hashes, hashes, n_keys=n_keys, min_common=1, group_q=group, group_db=group)
            return pairs, ctx.anchor_overlaps(pairs, dist, d_off, strands=strands, band=1, min_score=2, upper=True)

        def host():
            rec = anchor.match_read_anchors(ctx, hashes, row_off, params, n_keys=n_keys, min_common=1)
            return group_by(np, rec, params.get_stride(), strands, 1, 2)

        timed(device)
        timed(host)
        t = {"device": [], "host": []}
        for _ in range(args.repeats):
            t["device"].append(timed(device)[0])
            t["host"].append(timed(host)[0])
        pairs, got = device()
        got = got.cpu().numpy().astype(np.int64)
        got[:, 4:6] = got[:, 4:6] & 0xFFFFFFFF  # (score and votes are unsigned)
        want = host()
        same = bool(got.shape == want.shape and np.array_equal(got, want))
        ctx.profile_enable(True)
        ctx.profile_reset()
        device()
        ctx.synchronize()
        prof = {name: round(v[1], 4) for name, v in ctx.profile_get().items() if v[0]}
        ctx.profile_enable(False)
        res["cases"].append({"n_keys": n_keys, "strands": strands, "window_pairs": int(pairs.shape[0]), "overlaps": int(got.shape[0]),
                             "ms": {name: stat(v) for name, v in t.items()}, "records_equal": same,
                             "device_over_host": stat(t["device"])["median"] / stat(t["host"])["median"], "kernels_ms": prof})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    if not all(c["records_equal"] for c in res["cases"]):
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
