#!/usr/bin/env python3
"""kmu_read_anchors timed against what a caller does without it.

Device-resident ONT-shaped reads (kmerutils_amd.synth), k = 21, nbkmer 16, the reference's anchors (int64_hash of the forward
k-mer's value), two shapes: (window 2000, overlap 500) and (window 500, overlap 250).  Per shape:
  anchors       one kmu_read_anchors call over the reads
  baseline      every window materialised as a sequence of its own (one gather on the device), then ONE kmu_sketch(BOTTOMK)
                call over all of them -- timed as the sketch call alone and as copy + sketch
Host clock around synchronised calls; warm-up first, then --repeats runs of each in alternation; median / min / max, and the
device time of the kernels of one call (kmu_profile_get).  The rows of the two routes are compared once.  One JSON line.

  scripts/bench_anchors.py [--reads 20000] [--mean-len 5000] [--repeats 7] [--out FILE]
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
    k, nbkmer = 21, 16
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    h_off = off.cpu().numpy().astype(np.uint64)
    ctx = lib.Context(0)
    p = A.SketchParams(A.ALGO_BOTTOMK, A.KMER64BIT, k, nbkmer, A.SIG_U64, A.HASHER_INT64HASH, A.FHASH_VALUE_MASKED, 0,
                       A.MODE_PER_SEQ, A.INPUT_ASCII, A.MEM_DEVICE, 0)
    res = {"reads": args.reads, "bases": int(h_off[-1]), "k": k, "nbkmer": nbkmer, "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "shapes": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def kernels_ms(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        ctx.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        return {n: round(v[1], 4) for n, v in prof.items() if v[0]}

    for window, overlap in ((2000, 500), (500, 250)):
        stride = window - overlap
        rows = lib.anchor_layout(h_off, window, overlap)
        # the windows of the baseline, by the same rule: beg = s * stride, end = min(beg + window, L - 1); empty ones left out
        # (kmu_sketch has no row for an empty sequence)
        L = np.diff(h_off.astype(np.int64))
        read_of = np.repeat(np.arange(args.reads), np.diff(rows.astype(np.int64)))
        beg = (np.arange(int(rows[-1])) - rows[read_of].astype(np.int64)) * stride
        wlen = np.minimum(beg + window, L[read_of] - 1) - beg
        keep = wlen > 0
        d_beg = torch.from_numpy((h_off[read_of].astype(np.int64) + beg)[keep]).to(dev)
        d_len = torch.from_numpy(wlen[keep]).to(dev)

        def materialise():
            woff = torch.zeros(d_len.numel() + 1, dtype=torch.int64, device=dev)
            torch.cumsum(d_len, 0, out=woff[1:])
            idx = torch.arange(int(woff[-1].item()), device=dev) + torch.repeat_interleave(d_beg - woff[:-1], d_len)
            return bases[idx], woff

        def anchors():
            return ctx.read_anchors(bases, off, p, window, overlap)

        wb, wo = materialise()

        def sketch_windows():
            return ctx.sketch(wb, wo, p, want_counts=True)

        def copy_and_sketch():
            b, o = materialise()
            return ctx.sketch(b, o, p, want_counts=True)

        for f in (anchors, sketch_windows, copy_and_sketch):  # warm-up
            timed(f)
        t = {"anchors": [], "baseline_sketch": [], "baseline_copy_sketch": []}
        for _ in range(args.repeats):
            t["anchors"].append(timed(anchors)[0])
            t["baseline_sketch"].append(timed(sketch_windows)[0])
            t["baseline_copy_sketch"].append(timed(copy_and_sketch)[0])
        got, want = anchors(), sketch_windows()
        same = bool(torch.equal(got[0][torch.from_numpy(keep).to(dev)], want[0]) and
                    torch.equal(got[1][torch.from_numpy(keep).to(dev)], want[1]))
        res["shapes"].append({"window": window, "overlap": overlap, "rows": int(rows[-1]), "window_bases": int(wo[-1].item()),
                              "ms": {n: stat(v) for n, v in t.items()}, "rows_equal": same,
                              "anchors_over_baseline_sketch": stat(t["anchors"])["median"] / stat(t["baseline_sketch"])["median"],
                              "kernels_ms": {"anchors": kernels_ms(anchors), "baseline_sketch": kernels_ms(sketch_windows)}})
        del wb, wo
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
