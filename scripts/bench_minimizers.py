#!/usr/bin/env python3
"""kmu_read_minimizers timed against what a caller does without it.

Device-resident ONT-shaped reads (kmerutils_amd.synth), k = 21, KMU_FHASH_CANON_INVHASH, w in {5, 10, 19}.  Per w:
  minimizers    one Context.read_minimizers call (count + write) over the reads: hashes, positions, reads, strands stay on the device
  host_route    the route without it: kmu_kmer_hashes on the device, the array copied to the host (8 bytes per base), and a
                numpy sliding arg-min per read (sliding_window_view(...).argmin, first occurrence) with the distinct choices kept
  hashes_only   kmu_kmer_hashes alone: every k-mer hashed once and written -- the floor of the kernel
Host clock around synchronised calls; warm-up first, then --repeats runs of each in alternation; median / min / max, and the
device time of the kernels of one call (kmu_profile_get).  The positions of the two routes are compared once.  One JSON line.

  scripts/bench_minimizers.py [--reads 20000] [--mean-len 5000] [--repeats 7] [--out FILE]
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
    k, kt, fhash = 21, A.KMER64BIT, A.FHASH_CANON_INVHASH
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    h_off = off.cpu().numpy().astype(np.int64)
    ctx = lib.Context(0)
    res = {"reads": args.reads, "bases": int(h_off[-1]), "k": k, "fhash": "canon_invhash", "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "windows": []}
    d_hashes = torch.zeros(int(h_off[-1]), dtype=torch.int64, device=dev)

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

    def hashes_only():
        return ctx.kmer_hashes(bases, off, kt, k, fhash, out=d_hashes)

    for w in (5, 10, 19):
        def minimizers():
            return ctx.read_minimizers(bases, off, kt, k, fhash, w, want=("pos", "read", "strand"))

        def host_route():
            h = hashes_only().cpu().numpy().view(np.uint64)
            pos = []
            for i in range(args.reads):
                nk = int(h_off[i + 1] - h_off[i]) - k + 1
                if nk <= 0:
                    continue
                hr = h[h_off[i]:h_off[i] + nk]
                if nk <= w:
                    c = np.array([int(np.argmin(hr))])
                else:
                    c = np.lib.stride_tricks.sliding_window_view(hr, w).argmin(axis=1) + np.arange(nk - w + 1)
                keep = np.ones(c.size, bool)
                keep[1:] = c[1:] != c[:-1]
                pos.append(c[keep])
            return np.concatenate(pos)

        for f in (minimizers, host_route, hashes_only):  # warm-up
            timed(f)
        t = {"minimizers": [], "host_route": [], "hashes_only": []}
        for _ in range(args.repeats):
            t["minimizers"].append(timed(minimizers)[0])
            t["host_route"].append(timed(host_route)[0])
            t["hashes_only"].append(timed(hashes_only)[0])
        got, want = minimizers(), host_route()
        same = bool(np.array_equal(got[1].cpu().numpy().view(np.uint32), want.astype(np.uint32)))
        med = {n: stat(v)["median"] for n, v in t.items()}
        res["windows"].append({"w": w, "minimizers": int(got[0].numel()), "density": got[0].numel() / max(int(h_off[-1]), 1),
                               "ms": {n: stat(v) for n, v in t.items()}, "positions_equal": same,
                               "host_route_over_minimizers": med["host_route"] / med["minimizers"],
                               "minimizers_over_hashes_only": med["minimizers"] / med["hashes_only"],
                               "kernels_ms": {"minimizers": kernels_ms(minimizers), "hashes_only": kernels_ms(hashes_only)}})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
