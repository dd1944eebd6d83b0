#!/usr/bin/env python3
"""Reading the count table back, timed against the kernels and the routes it stands next to.

Device-resident synthetic reads (kmerutils_amd.synth: fixed-length reads of a uniform genome with substitutions), counted into
an 8-bit Kmer64bit k = 31 table; then, per-kernel times through kmu_profile_get (HIP events on the context's stream):
  histogram  k_count_hist against k_count_stats (kmu_count_nb_distinct) on the same table: both one streaming read of the image;
             and the route it replaces, dump(1) + bincount on the host (host clock, once)
  profile    k_count_profile (counts only) against k_once_count (kmu_count_once_positions, size query) over the same reads and
             table: the same walk and look-ups without the 2 B per base of stores; stats only (k_count_profile + k_profile_stats);
             and today's three calls, kmu_kmer_hashes + kmu_count_query on the device + a per-read reduction on the host (host clock)
Warm-up first, then --repeats runs of each in alternation; median / min / max.  One JSON line, a text report in --out.

  scripts/bench_count_readback.py [--reads 1000000] [--read-len 150] [--genome 50000000] [--repeats 7] [--out FILE] [--no-routes]
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


def kernel_ms(ctx, fn, names):
    """per-launch time of the named kernels over one call of fn"""
    ctx.profile_reset()
    fn()
    ctx.synchronize()
    prof = ctx.profile_get()
    return {n: (prof[n][1] / prof[n][0] if n in prof and prof[n][0] else float("nan")) for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-routes", action="store_true", help="skip the host-clock routes (dump + bincount, the three calls)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, synth
    dev = torch.device("cuda", 0)
    k = 31
    total = args.reads * args.read_len
    bases, off, _ = synth.ont_reads_device(args.reads, total, args.genome, 0xC4, dev, errors=(0.005, 0.0, 0.0), fixed_len=args.read_len)
    ctx = lib.Context(0)
    c = ctx.counter(A.KMER64BIT, k, 8, max(1 << 20, int(args.genome * 1.5)))
    c.add_reads(bases, off)
    distinct = c.nb_distinct()
    ti = c.table_info()
    ctx.profile_enable(True)
    res = {"reads": args.reads, "read_len": args.read_len, "bases": total, "distinct": distinct, "table_bytes": ti["table_bytes"],
           "bytes_per_slot": ti["bytes_per_slot"], "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    hist_out = torch.zeros(256, dtype=torch.int64, device=dev)

    def run_hist():
        ctx._check(ctx.L.kmu_count_histogram(c.h, lib._ptr(hist_out)[0], 256, A.MEM_DEVICE))

    def run_once_count():
        n = lib.C.c_uint64(0)
        ctx._check(ctx.L.kmu_count_once_positions(c.h, lib._ptr(bases)[0], lib._ptr(off)[0], args.reads, A.MEM_DEVICE, None, None, None, 0,
                                                  lib.C.byref(n)))

    counts = torch.zeros(total, dtype=torch.int16, device=dev)
    for f in (run_hist, c.nb_distinct, run_once_count, lambda: c.read_profile(bases, off, want_stats=False, counts_out=counts),
              lambda: c.read_profile(bases, off, want_counts=False)):  # warm-up
        f()
    t = {"k_count_hist": [], "k_count_stats": [], "k_count_profile": [], "k_once_count": [], "stats_only.k_count_profile": [],
         "stats_only.k_profile_stats": []}
    for _ in range(args.repeats):
        t["k_count_hist"].append(kernel_ms(ctx, run_hist, ["k_count_hist"])["k_count_hist"])
        t["k_count_stats"].append(kernel_ms(ctx, c.nb_distinct, ["k_count_stats"])["k_count_stats"])
        t["k_count_profile"].append(kernel_ms(ctx, lambda: c.read_profile(bases, off, want_stats=False, counts_out=counts),
                                              ["k_count_profile"])["k_count_profile"])
        t["k_once_count"].append(kernel_ms(ctx, run_once_count, ["k_once_count"])["k_once_count"])
        so = kernel_ms(ctx, lambda: c.read_profile(bases, off, want_counts=False), ["k_count_profile", "k_profile_stats"])
        t["stats_only.k_count_profile"].append(so["k_count_profile"])
        t["stats_only.k_profile_stats"].append(so["k_profile_stats"])
    res["kernel_ms"] = {n: stat(v) for n, v in t.items()}
    res["hist_over_stats"] = res["kernel_ms"]["k_count_hist"]["median"] / res["kernel_ms"]["k_count_stats"]["median"]
    res["profile_minus_once_ms"] = res["kernel_ms"]["k_count_profile"]["median"] - res["kernel_ms"]["k_once_count"]["median"]
    res["profile_store_bytes"] = 2 * total
    hist = c.histogram()
    assert int(hist.sum()) == distinct and np.array_equal(hist, hist_out.cpu().numpy().astype(np.uint64))
    if not args.no_routes:
        ctx.profile_enable(False)
        t0 = time.perf_counter()
        _, dc = c.dump(1)
        want = np.bincount(dc.astype(np.int64), minlength=256)
        res["route_dump_bincount_ms"] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(want.astype(np.uint64), hist)
        t0 = time.perf_counter()
        h = ctx.kmer_hashes(bases, off, A.KMER64BIT, k, A.FHASH_CANON_VALUE)
        q = c.query(h).cpu().numpy()
        o = off.cpu().numpy()
        q2 = q.reshape(args.reads, args.read_len)[:, :args.read_len - k + 1]  # (fixed-length reads: the reduction at its cheapest)
        route = (q2.min(1), np.sort(q2, 1)[:, (q2.shape[1] - 1) // 2], q2.max(1), q2.sum(1), (q2 == 0).sum(1), (q2 == 1).sum(1), (q2 >= 2).sum(1))
        res["route_three_calls_ms"] = (time.perf_counter() - t0) * 1e3
        st = c.read_profile(bases, off, want_counts=False).cpu().numpy().view(np.dtype(A.READ_ABUNDANCE_DTYPE)).reshape(-1)
        assert np.array_equal(st["min"], route[0]) and np.array_equal(st["median"], route[1]) and np.array_equal(st["sum"], route[3])
        assert o[-1] == total
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    c.close()
    ctx.close()


if __name__ == "__main__":
    main()
