#!/usr/bin/env python3
"""The count prefilter, timed against the plain count of the same reads in the same build.

Device-resident ONT-shaped synthetic reads (kmerutils_amd.synth.ont_reads_device), Kmer64bit k = 31, 8-bit counters.  Host clock
around synchronous calls on the context's stream, median / min / max of --repeats runs after a warm-up:
  filter_build_ms   kmu_kfilter_add_reads into an empty filter of --filter-bits bits per k-mer occurrence
  size_query_ms     kmu_kfilter_select_reads, kmers_out == NULL: the number P of occurrences that pass
  filtered_add_ms   kmu_count_add_reads_filtered into an empty table made for P k-mers
  plain_add_ms      kmu_count_add_reads of the same reads into an empty table made for every occurrence
and, once: the bytes of table + filter against the bytes of the plain table, the distinct k-mers each holds, the singletons that
slipped through, and the relative error of the filter's estimate of the distinct k-mers.  One JSON line, also written to --out.

  scripts/bench_kfilter.py [--reads 25000] [--bases 250000000] [--genome 50000000] [--filter-bits 16] [--hashes 4] [--repeats 5] [--out FILE]
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
    ap.add_argument("--reads", type=int, default=25_000)
    ap.add_argument("--bases", type=int, default=250_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--filter-bits", type=int, default=16)
    ap.add_argument("--hashes", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, synth
    dev = torch.device("cuda", 0)
    k = 31
    bases, off, lens = synth.ont_reads_device(args.reads, args.bases, args.genome, 0xC4, dev)
    occurrences = int(np.maximum(lens - k + 1, 0).sum())
    ctx = lib.Context(0)

    def timed(fn, before=None):
        ts = []
        for i in range(args.repeats + 1):  # (the first run warms up: workspaces, the table's pages)
            if before:
                before()
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        return stat(ts)

    f = ctx.kfilter(A.KMER64BIT, k, lib.kfilter_cells_for(occurrences, args.filter_bits), args.hashes)
    res = {"reads": args.reads, "bases": int(lens.sum()), "occurrences": occurrences, "genome": args.genome, "filter_bits": args.filter_bits,
           "hashes": args.hashes, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    res["filter_build_ms"] = timed(lambda: f.add_reads(bases, off), before=f.reset)
    info = f.info()
    assert info["n_added"] == occurrences
    passing = f.n_passing(bases, off)
    res["size_query_ms"] = timed(lambda: f.n_passing(bases, off))
    filtered = ctx.counter(A.KMER64BIT, k, 8, max(passing, 1024))
    res["filtered_add_ms"] = timed(lambda: filtered.add_reads_filtered(f, bases, off), before=filtered.reset)
    plain = ctx.counter(A.KMER64BIT, k, 8, max(occurrences, 1024))
    res["plain_add_ms"] = timed(lambda: plain.add_reads(bases, off), before=plain.reset)
    distinct = plain.nb_distinct()
    repeated = distinct - plain.nb_unique()
    held, slipped = filtered.nb_distinct(), filtered.nb_unique()
    assert held - slipped == repeated and filtered.nb_occurrences() == passing  # every repeated k-mer is held, nothing else but slips
    res.update({"passing": passing, "distinct": distinct, "repeated": repeated, "held": held, "slipped": slipped,
                "filter_bytes": info["bytes"], "filtered_table_bytes": filtered.table_bytes(), "plain_table_bytes": plain.table_bytes(),
                "bits_a": info["bits_a"], "bits_b": info["bits_b"], "est_distinct": info["est_distinct"],
                "est_distinct_rel_err": info["est_distinct"] / distinct - 1.0})
    res["bytes_ratio"] = (res["filtered_table_bytes"] + res["filter_bytes"]) / res["plain_table_bytes"]
    res["two_pass_over_plain"] = ((res["filter_build_ms"]["median"] + res["size_query_ms"]["median"] + res["filtered_add_ms"]["median"])
                                  / res["plain_add_ms"]["median"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    for x in (filtered, plain, f):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
