#!/usr/bin/env python3
"""kmu_chain_align timed: the banded alignment of every chain of the workload of scripts/bench_chains.py.

Device-resident ONT-shaped reads (kmerutils_amd.synth: 8 % errors), k = 21, w = 10, KMU_FHASH_CANON_INVHASH; chains with max_gap
5000, band 500, min_seeds 3, each read pair once.
  device    Context.chain_align over all chains at band 64 and at band 256, on the resident reads and records; beside it, in the
            same run, read_minimizers, seed_pairs and seed_chains.  Only the 16-byte records would leave the device.
  host      the route without kmu_chain_align: reads and records copied to the host, then the reference of
            tests/test_chain_align_abi.py (reference_align: the contract in numpy, one Python loop over the anti-diagonals of a
            chain) at band 64 on the chains whose read_a is below --host-reads, run once; the time is reported for that sub-sample
            and scaled by its share of the cells, and its records are compared with the device's.
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max; the device time of
k_chain_align (kmu_profile_get) and, from it, cells per second: the sum of (m + n + 1) * n_diags / 2 over the chains with
ALN_DONE; and the device time of the chain with the most anti-diagonals aligned on its own (the tail).  One JSON line.

  scripts/bench_chain_align.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--host-reads 200] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--mean-len", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-reads", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer, synth
    from test_chain_align_abi import reference_align
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds = 21, 10, 5000, 500, 3
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    res = {"reads": args.reads, "bases": int(off[-1].item()), "k": k, "w": w, "max_gap": max_gap, "band_chain": band_chain,
           "min_seeds": min_seeds, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def minimizers():
        return minimizer.read_minimizers(ctx, bases, off, k, w)

    q = minimizers()
    max_pos = int(lens.max())

    def pairs_of():
        return minimizer.seed_pairs(ctx, q)

    pairs = pairs_of()

    def chains_of():
        return ctx.seed_chains(pairs, q, None, span=k, max_gap=max_gap, band=band_chain, min_seeds=min_seeds, max_pos=max_pos, upper=True)

    chains = chains_of()
    routes = {"minimizers": minimizers, "seed_pairs": pairs_of, "seed_chains": chains_of,
              "chain_align_band64": lambda: ctx.chain_align(chains, bases, off, band=64),
              "chain_align_band256": lambda: ctx.chain_align(chains, bases, off, band=256)}
    for f in routes.values():  # warm-up
        timed(f)
    t = {n: [] for n in routes}
    for _ in range(args.repeats):
        for n, f in routes.items():
            t[n].append(timed(f)[0])

    rec = chains.cpu().numpy().view(np.uint32).reshape(-1, 10)
    m, n = (rec[:, 7] - rec[:, 6]).astype(np.int64), (rec[:, 9] - rec[:, 8]).astype(np.int64)
    res.update({"minimizers": int(q.hashes.numel()), "pairs": int(pairs.shape[0]), "chains": int(rec.shape[0]),
                "segment_bases_median": float(np.median(np.maximum(m, n))) if rec.shape[0] else 0.0,
                "segment_bases_max": int(np.maximum(m, n).max()) if rec.shape[0] else 0, "ms": {name: stat(v) for name, v in t.items()}})
    alns = {}
    for band in (64, 256):
        ctx.profile_enable(True)
        ctx.profile_reset()
        aln = ctx.chain_align(chains, bases, off, band=band)
        ctx.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        aln = aln.cpu().numpy().view(np.uint32).reshape(-1, 4)
        alns[band] = aln
        done = (aln[:, 3] & A.ALN_DONE) != 0
        cells = float(((m + n + 1) * aln[:, 2].astype(np.int64))[done].sum()) / 2
        dev_ms = prof["k_chain_align"][1]
        res["band%d" % band] = {"share_done": float(done.mean()) if done.size else 0.0,
                                "share_exact": float(((aln[:, 3] & A.ALN_EXACT) != 0).mean()) if done.size else 0.0,
                                "k_chain_align_ms": round(dev_ms, 4), "cells": cells, "cells_per_s": cells / (dev_ms * 1e-3) if dev_ms else 0.0,
                                "edit_over_block_median": float(np.median(aln[done, 0] / np.maximum(aln[done, 0] + aln[done, 1], 1))) if done.any() else 0.0}

    # the tail: the chain with the most anti-diagonals on its own -- one wave's sequential work, a floor of the whole call
    if rec.shape[0]:
        longest = int(np.argmax(m + n))
        one = chains[longest:longest + 1].contiguous()
        timed(lambda: ctx.chain_align(one, bases, off, band=64))
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.chain_align(one, bases, off, band=64)
        ctx.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        res["longest_chain_alone"] = {"m": int(m[longest]), "n": int(n[longest]), "n_diags": int(alns[64][longest, 2]),
                                      "k_chain_align_ms": round(prof["k_chain_align"][1], 4)}

    # the host route on a sub-sample of the reads: a Python loop, run once
    h_bases, h_off = bases.cpu().numpy(), off.cpu().numpy().view(np.uint64)
    sub = rec[:, 0] < args.host_reads
    h_chains = np.ascontiguousarray(rec[sub]).view(np.dtype(A.CHAIN_DTYPE)).reshape(-1)
    t0 = time.perf_counter()
    want = reference_align(h_chains, h_bases, h_off, band=64)
    host_ms = (time.perf_counter() - t0) * 1e3
    aln = alns[64]
    done = (aln[:, 3] & A.ALN_DONE) != 0
    cells_all = ((m + n + 1) * aln[:, 2].astype(np.int64))[done].sum()
    cells_sub = ((m + n + 1) * aln[:, 2].astype(np.int64))[done & sub].sum()
    res["host"] = {"reads": args.host_reads, "chains": int(sub.sum()), "ms_python_loop": host_ms, "share_of_cells": float(cells_sub / max(cells_all, 1)),
                   "ms_scaled_to_all_chains": host_ms * float(cells_all / max(cells_sub, 1)),
                   "records_equal_on_the_sub_sample": bool(np.array_equal(aln[sub], want.view(np.uint32).reshape(-1, 4)))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
