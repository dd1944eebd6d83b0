#!/usr/bin/env python3
"""kmu_seed_chains timed: from device-resident reads to one base-resolution chain per read pair.

Device-resident ONT-shaped reads (kmerutils_amd.synth), k = 21, w = 10, KMU_FHASH_CANON_INVHASH; max_gap 5000, band 500,
min_seeds 3, each read pair once.
  device    minimizer.read_minimizers -> minimizer.seed_pairs -> Context.seed_chains on the resident arrays, each step timed on
            its own and the three together; only the records would leave the device
  host      the route without kmu_seed_chains: the entry pairs and the minimizer arrays copied to the host, then the reference of
            tests/test_chains_abi.py (reference_chains: the contract in plain Python).  Its DP is a Python loop, so it runs on the
            pairs whose read_a is below --host-reads only; the time is reported for that sub-sample, with its share of the pairs,
            and its records are compared with the device's records of the same reads.
  slices    context, on the same reads: Context.read_anchors (nbkmer 16, window 500 / overlap 250) is not timed; anchor_match as a
            self-join and anchor_overlaps (strands 2, band 1, min_score 2) are -- the slice-resolution route to read pairs.
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max, and the device
time of the kernels of one seed_chains call (kmu_profile_get).  One JSON line.

  scripts/bench_chains.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--host-reads 200] [--out FILE]
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
    from kmerutils_amd import anchor, lib, minimizer, synth
    from test_chains_abi import reference_chains
    dev = torch.device("cuda", 0)
    k, w, max_gap, band, min_seeds = 21, 10, 5000, 500, 3
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    res = {"reads": args.reads, "bases": int(off[-1].item()), "k": k, "w": w, "max_gap": max_gap, "band": band, "min_seeds": min_seeds,
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

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

    def chains():
        return ctx.seed_chains(pairs, q, None, span=k, max_gap=max_gap, band=band, min_seeds=min_seeds, max_pos=max_pos, upper=True)

    def whole():
        return minimizer.read_chains(ctx, bases, off, k, w, max_gap=max_gap, band=band, min_seeds=min_seeds)

    # the slice-resolution route on the same reads
    params = anchor.AnchorsGeneratorParameters("bench", 500, 16, k, 250)
    p = params.sketch_params()
    p.mem = A.MEM_DEVICE
    p.fhash = A.FHASH_CANON_VALUE
    hashes, _, _, row_off = ctx.read_anchors(bases, off, p, 500, 250, want_counts=False)
    hashes = hashes.contiguous()
    group = torch.from_numpy(np.repeat(np.arange(args.reads, dtype=np.uint32), np.diff(row_off.astype(np.int64))).view(np.int32)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(row_off.astype(np.uint64)).view(np.int64)).to(dev)

    def slices():
        sp, sd = ctx.anchor_match(hashes, hashes, n_keys=4, min_common=1, group_q=group, group_db=group)
        return ctx.anchor_overlaps(sp, sd, d_off, strands=2, band=1, min_score=2, upper=True)

    # the host route on a sub-sample of the reads
    def host():
        hp = pairs.cpu().numpy().view(np.uint32)
        hq = minimizer.Minimizers(*[x.cpu().numpy().view({8: np.uint64, 4: np.uint32, 1: np.uint8}[x.element_size()]) for x in q[:5]], k, w, q.fhash)
        sub = hp[hq.read[hp[:, 0]] < args.host_reads]
        return sub.shape[0], reference_chains(sub, hq, hq, k, max_gap, band, min_seeds=min_seeds, upper=True)

    routes = {"minimizers": minimizers, "seed_pairs": pairs_of, "seed_chains": chains, "read_chains": whole, "slices": slices, "host": host}
    for f in routes.values():  # warm-up
        timed(f)
    t = {n: [] for n in routes}
    for _ in range(args.repeats):
        for n, f in routes.items():
            t[n].append(timed(f)[0])
    rec = chains().cpu().numpy().view(np.uint32).reshape(-1, 10)
    n_sub, want = host()
    want = want.view(np.uint32).reshape(-1, 10)
    ctx.profile_enable(True)
    ctx.profile_reset()
    chains()
    ctx.synchronize()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    res.update({"minimizers": int(q.hashes.numel()), "pairs": int(pairs.shape[0]), "chains": int(rec.shape[0]),
                "overlaps_by_slices": int(slices().shape[0]), "host_reads": args.host_reads, "host_pairs": int(n_sub),
                "host_share_of_pairs": n_sub / max(int(pairs.shape[0]), 1),
                "records_equal_on_the_sub_sample": bool(np.array_equal(rec[rec[:, 0] < args.host_reads], want)),
                "seeds_per_chain_median": float(np.median(rec[:, 4])) if rec.shape[0] else 0.0,
                "largest_group": int(rec[:, 5].max()) if rec.shape[0] else 0,
                "ms": {n: stat(v) for n, v in t.items()},
                "kernels_ms": {n: round(v[1], 4) for n, v in prof.items() if v[0]}})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
