#!/usr/bin/env python3
"""kmu_read_syncmers timed beside the seed selector it stands next to, and what the seeds are worth downstream.

Device-resident ONT-shaped reads (kmerutils_amd.synth), k = 21, KMU_FHASH_CANON_INVHASH for both widths:
  syncmers      one Context.read_syncmers call (count + write) at (s, t) = (11, 0), closed, and (11, 5), open
  minimizers    one Context.read_minimizers call at w = 10 on the same reads: existing code, the yardstick (2 / 11 of the k-mers, the
                density of the closed syncmers)
  hashes_only   kmu_kmer_hashes alone: every k-mer hashed once and written -- the floor of either kernel
Host clock around synchronised calls; warm-up first, then --repeats runs of each in alternation; median / min / max, and the
device time of the kernels of one call (kmu_profile_get).
Seeds on reads with planted errors (synth.ont_reads: 4 % substitutions, 2 % insertions, 2 % deletions, both strands of one random
genome, --chain-reads reads at about 20-fold coverage): the number of seeds, of seed_pairs and of chains (chain_hits, self-join) from
the closed syncmers, the open syncmers and the minimizers.  One JSON line.

  scripts/bench_syncmers.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--chain-reads 2000] [--out FILE]
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chain-reads", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer, synth
    dev = torch.device("cuda", 0)
    k, kt, fhash, s, w = 21, A.KMER64BIT, A.FHASH_CANON_INVHASH, 11, 10
    bases, off, _ = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    n_bases = int(off[-1].item())
    ctx = lib.Context(0)
    res = {"reads": args.reads, "bases": n_bases, "k": k, "s": s, "w": w, "fhash": "canon_invhash", "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats}
    d_hashes = torch.zeros(n_bases, dtype=torch.int64, device=dev)

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

    runs = {
        "syncmers_closed": lambda: ctx.read_syncmers(bases, off, kt, k, fhash, s, 0),
        "syncmers_open": lambda: ctx.read_syncmers(bases, off, kt, k, fhash, s, 5),
        "minimizers": lambda: ctx.read_minimizers(bases, off, kt, k, fhash, w),
        "hashes_only": lambda: ctx.kmer_hashes(bases, off, kt, k, fhash, out=d_hashes),
    }
    for f in runs.values():  # warm-up: the workspaces grow here
        timed(f)
        timed(f)
    t = {n: [] for n in runs}
    for _ in range(args.repeats):
        for n, f in runs.items():
            t[n].append(timed(f)[0])
    res["ms"] = {n: stat(v) for n, v in t.items()}
    res["kernels_ms"] = {n: kernels_ms(f) for n, f in runs.items()}
    res["seeds"] = {n: int(runs[n]()[0].numel()) for n in ("syncmers_closed", "syncmers_open", "minimizers")}
    res["density"] = {n: v / max(n_bases, 1) for n, v in res["seeds"].items()}
    res["syncmers_closed_over_minimizers"] = res["ms"]["syncmers_closed"]["median"] / res["ms"]["minimizers"]["median"]

    # what the seeds find on noisy reads of one genome
    h_bases, h_off = synth.ont_reads(args.chain_reads, args.chain_reads * args.mean_len // 20, 0xB3, mean_len=args.mean_len)
    c_bases, c_off = torch.from_numpy(h_bases).to(dev), torch.from_numpy(h_off.astype(np.int64)).to(dev)
    seeders = {
        "syncmers_closed": lambda: minimizer.read_syncmers(ctx, c_bases, c_off, k, s, 0),
        "syncmers_open": lambda: minimizer.read_syncmers(ctx, c_bases, c_off, k, s, 5),
        "minimizers": lambda: minimizer.read_minimizers(ctx, c_bases, c_off, k, w),
    }
    res["noisy"] = {"reads": args.chain_reads, "bases": int(h_off[-1]), "errors": "4/2/2 % sub/ins/del"}
    for n, f in seeders.items():
        q = f()
        pairs = minimizer.seed_pairs(ctx, q)
        chains = minimizer.chain_hits(ctx, q)
        res["noisy"][n] = {"seeds": int(q.hashes.numel()), "seed_pairs": int(pairs.shape[0]), "chains": int(chains.shape[0])}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
