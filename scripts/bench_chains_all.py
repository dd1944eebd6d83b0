#!/usr/bin/env python3
"""kmu_seed_chains_all and kmu_chain_rank timed beside kmu_seed_chains on the same hits.

The workload of scripts/bench_chains.py: device-resident ONT-shaped reads (kmerutils_amd.synth), k = 21, w = 10,
KMU_FHASH_CANON_INVHASH, the self-join's entry pairs; max_gap 5000, band 500, min_seeds 3, each read pair once.
  seed_chains       Context.seed_chains on the resident pairs: one chain per read pair
  seed_chains_all   Context.seed_chains_all on the same pairs: every chain of every group
  chain_rank        Context.chain_rank on the records of seed_chains_all (mask 500 permille)
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max, the device time
of the kernels of one call of each entry (kmu_profile_get), and the number of chains each entry reports.  On --check-reads reads
the records of both new entries are compared with the references of tests/test_chains_all_abi.py.  One JSON line.

  scripts/bench_chains_all.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--check-reads 100] [--out FILE]
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
    ap.add_argument("--check-reads", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import lib, minimizer, synth
    from test_chains_all_abi import reference_chains_all, reference_rank
    dev = torch.device("cuda", 0)
    k, w, max_gap, band, min_seeds, mask = 21, 10, 5000, 500, 3, 500
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    res = {"reads": args.reads, "bases": int(off[-1].item()), "k": k, "w": w, "max_gap": max_gap, "band": band, "min_seeds": min_seeds,
           "mask_permille": mask, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    q = minimizer.read_minimizers(ctx, bases, off, k, w)
    max_pos = int(lens.max())
    pairs = minimizer.seed_pairs(ctx, q)
    kw = dict(span=k, max_gap=max_gap, band=band, min_seeds=min_seeds, max_pos=max_pos, upper=True)

    def one():
        return ctx.seed_chains(pairs, q, None, **kw)

    def every():
        return ctx.seed_chains_all(pairs, q, None, **kw)

    all_rec = every()

    def rank():
        return ctx.chain_rank(all_rec, args.reads, mask)

    routes = {"seed_chains": one, "seed_chains_all": every, "chain_rank": rank}
    for f in routes.values():  # warm-up
        timed(f)
    t = {n: [] for n in routes}
    for _ in range(args.repeats):
        for n, f in routes.items():
            t[n].append(timed(f)[0])
    kernels = {}
    for n, f in routes.items():
        ctx.profile_enable(True)
        ctx.profile_reset()
        f()
        ctx.synchronize()
        kernels[n] = {name: round(v[1], 4) for name, v in ctx.profile_get().items() if v[0]}
        ctx.profile_enable(False)
    host = lambda x: x.cpu().numpy().view({8: np.uint64, 4: np.uint32, 1: np.uint8}[x.element_size()])  # noqa: E731
    one_rec = host(one()).reshape(-1, 10)
    rec = host(all_rec).reshape(-1, 10)
    rk = host(rank()).reshape(-1, 4)
    # the references on the pairs of the first reads
    hp = host(pairs)
    hq = minimizer.Minimizers(*[host(x) for x in q[:5]], k, w, q.fhash)
    sub = hp[hq.read[hp[:, 0]] < args.check_reads]
    want = reference_chains_all(sub, hq, hq, k, max_gap, band, min_seeds=min_seeds, upper=True)
    mine = rec[rec[:, 0] < args.check_reads]
    dt = np.dtype([(n, "<u4") for n in ("read_a", "read_b", "strand", "score", "n_seeds", "n_anchors", "a_start", "a_end", "b_start", "b_end")])
    want_rank = reference_rank(np.ascontiguousarray(mine).view(dt).reshape(-1), args.reads, mask)
    per_read = np.bincount(rec[:, 0].astype(np.int64), minlength=args.reads)
    res.update({"pairs": int(pairs.shape[0]), "chains": int(one_rec.shape[0]), "chains_all": int(rec.shape[0]),
                "primary": int((rk[:, 1] == np.arange(rk.shape[0])).sum()), "most_chains_of_a_read": int(per_read.max()),
                "check_reads": args.check_reads, "check_pairs": int(sub.shape[0]),
                "records_equal_on_the_sub_sample": bool(np.array_equal(mine, want.view(np.uint32).reshape(-1, 10))),
                "ranks_equal_on_the_sub_sample": bool(np.array_equal(rk[:mine.shape[0]], want_rank.view(np.uint32).reshape(-1, 4))),
                "every_one_per_pair_record_is_among_all": bool(set(map(tuple, one_rec.tolist())) <= set(map(tuple, rec.tolist()))),
                "ms": {n: stat(v) for n, v in t.items()}, "kernels_ms": kernels})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
