#!/usr/bin/env python3
"""kmu_chain_pileup and kmu_pile_call timed: the pileup of every read of the workload of scripts/bench_chain_cigar.py.

Device-resident ONT-shaped reads (kmerutils_amd.synth: 8 % errors), k = 21, w = 10, KMU_FHASH_CANON_INVHASH; chains with max_gap
5000, band 500, min_seeds 3, each read pair once; their records and runs at band 64.  On the resident reads, records and runs:
  cigar_one_call   Context.chain_cigar(aln=...): the step the pileup follows, the yardstick
  pileup           Context.chain_pileup into a zeroed table of its own: both sides, the self-join's one table
  pile_call        Context.pile_call on that table: calls and read summaries
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max.  Then one profiled
run of each: the device time of every kernel (kmu_profile_get); the votes (columns on both sides, run votes, ends), the votes per
second of k_pile_vote, the bytes it must move (runs and tile records read, letters read, 32-byte rows touched once) against the
4.1 TB/s the project measures elsewhere, and the atomic adds per second it reaches -- a measured rate, not a known roof; the vote
kernel with one side at a time (the same columns walked, half the letter votes); and the chain with the most runs on its own.
  host      for context: the records and runs brought to the host, and the reference of tests/test_pileup_abi.py
            (reference_pileup: one replay loop per chain in numpy) on the chains whose read_a is below --host-reads, run once and
            compared with the device's table of the same chains.
One JSON line.

  scripts/bench_chain_pileup.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--host-reads 200] [--out FILE]
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
    from test_pileup_abi import reference_pileup
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds, band = 21, 10, 5000, 500, 3, 64
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    n_bases = int(off[-1].item())
    res = {"reads": args.reads, "bases": n_bases, "k": k, "w": w, "max_gap": max_gap, "band_chain": band_chain, "min_seeds": min_seeds,
           "band": band, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    q = minimizer.read_minimizers(ctx, bases, off, k, w)
    pairs = minimizer.seed_pairs(ctx, q)
    chains = ctx.seed_chains(pairs, q, None, span=k, max_gap=max_gap, band=band_chain, min_seeds=min_seeds, max_pos=int(lens.max()), upper=True)
    n_chains = int(chains.shape[0])
    plain = ctx.chain_align(chains, bases, off, band=band)
    aln, ops, op_off = ctx.chain_cigar(chains, bases, off, band=band, aln=plain)
    table = ctx.chain_pileup(chains, aln, ops, op_off, bases, off)[0]

    routes = {"cigar_one_call": lambda: ctx.chain_cigar(chains, bases, off, band=band, aln=plain),
              "pileup": lambda: ctx.chain_pileup(chains, aln, ops, op_off, bases, off),
              "pile_call": lambda: ctx.pile_call(table, bases, off)}
    for f in routes.values():  # warm-up
        timed(f)
    t = {n: [] for n in routes}
    for _ in range(args.repeats):
        for n, f in routes.items():
            t[n].append(timed(f)[0])
    res.update({"chains": n_chains, "runs": int(ops.shape[0]), "ms": {name: stat(v) for name, v in t.items()}})

    def profiled(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = fn()
        ctx.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        return out, {name: round(v[1], 4) for name, v in prof.items()}

    _, prof_cigar = profiled(routes["cigar_one_call"])
    _, prof_pile = profiled(routes["pileup"])
    (call, summary), prof_call = profiled(routes["pile_call"])
    h_ops = ops.cpu().numpy().view(np.uint32)
    h_off = op_off.cpu().numpy().view(np.uint64).astype(np.int64)
    rec = chains.cpu().numpy().view(np.uint32).reshape(-1, 10)
    length, op = (h_ops >> 4).astype(np.int64), h_ops & 15
    diag = int(length[(op == 7) | (op == 8)].sum())
    gap_cols, gap_runs = int(length[(op == 1) | (op == 2)].sum()), int(((op == 1) | (op == 2)).sum())
    adds = 2 * diag + gap_cols + 2 * gap_runs + 4 * n_chains  # atomic adds: a diagonal column votes on both sides, a gap run adds INS and INS_BASES
    tiles = int(((h_off[1:] - h_off[:-1] + 63) // 64).sum())
    touched = int((table[:, :5].sum(dim=1) > 0).sum().item())
    must_move = 4 * h_ops.size + 16 * tiles + 2 * diag + 2 * 32 * touched  # runs, tile records, letters, rows read and written once
    vote_s = prof_pile.get("k_pile_vote", 0.0) * 1e-3
    res["pileup"] = {"kernels_ms": prof_pile, "tiles": tiles, "columns": diag + gap_cols, "columns_per_run": (diag + gap_cols) / max(h_ops.size, 1),
                     "atomic_adds": adds, "rows_touched": touched, "bytes_must_move": must_move,
                     "vote_adds_per_s": adds / vote_s if vote_s else 0.0, "vote_columns_per_s": (diag + gap_cols) / vote_s if vote_s else 0.0,
                     "vote_ms_at_4100_GBps": must_move / 4.1e12 * 1e3, "vote_GBps_of_must_move": must_move / vote_s / 1e9 if vote_s else 0.0}
    res["pile_call"] = {"kernels_ms": prof_call, "bytes": 33 * n_bases + n_bases + 32 * args.reads,
                        "covered_share": float(summary.cpu().numpy().view(np.uint32)[:, 1].sum()) / max(n_bases, 1),
                        "diff_share_of_covered": float(summary.cpu().numpy().view(np.uint32)[:, 2].sum()) /
                        max(float(summary.cpu().numpy().view(np.uint32)[:, 1].sum()), 1.0)}
    # one side at a time: the same columns walked, half the letter votes
    for name, side in (("q_only", A.PILE_Q), ("db_only", A.PILE_DB)):
        _, prof_side = profiled(lambda side=side: ctx.chain_pileup(chains, aln, ops, op_off, bases, off, sides=side))
        res["pileup"]["k_pile_vote_ms_" + name] = prof_side.get("k_pile_vote", 0.0)
    res["cigar_one_call_kernels_ms"] = prof_cigar
    res["pileup_over_cigar"] = res["ms"]["pileup"]["median"] / res["ms"]["cigar_one_call"]["median"]

    # the tail: the chain with the most runs on its own
    if n_chains:
        longest = int(np.argmax(h_off[1:] - h_off[:-1]))
        lo, hi = int(h_off[longest]), int(h_off[longest + 1])
        one = (chains[longest:longest + 1].contiguous(), aln[longest:longest + 1].contiguous(), ops[lo:hi].contiguous(),
               torch.tensor([0, hi - lo], dtype=torch.int64, device=dev))
        timed(lambda: ctx.chain_pileup(*one, bases, off))
        ms_one, _ = timed(lambda: ctx.chain_pileup(*one, bases, off))
        _, prof_one = profiled(lambda: ctx.chain_pileup(*one, bases, off))
        res["longest_chain_alone"] = {"m": int(rec[longest, 7] - rec[longest, 6]), "n": int(rec[longest, 9] - rec[longest, 8]), "runs": hi - lo,
                                      "tiles": (hi - lo + 63) // 64, "kernels_ms": prof_one, "ms_with_the_table": ms_one}

    # the host route on a sub-sample: the records and runs to the host, then numpy and a Python loop, run once
    t0 = time.perf_counter()
    h_chains = chains.cpu().numpy().view(np.uint32).reshape(-1, 10)
    h_aln = aln.cpu().numpy().view(np.uint32).reshape(-1, 4)
    h_runs, h_roff = ops.cpu().numpy().view(np.uint32), op_off.cpu().numpy().view(np.uint64)
    h_bases, h_boff = bases.cpu().numpy(), off.cpu().numpy().view(np.uint64)
    copy_ms = (time.perf_counter() - t0) * 1e3
    sub = np.nonzero(h_chains[:, 0] < args.host_reads)[0]
    s_chains = np.ascontiguousarray(h_chains[sub]).view(np.dtype(A.CHAIN_DTYPE)).reshape(-1)
    s_aln = np.ascontiguousarray(h_aln[sub]).view(np.dtype(A.CHAIN_ALN_DTYPE)).reshape(-1)
    parts = [h_runs[int(h_roff[c]):int(h_roff[c + 1])] for c in sub.tolist()]
    s_off = np.zeros(sub.size + 1, np.uint64)
    s_off[1:] = np.cumsum([p.size for p in parts])
    s_ops = np.concatenate(parts) if parts else h_runs[:0]
    t0 = time.perf_counter()
    want = reference_pileup(s_chains, s_aln, s_ops, s_off, h_bases, h_boff)[0]
    host_ms = (time.perf_counter() - t0) * 1e3
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)  # noqa: E731
    got = ctx.chain_pileup(d(s_chains, np.int32).reshape(-1, 10), d(s_aln, np.int32).reshape(-1, 4), d(s_ops, np.int32), d(s_off, np.int64), bases, off)[0]
    res["host"] = {"reads": args.host_reads, "chains": int(sub.size), "runs": int(s_ops.size), "copy_to_host_ms": copy_ms,
                   "ms_numpy_and_python": host_ms, "tables_equal_on_the_sub_sample": bool(np.array_equal(got.cpu().numpy().view(np.uint32), want))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
