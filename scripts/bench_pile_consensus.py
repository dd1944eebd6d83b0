#!/usr/bin/env python3
"""kmu_pile_ins_plan, kmu_chain_pile_ins and kmu_pile_consensus timed: the corrected reads of the workload of
scripts/bench_chain_pileup.py.

Device-resident ONT-shaped reads (kmerutils_amd.synth: 8 % errors), k = 21, w = 10, KMU_FHASH_CANON_INVHASH; chains with max_gap
5000, band 500, min_seeds 3, each read pair once; their records and runs at band 64; the self-join's table and its calls at
min_depth 3.  On the resident reads, records, runs, table and calls:
  pileup           Context.chain_pileup into a zeroed table of its own: the yardstick of the votes
  pile_call        Context.pile_call on that table: the yardstick of the passes over the rows
  ins_plan         Context.pile_ins_plan (max_ins 16)
  pile_ins         Context.chain_pile_ins into a zeroed slot table of its own: both sides, the self-join's one table
  consensus        Context.pile_consensus: one call, the output sized by n_bases + n_slots
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max.  Then one profiled
run of each: the device time of every kernel (kmu_profile_get); the rows with slots, the slots, the voted letters; the bytes each
kernel must move and the bandwidth that is of its time.  One JSON line.

  scripts/bench_pile_consensus.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--max-ins 16] [--out FILE]
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
    ap.add_argument("--max-ins", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import lib, minimizer, synth
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds, band, min_depth = 21, 10, 5000, 500, 3, 64, 3
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    n_bases = int(off[-1].item())
    res = {"reads": args.reads, "bases": n_bases, "k": k, "w": w, "max_gap": max_gap, "band_chain": band_chain, "min_seeds": min_seeds,
           "band": band, "min_depth": min_depth, "max_ins": args.max_ins, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

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
    plain = ctx.chain_align(chains, bases, off, band=band)
    aln, ops, op_off = ctx.chain_cigar(chains, bases, off, band=band, aln=plain)
    table = ctx.chain_pileup(chains, aln, ops, op_off, bases, off)[0]
    call, summary = ctx.pile_call(table, bases, off, min_depth=min_depth)
    ins_len, n_slots = ctx.pile_ins_plan(table, call, max_ins=args.max_ins)
    ins = ctx.chain_pile_ins(chains, aln, ops, op_off, bases, off, ins_len, n_slots)[0]
    cons, coff = ctx.pile_consensus(table, call, ins_len, n_slots, ins, bases, off)

    routes = {"pileup": lambda: ctx.chain_pileup(chains, aln, ops, op_off, bases, off),
              "pile_call": lambda: ctx.pile_call(table, bases, off, min_depth=min_depth),
              "ins_plan": lambda: ctx.pile_ins_plan(table, call, max_ins=args.max_ins),
              "pile_ins": lambda: ctx.chain_pile_ins(chains, aln, ops, op_off, bases, off, ins_len, n_slots),
              "consensus": lambda: ctx.pile_consensus(table, call, ins_len, n_slots, ins, bases, off)}
    for f in routes.values():  # warm-up
        timed(f)
    t = {n: [] for n in routes}
    for _ in range(args.repeats):
        for n, f in routes.items():
            t[n].append(timed(f)[0])
    res.update({"chains": int(chains.shape[0]), "runs": int(ops.shape[0]), "ms": {name: stat(v) for name, v in t.items()}})

    def profiled(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        ctx.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        return {name: round(v[1], 4) for name, v in prof.items()}
    prof = {name: profiled(f) for name, f in routes.items()}
    res["kernels_ms"] = prof

    h_len = ins_len.cpu().numpy()
    h_call = call.cpu().numpy()
    rows_with_slots = int((h_len > 0).sum())
    votes = int((ins.long() & 0xFFFFFFFF).sum().item())
    h_ops = ops.cpu().numpy().view(np.uint32)
    h_off = op_off.cpu().numpy().view(np.uint64).astype(np.int64)
    gap_runs = int((((h_ops & 15) == 1) | ((h_ops & 15) == 2)).sum())
    tiles = int(((h_off[1:] - h_off[:-1] + 63) // 64).sum())
    n_blocks = (n_bases + 63) // 64
    n_cons = int(cons.shape[0])
    must = {
        # call byte in, ins_len byte out; the 32-byte row behind KMU_CALL_INS
        "k_ins_plan": 2 * n_bases + 32 * int(((h_call & 8) != 0).sum()),
        # the bytes in, a block sum out
        "k_ins_blocks": n_bases + 4 * n_blocks,
        # runs and tile records; one ins_len byte per gap run and side; a letter and a 4-byte count read and written per vote
        "k_ins_vote": 4 * h_ops.size + 16 * tiles + 2 * gap_runs + 9 * votes,
        # call and ins_len per row; the pile row and the slots of the rows that have slots; a tile sum out
        "k_cons_count": 2 * n_bases + 32 * rows_with_slots + 16 * n_slots + 4 * n_blocks,
        # the same and the read's own byte, the output bytes
        "k_cons_write": 3 * n_bases + 32 * rows_with_slots + 16 * n_slots + n_cons,
    }

    def gbps(kernel, route):
        ms = prof[route].get(kernel, 0.0)
        return must[kernel] / (ms * 1e-3) / 1e9 if ms else 0.0
    res["consensus"] = {"rows_with_call_ins": int(((h_call & 8) != 0).sum()), "rows_with_slots": rows_with_slots, "slots": n_slots, "votes": votes,
                        "gap_runs": gap_runs, "tiles": tiles, "cons_bases": n_cons, "bytes_must_move": must,
                        "GBps_of_must_move": {"k_ins_plan": gbps("k_ins_plan", "ins_plan"), "k_ins_blocks": gbps("k_ins_blocks", "pile_ins"),
                                              "k_ins_vote": gbps("k_ins_vote", "pile_ins"), "k_cons_count": gbps("k_cons_count", "consensus"),
                                              "k_cons_write": gbps("k_cons_write", "consensus")},
                        "covered_share": float(summary.cpu().numpy().view(np.uint32)[:, 1].sum()) / max(n_bases, 1)}
    res["pile_ins_over_pileup"] = res["ms"]["pile_ins"]["median"] / res["ms"]["pileup"]["median"]
    res["consensus_over_pile_call"] = res["ms"]["consensus"]["median"] / res["ms"]["pile_call"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
