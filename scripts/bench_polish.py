#!/usr/bin/env python3
"""kmu_sg_unitig_chains and the stages of minimizer.polish_unitigs timed on resident data.

  sparse, dense   the two workloads of scripts/bench_unitigs.py (same reads, same chains, same graph parameters): the layout of
                  sg_unitigs on the graph of sg_graph, the draft of sg_unitig_seqs, the self-join and its classes
On the resident data, each stage on the outputs of the one before it:
  sg_unitig_chains   Context.sg_unitig_chains (the map)
  cigar, pileup, call, ins_plan, insertions, consensus, positions
                     the stages of polish_unitigs, the unitig batch as the q side, the reads as the db side, votes with A.PILE_Q
  polish_unitigs     the composition, one round
Host clock around synchronised calls; a warm-up of each, then --repeats runs; median / min / max.  The map's counts, the share of
its records whose alignment carries A.ALN_EXACT at the band, and the launches and device time of the map's kernels
(kmu_profile_get).  One JSON line.

  scripts/bench_polish.py [--reads 20000] [--mean-len 5000] [--dense-genome 1000000] [--dense-cov 30] [--dense-len 5000] [--fuzz 100]
                          [--band 64] [--repeats 5] [--only sparse|dense] [--out FILE]
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
    ap.add_argument("--dense-genome", type=int, default=1_000_000)
    ap.add_argument("--dense-cov", type=int, default=30)
    ap.add_argument("--dense-len", type=int, default=5000)
    ap.add_argument("--fuzz", type=int, default=100)
    ap.add_argument("--band", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=("sparse", "dense"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer, synth
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds = 21, 10, 5000, 500, 3
    graph = dict(min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=700, fuzz=args.fuzz)
    ctx = lib.Context(0)
    res = {"k": k, "w": w, "band": args.band, "graph": graph, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def measured(fn):
        timed(fn)  # warm-up
        runs = [timed(fn) for _ in range(args.repeats)]
        return stat([t for t, _ in runs]), runs[-1][1]

    def workload(name, bases, off):
        chains, aln = minimizer.read_alignments(ctx, bases, off, k, w, max_gap=max_gap, band_chain=band_chain, min_seeds=min_seeds, band=args.band)
        arcs, _, classes, reads = ctx.sg_graph(chains, aln, off, **graph)
        unitigs, path, place = ctx.sg_unitigs(arcs, reads, off)
        seq, seq_off = ctx.sg_unitig_seqs(unitigs, path, bases, off)
        print("%s: %d reads, %d chains, %d unitigs" % (name, int(off.shape[0]) - 1, int(chains.shape[0]), int(unitigs.shape[0])), file=sys.stderr, flush=True)
        ms = {}
        ms["sg_unitig_chains"], (records, counts) = measured(lambda: ctx.sg_unitig_chains(unitigs, path, place, chains, classes, off))
        ms["cigar"], (r_aln, ops, op_off) = measured(lambda: minimizer.cigar_chains(ctx, records, seq, seq_off, bases, off, band=args.band))
        ms["pileup"], (pile, _) = measured(lambda: minimizer.pileup_chains(ctx, records, r_aln, ops, op_off, seq, seq_off, bases, off, sides=A.PILE_Q))
        ms["call"], (call, _) = measured(lambda: ctx.pile_call(pile, seq, seq_off, min_depth=2))
        ms["ins_plan"], (ins_len, n_slots) = measured(lambda: ctx.pile_ins_plan(pile, call, max_ins=16))
        ms["insertions"], (ins, _) = measured(lambda: minimizer.insertions_chains(ctx, records, r_aln, ops, op_off, seq, seq_off, ins_len, n_slots,
                                                                                 bases, off, sides=A.PILE_Q))
        ms["consensus"], (cons, cons_off) = measured(lambda: minimizer.consensus_reads(ctx, pile, call, ins_len, n_slots, ins, seq, seq_off))
        ms["positions"], _ = measured(lambda: minimizer._polished_coordinates(ctx, (pile, call, ins_len, n_slots, ins), seq, seq_off, cons_off, path,
                                                                             place, records))
        ms["polish_unitigs"], _ = measured(lambda: minimizer.polish_unitigs(ctx, unitigs, path, place, seq, seq_off, bases, off, chains, classes,
                                                                            band=args.band))
        flags = r_aln[:, 3].cpu().numpy().astype(np.int64)
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.sg_unitig_chains(unitigs, path, place, chains, classes, off)
        ctx.synchronize()
        kernels = {n: {"launches": v[0], "ms": round(v[1], 4)} for n, v in ctx.profile_get().items()}
        ctx.profile_enable(False)
        res[name] = {"reads": int(off.shape[0]) - 1, "chains": int(chains.shape[0]), "unitigs": int(unitigs.shape[0]), "draft_bytes": int(seq.shape[0]),
                     "polished_bytes": int(cons.shape[0]), "map": counts, "records": int(records.shape[0]),
                     "share_exact": float(((flags & A.ALN_EXACT) != 0).mean()) if len(flags) else None,
                     "share_path": float(((flags & A.ALN_PATH) != 0).mean()) if len(flags) else None, "ms": ms, "kernels": kernels}

    if args.only != "dense":
        bases, off, _ = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
        workload("sparse", bases, off)
        del bases, off
    if args.only != "sparse":
        n_dense = args.dense_genome * args.dense_cov // args.dense_len
        h_bases, h_off = synth.genome_reads(n_dense, np.full(n_dense, args.dense_len), args.dense_genome, 0xD5, sub=0.04, ins=0.02, dele=0.02)
        workload("dense", torch.from_numpy(h_bases).to(dev), torch.from_numpy(h_off.astype(np.int64)).to(dev))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
