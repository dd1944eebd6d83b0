#!/usr/bin/env python3
"""kmu_pile_segments, kmu_pile_consensus_pos and kmu_extract_ranges timed: the trimmed and the corrected-and-trimmed
reads of the workload of scripts/bench_pile_consensus.py.

Device-resident ONT-shaped reads (kmerutils_amd.synth: 8 % errors), k = 21, w = 10, KMU_FHASH_CANON_INVHASH; chains with max_gap
5000, band 500, min_seeds 3, each read pair once; their records and runs at band 64; the self-join's table, its calls, slots and
consensus at min_depth 3, max_ins 16.  On the resident table, calls, slots and consensus:
  pile_call        Context.pile_call on the table: the yardstick of the passes over the rows
  segments         Context.pile_segments (min_depth 3, min_span 3, min_len --min-len)
  pos_extract      Context.pile_consensus_pos of every segment's first row and end row + Context.extract_ranges on the consensus
  trim_raw         minimizer.trim_reads on the table and the raw reads
  correct          minimizer.correct_reads from the reads (the yardstick of the whole route)
  correct_trim     minimizer.correct_trim_reads from the reads
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max.  The host route:
the table and the offsets copied to the host (timed), and the numpy reference of tests/test_trim_abi.py on the first --host-reads
reads (timed; it is a Python loop over the rows).  Then one profiled run of each: the device time of every kernel
(kmu_profile_get), and the bytes the row passes must move with the bandwidth that is of their time.  One JSON line.

  scripts/bench_trim.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--min-len 500] [--host-reads 200] [--out FILE]
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
    ap.add_argument("--min-len", type=int, default=500)
    ap.add_argument("--host-reads", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import lib, minimizer, synth
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds, band, min_depth, max_ins = 21, 10, 5000, 500, 3, 64, 3, 16
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    n_bases = int(off[-1].item())
    res = {"reads": args.reads, "bases": n_bases, "k": k, "w": w, "band": band, "min_depth": min_depth, "min_span": min_depth, "min_len": args.min_len,
           "max_ins": max_ins, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    chains, aln, ops, op_off = minimizer.read_cigars(ctx, bases, off, k, w, max_gap=max_gap, band_chain=band_chain, min_seeds=min_seeds, band=band)
    table = ctx.chain_pileup(chains, aln, ops, op_off, bases, off)[0]
    call, _ = ctx.pile_call(table, bases, off, min_depth=min_depth)
    ins_len, n_slots = ctx.pile_ins_plan(table, call, max_ins=max_ins)
    ins = ctx.chain_pile_ins(chains, aln, ops, op_off, bases, off, ins_len, n_slots)[0]
    cons, _ = ctx.pile_consensus(table, call, ins_len, n_slots, ins, bases, off)
    seg_kw = dict(min_depth=min_depth, min_span=min_depth, min_len=args.min_len)
    segs, seg_off, trims = ctx.pile_segments(table, off, **seg_kw)
    first, last = minimizer._segment_rows(segs, off)
    rows = torch.cat([first, last])
    n_segs = int(segs.shape[0])
    del chains, aln, ops, op_off

    def pos_extract():
        pos = ctx.pile_consensus_pos(table, call, ins_len, n_slots, ins, bases, off, rows)
        return ctx.extract_ranges(cons, pos[:n_segs].contiguous(), pos[n_segs:].contiguous())
    cut = dict(k=k, w=w, max_gap=max_gap, band_chain=band_chain, min_seeds=min_seeds, band=band, min_depth=min_depth, max_ins=max_ins)
    routes = {"pile_call": lambda: ctx.pile_call(table, bases, off, min_depth=min_depth),
              "segments": lambda: ctx.pile_segments(table, off, **seg_kw),
              "segments_longest": lambda: ctx.pile_segments(table, off, longest=True, **seg_kw),
              "pos_extract": pos_extract,
              "trim_raw": lambda: minimizer.trim_reads(ctx, table, bases, off, **seg_kw),
              "correct": lambda: minimizer.correct_reads(ctx, bases, off, **cut),
              "correct_trim": lambda: minimizer.correct_trim_reads(ctx, bases, off, min_span=min_depth, min_len=args.min_len, **cut)}
    for f in routes.values():  # warm-up
        timed(f)
    t = {n: [] for n in routes}
    for _ in range(args.repeats):
        for n, f in routes.items():
            t[n].append(timed(f)[0])
    res["ms"] = {name: stat(v) for name, v in t.items()}

    def profiled(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        ctx.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        return {name: round(v[1], 4) for name, v in prof.items()}
    prof = {name: profiled(routes[name]) for name in ("pile_call", "segments", "segments_longest", "pos_extract", "trim_raw")}
    res["kernels_ms"] = prof

    h_trims = trims.cpu().numpy().view(np.uint32)
    out_bytes = int(pos_extract()[0].shape[0])
    must = {
        # the 32-byte row and the call byte out / the 32-byte row and the read's byte
        "k_pile_call": 34 * n_bases, "k_pile_reads": 33 * n_bases,
        # 24 bytes of every row (the sectors fetched are the row's 32) and a mark bit; the write pass also 16 bytes per run
        "k_seg_count": 32 * n_bases + n_bases // 8, "k_seg_write": 32 * n_bases + n_bases // 8,
        # every output byte read and written, two offsets per range
        "k_ext_copy": 2 * out_bytes + 24 * n_segs,
    }

    def gbps(kernel, route):
        ms = prof[route].get(kernel, 0.0)
        return must[kernel] / (ms * 1e-3) / 1e9 if ms else 0.0
    res["trim"] = {"segments": n_segs, "classes": {name: int((h_trims[:, 7] == c).sum()) for c, name in enumerate(("whole", "ends", "split", "none"))},
                   "kept_bases": int(h_trims[:, 3].sum()), "good_bases": int(h_trims[:, 1].sum()), "out_bytes": out_bytes,
                   "bytes_must_move": must,
                   "GBps_of_must_move": {"k_pile_call": gbps("k_pile_call", "pile_call"), "k_pile_reads": gbps("k_pile_reads", "pile_call"),
                                         "k_seg_count": gbps("k_seg_count", "segments"), "k_seg_write": gbps("k_seg_write", "segments"),
                                         "k_ext_copy": gbps("k_ext_copy", "pos_extract")}}

    # the host route: the copies, and the numpy reference on the first reads
    from test_trim_abi import reference_segments
    t_copy, (h_table, h_off) = timed(lambda: (table.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint64)))
    n_host = min(args.host_reads, args.reads)
    rows_host = int(h_off[n_host])
    t0 = time.perf_counter()
    want = reference_segments(h_table[:rows_host], h_off[:n_host + 1], min_depth, min_depth, args.min_len)
    t_ref = (time.perf_counter() - t0) * 1e3
    got = ctx.pile_segments(table[:rows_host].contiguous(), off[:n_host + 1].contiguous(), **seg_kw)
    same = all(g.cpu().numpy().tobytes() == w_.tobytes() for g, w_ in zip(got, want))
    res["host_route"] = {"copy_table_and_offsets_ms": t_copy, "table_bytes": int(h_table.nbytes), "reference_reads": n_host, "reference_rows": rows_host,
                         "reference_ms": t_ref, "reference_equals_device": bool(same)}
    res["segments_over_pile_call"] = res["ms"]["segments"]["median"] / res["ms"]["pile_call"]["median"]
    res["correct_trim_over_correct"] = res["ms"]["correct_trim"]["median"] / res["ms"]["correct"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
