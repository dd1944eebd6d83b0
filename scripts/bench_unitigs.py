#!/usr/bin/env python3
"""kmu_sg_unitigs and kmu_sg_unitig_seqs timed on resident arcs and reads.

  sparse, dense   the two workloads of scripts/bench_string_graph.py (same reads, same chains, same graph parameters): the arcs
                  and the summaries of sg_graph, the batch itself
  line            one synthetic line of --line-reads reads of 1 000 bases, each 100 to the right of the one before, with shuffled
                  read numbers and strands, given as arcs; random bases (the layout, not the letters, is timed)
  many            --many-unitigs lines of 5 .. 15 reads of the same kind in one call
On the resident data:
  sg_unitigs       Context.sg_unitigs
  sg_unitig_seqs   Context.sg_unitig_seqs (its two library calls: the count, then the bytes)
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max.  Then one profiled
run of each: the launches and the device time of every kernel (kmu_profile_get).  The host route beside it: the arcs, the summaries
and the bases copied to the host (timed), and reference_unitigs / reference_sequences of tests/test_unitigs_abi.py on the arcs among
the first --host-reads reads (timed; Python loops), which must equal the device on the same arcs.  One JSON line.

  scripts/bench_unitigs.py [--reads 20000] [--mean-len 5000] [--dense-genome 1000000] [--dense-cov 30] [--dense-len 5000] [--fuzz 100]
                           [--line-reads 1000000] [--many-unitigs 100000] [--repeats 5] [--host-reads 2000] [--skip-reads] [--out FILE]
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


def line_arcs(np, A, sizes, seed):
    """lines of the given numbers of reads (1 000 bases, step 100) with shuffled read numbers and strands: (arcs, offsets), numpy"""
    rng = np.random.default_rng(seed)
    n = int(sizes.sum())
    ids, flip = rng.permutation(n).astype(np.int64), rng.integers(0, 2, n)
    v = 2 * ids + flip
    last = np.zeros(n, bool)
    last[np.cumsum(sizes) - 1] = True
    a, b = v[:-1][~last[:-1]], v[1:][~last[:-1]]
    arcs = np.zeros(2 * len(a), np.dtype(A.SG_ARC_DTYPE))
    arcs["from"], arcs["to"] = np.concatenate([a, b ^ 1]), np.concatenate([b, a ^ 1])
    arcs["len"], arcs["ovl"], arcs["unique"] = 100, 900, 1
    arcs["rec"] = np.concatenate([np.arange(len(a)), np.arange(len(a))])
    return arcs[rng.permutation(len(arcs))], np.arange(n + 1, dtype=np.uint64) * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--mean-len", type=int, default=5000)
    ap.add_argument("--dense-genome", type=int, default=1_000_000)
    ap.add_argument("--dense-cov", type=int, default=30)
    ap.add_argument("--dense-len", type=int, default=5000)
    ap.add_argument("--fuzz", type=int, default=100)
    ap.add_argument("--line-reads", type=int, default=1_000_000)
    ap.add_argument("--many-unitigs", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-reads", type=int, default=2000)
    ap.add_argument("--skip-reads", action="store_true", help="leave out sparse and dense (they need the whole long-read route first)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer, synth
    from test_unitigs_abi import reference_sequences, reference_unitigs
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds, band = 21, 10, 5000, 500, 3, 64
    graph = dict(min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=700, fuzz=args.fuzz)
    ctx = lib.Context(0)
    res = {"k": k, "w": w, "band": band, "graph": graph, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    ARC, READ = np.dtype(A.SG_ARC_DTYPE), np.dtype(A.SG_READ_DTYPE)
    UNITIG, STEP, PLACE = np.dtype(A.SG_UNITIG_DTYPE), np.dtype(A.SG_STEP_DTYPE), np.dtype(A.SG_PLACE_DTYPE)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def profiled(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        ctx.synchronize()
        got = {n: {"launches": v[0], "ms": round(v[1], 4)} for n, v in ctx.profile_get().items()}
        ctx.profile_enable(False)
        return got

    def workload(name, arcs, reads, bases, off):
        n_reads = int(off.shape[0]) - 1
        unitigs, path, place = ctx.sg_unitigs(arcs, reads, off)
        routes = {"sg_unitigs": lambda: ctx.sg_unitigs(arcs, reads, off), "sg_unitig_seqs": lambda: ctx.sg_unitig_seqs(unitigs, path, bases, off)}
        for f in routes.values():  # warm-up
            timed(f)
        t = {n: [] for n in routes}
        for _ in range(args.repeats):
            for n, f in routes.items():
                t[n].append(timed(f)[0])
        h_unitigs = unitigs.cpu().numpy().reshape(-1).view(UNITIG)
        seq, _ = routes["sg_unitig_seqs"]()
        out = {"reads": n_reads, "bases": int(off[-1].item()), "arcs": int(arcs.shape[0]), "unitigs": int(h_unitigs.shape[0]),
               "reads_placed": int(path.shape[0]), "unitigs_of_two_or_more_reads": int((h_unitigs["n_reads"] > 1).sum()),
               "circular": int((h_unitigs["flags"] & 1).sum()), "longest_unitig_reads": int(h_unitigs["n_reads"].max()) if len(h_unitigs) else 0,
               "longest_unitig_bases": int(h_unitigs["len"].max()) if len(h_unitigs) else 0, "sequence_bytes": int(seq.shape[0]),
               "ms": {n: stat(v) for n, v in t.items()}}
        out["kernels"] = {n: profiled(f) for n, f in routes.items()}
        print("%s: %d unitigs; the host route" % (name, out["unitigs"]), file=sys.stderr, flush=True)
        # the host route: the copies, and the reference walk on the arcs among the first reads
        t_copy, (h_arcs, h_reads, h_bases, h_off) = timed(lambda: (arcs.cpu().numpy().reshape(-1).view(ARC),
                                                                   None if reads is None else reads.cpu().numpy().reshape(-1).view(READ),
                                                                   bases.cpu().numpy(), off.cpu().numpy().view(np.uint64)))
        n_host = min(args.host_reads, n_reads)
        keep = ((h_arcs["from"] >> 1) < n_host) & ((h_arcs["to"] >> 1) < n_host)
        sub_arcs, sub_off = np.ascontiguousarray(h_arcs[keep]), h_off[:n_host + 1]  # (an arc and its mate join the same two reads)
        sub_reads = None if h_reads is None else np.ascontiguousarray(h_reads[:n_host])
        sub_bases = h_bases[:int(sub_off[-1])]
        t0 = time.perf_counter()
        want = reference_unitigs(sub_arcs, sub_reads, sub_off)
        t_walk = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        want_seq = reference_sequences(want[0], want[1], sub_bases, sub_off)
        t_seq = (time.perf_counter() - t0) * 1e3
        t_dev, got = timed(lambda: ctx.sg_unitigs(sub_arcs, sub_reads, sub_off))
        t_dev_seq, got_seq = timed(lambda: ctx.sg_unitig_seqs(got[0], got[1], sub_bases, sub_off))
        out["host_route"] = {"copy_ms": t_copy, "copied_bytes": int(h_arcs.nbytes + h_bases.nbytes + (0 if h_reads is None else h_reads.nbytes)),
                             "reference_reads": n_host, "reference_arcs": int(keep.sum()), "reference_unitigs": int(want[0].shape[0]),
                             "reference_walk_ms": t_walk, "reference_sequences_ms": t_seq, "device_on_the_same_arcs_ms": t_dev,
                             "device_sequences_on_the_same_ms": t_dev_seq,
                             "reference_equals_device": bool(all(g.tobytes() == w_.tobytes() for g, w_ in zip(got + got_seq, want + want_seq)))}
        res[name] = out

    def from_reads(name, bases, off):
        chains, aln = minimizer.read_alignments(ctx, bases, off, k, w, max_gap=max_gap, band_chain=band_chain, min_seeds=min_seeds, band=band)
        arcs, _, _, reads = ctx.sg_graph(chains, aln, off, **graph)
        print("%s: %d reads, %d chains, %d arcs" % (name, int(off.shape[0]) - 1, int(chains.shape[0]), int(arcs.shape[0])), file=sys.stderr, flush=True)
        workload(name, arcs, reads, bases, off)

    def from_lines(name, sizes, seed):
        arcs, off = line_arcs(np, A, sizes, seed)
        block = torch.from_numpy(np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), 1 << 20)).to(dev)
        bases = block.repeat((int(off[-1]) >> 20) + 1)[:int(off[-1])].contiguous()
        workload(name, torch.from_numpy(arcs.view(np.int32).reshape(-1, 8)).to(dev), None, bases, torch.from_numpy(off.astype(np.int64)).to(dev))

    if not args.skip_reads:
        bases, off, _ = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
        from_reads("sparse", bases, off)
        del bases, off
        n_dense = args.dense_genome * args.dense_cov // args.dense_len
        h_bases, h_off = synth.genome_reads(n_dense, np.full(n_dense, args.dense_len), args.dense_genome, 0xD5, sub=0.04, ins=0.02, dele=0.02)
        from_reads("dense", torch.from_numpy(h_bases).to(dev), torch.from_numpy(h_off.astype(np.int64)).to(dev))
    from_lines("line", np.array([args.line_reads]), 1)
    from_lines("many", np.random.default_rng(2).integers(5, 16, args.many_unitigs), 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
