#!/usr/bin/env python3
"""kmu_sg_clean timed on resident arcs and summaries.

  sparse, dense   the two workloads of scripts/bench_string_graph.py (same reads, same chains, same graph parameters): the arcs
                  and the summaries of sg_graph
  planted         --backbones copies of the mix of tests/test_clean_abi.py (65 backbone reads, ten dead ends, five alternative
                  paths: 107 reads and 222 arcs each) in one call, read numbers and strands shuffled over all of them
On the resident data: Context.sg_clean with --tips / --bubbles, host clock around synchronised calls; a warm-up, then --repeats runs;
median / min / max.  Then one profiled run: the launches and the device time of every kernel (kmu_profile_get).  The counts of the
call, and what it does to the layout: the vertices with more than one surviving arc and the unitigs of Context.sg_unitigs (how many,
how many of two or more reads, the longest in reads) before and after one round and after --rounds rounds.  The host route beside
it: the arcs and the summaries copied to the host (timed), and reference_clean of tests/test_clean_abi.py on the arcs among the first
--host-reads reads (planted: on a smaller batch of about as many reads) (timed; Python loops), which must equal the device on the same
arcs.  One JSON line.

  scripts/bench_clean.py [--reads 20000] [--mean-len 5000] [--dense-genome 1000000] [--dense-cov 30] [--dense-len 5000] [--fuzz 100]
                         [--backbones 100000] [--tips 4] [--bubbles 8] [--rounds 3] [--repeats 5] [--host-reads 2000] [--skip-reads]
                         [--out FILE]
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


def planted_batch(np, A, spec, copies, seed):
    """`copies` of one planted graph (the edges of tests/test_clean_abi.planted, laid out with numpy): (arcs, n_reads), sorted"""
    from test_clean_abi import planted
    one, n_one, _ = planted(seed=seed, **spec)  # one copy gives the edges: its forward arcs, as (from, to) between its reads
    rng = np.random.default_rng(seed)
    pairs = {}
    for x in one.tolist():
        pairs.setdefault(x[4], (x[0], x[1]))  # rec -> the first of its two arcs
    edges = np.array(sorted(pairs.values()), np.int64)
    n = n_one * copies
    ids, flip = rng.permutation(n).astype(np.int64), rng.integers(0, 2, n)
    base = (np.arange(copies, dtype=np.int64) * n_one)[:, None]
    node_a, node_b = (base + (edges[:, 0] >> 1)[None, :]).reshape(-1), (base + (edges[:, 1] >> 1)[None, :]).reshape(-1)
    a = 2 * ids[node_a] + (flip[node_a] ^ np.tile(edges[:, 0] & 1, copies))
    b = 2 * ids[node_b] + (flip[node_b] ^ np.tile(edges[:, 1] & 1, copies))
    arcs = np.zeros(2 * len(a), np.dtype(A.SG_ARC_DTYPE))
    arcs["from"], arcs["to"] = np.concatenate([a, b ^ 1]), np.concatenate([b, a ^ 1])
    arcs["len"], arcs["ovl"] = 100, 900
    arcs["rec"] = np.concatenate([np.arange(len(a)), np.arange(len(a))])
    return arcs[np.lexsort((arcs["rec"], arcs["to"], arcs["from"]))], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--mean-len", type=int, default=5000)
    ap.add_argument("--dense-genome", type=int, default=1_000_000)
    ap.add_argument("--dense-cov", type=int, default=30)
    ap.add_argument("--dense-len", type=int, default=5000)
    ap.add_argument("--fuzz", type=int, default=100)
    ap.add_argument("--backbones", type=int, default=100_000)
    ap.add_argument("--tips", type=int, default=4)
    ap.add_argument("--bubbles", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-reads", type=int, default=2000)
    ap.add_argument("--skip-reads", action="store_true", help="leave out sparse and dense (they need the whole long-read route first)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer, synth
    from test_clean_abi import MIX, reference_clean
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds, band = 21, 10, 5000, 500, 3, 64
    graph = dict(min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=700, fuzz=args.fuzz)
    ctx = lib.Context(0)
    res = {"k": k, "w": w, "band": band, "graph": graph, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "max_tip_reads": args.tips, "max_bubble_reads": args.bubbles, "rounds": args.rounds}
    ARC, READ, UNITIG = np.dtype(A.SG_ARC_DTYPE), np.dtype(A.SG_READ_DTYPE), np.dtype(A.SG_UNITIG_DTYPE)

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

    def layout(arcs, reads, off):
        """what the unitig layout makes of a graph: branching vertices, unitigs, the longest"""
        h_reads = reads.cpu().numpy().reshape(-1).view(READ)
        unitigs, path, _ = ctx.sg_unitigs(arcs, minimizer.layout_reads(reads), off)
        u = unitigs.cpu().numpy().reshape(-1).view(UNITIG)
        return {"branching_vertices": int((h_reads["out_fwd"] > 1).sum() + (h_reads["out_rev"] > 1).sum()), "unitigs": int(u.shape[0]),
                "reads_placed": int(path.shape[0]), "unitigs_of_two_or_more_reads": int((u["n_reads"] > 1).sum()),
                "longest_unitig_reads": int(u["n_reads"].max()) if len(u) else 0, "longest_unitig_bases": int(u["len"].max()) if len(u) else 0}

    def workload(name, arcs, reads, off, host_graph=None):
        n_reads = int(off.shape[0]) - 1
        call = lambda: ctx.sg_clean(arcs, reads, n_reads, args.tips, args.bubbles)  # noqa: E731
        timed(call)  # warm-up
        t = [timed(call)[0] for _ in range(args.repeats)]
        c_arcs, c_reads, stats = call()
        out = {"reads": n_reads, "arcs": int(arcs.shape[0]), "ms": {"sg_clean": stat(t)}, "stats": stats, "kernels": profiled(call)}
        # (arcs without summaries: a call with both phases off gives them, and `unique`)
        own_arcs, own = (arcs, reads) if reads is not None else ctx.sg_clean(arcs, None, n_reads, 0, 0)[:2]
        out["before"] = layout(own_arcs, own, off)
        out["after_one_round"] = layout(c_arcs, c_reads, off)
        t_rounds, (r_arcs, r_reads, r_stats) = timed(lambda: minimizer.clean_graph(ctx, arcs, reads, n_reads, args.tips, args.bubbles, args.rounds))
        out["after_rounds"] = dict(layout(r_arcs, r_reads, off), stats=r_stats, ms=t_rounds)
        print("%s: %s; the host route" % (name, stats), file=sys.stderr, flush=True)
        # the host route: the copies, and the reference on the arcs among the first reads
        t_copy, (h_arcs, h_reads) = timed(lambda: (arcs.cpu().numpy().reshape(-1).view(ARC),
                                                   None if reads is None else reads.cpu().numpy().reshape(-1).view(READ)))
        if host_graph is None:
            n_host = min(args.host_reads, n_reads)
            keep = ((h_arcs["from"] >> 1) < n_host) & ((h_arcs["to"] >> 1) < n_host)
            sub_arcs = np.ascontiguousarray(h_arcs[keep])  # (an arc and its mate join the same two reads)
            sub_reads = None if h_reads is None else np.ascontiguousarray(h_reads[:n_host])
        else:  # (shuffled read numbers: the first reads share no arc, so the subset is a smaller batch of the same kind)
            sub_arcs, n_host = host_graph
            sub_reads = None
        t0 = time.perf_counter()
        want = reference_clean(sub_arcs, n_host, args.tips, args.bubbles, sub_reads)
        t_ref = (time.perf_counter() - t0) * 1e3
        t_dev, got = timed(lambda: ctx.sg_clean(sub_arcs, sub_reads, n_host, args.tips, args.bubbles))
        out["host_route"] = {"copy_ms": t_copy, "copied_bytes": int(h_arcs.nbytes + (0 if h_reads is None else h_reads.nbytes)),
                             "reference_reads": n_host, "reference_arcs": int(sub_arcs.shape[0]), "reference_ms": t_ref, "reference_stats": want[2],
                             "device_on_the_same_arcs_ms": t_dev,
                             "reference_equals_device": bool(got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
                                                             and got[2] == want[2])}
        res[name] = out

    def from_reads(name, bases, off):
        chains, aln = minimizer.read_alignments(ctx, bases, off, k, w, max_gap=max_gap, band_chain=band_chain, min_seeds=min_seeds, band=band)
        arcs, _, _, reads = ctx.sg_graph(chains, aln, off, **graph)
        print("%s: %d reads, %d chains, %d arcs" % (name, int(off.shape[0]) - 1, int(chains.shape[0]), int(arcs.shape[0])), file=sys.stderr, flush=True)
        workload(name, arcs, reads, off)

    if not args.skip_reads:
        bases, off, _ = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
        from_reads("sparse", bases, off)
        del bases, off
        n_dense = args.dense_genome * args.dense_cov // args.dense_len
        h_bases, h_off = synth.genome_reads(n_dense, np.full(n_dense, args.dense_len), args.dense_genome, 0xD5, sub=0.04, ins=0.02, dele=0.02)
        from_reads("dense", torch.from_numpy(h_bases).to(dev), torch.from_numpy(h_off.astype(np.int64)).to(dev))
    t0 = time.perf_counter()
    arcs, n_reads = planted_batch(np, A, MIX, args.backbones, 3)
    print("planted: %d reads, %d arcs, built in %.1f s" % (n_reads, len(arcs), time.perf_counter() - t0), file=sys.stderr, flush=True)
    workload("planted", torch.from_numpy(arcs.view(np.int32).reshape(-1, 8)).to(dev), None,
             torch.from_numpy((np.arange(n_reads + 1, dtype=np.int64) * 1000)).to(dev),
             host_graph=planted_batch(np, A, MIX, max(1, args.host_reads // 107), 4))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
