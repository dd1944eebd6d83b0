#!/usr/bin/env python3
"""kmu_sg_classify, kmu_sg_graph and minimizer.unitig_labels timed on two sets of resident chain records.

  sparse   the workload of DESIGN.md 3.16: device-resident ONT-shaped reads (kmerutils_amd.synth: 8 % errors) over a genome of 50
           Mbases, so that a read has about one partner
  dense    reads of --dense-len bases made here with synth.genome_reads (8 % errors) at --dense-cov fold over a genome of
           --dense-genome bases, so that a vertex has tens of arcs
Both: k = 21, w = 10, KMU_FHASH_CANON_INVHASH; chains with max_gap 5000, band 500, min_seeds 3, each read pair once; alignment
records at band 64.  The graph: min_overlap 500, max_hang 1000, int_permille 250, min_identity_permille 700, fuzz --fuzz.  On the
resident records:
  sg_classify     Context.sg_classify
  sg_graph        Context.sg_graph (its two library calls: the count, then the graph)
  unitig_labels   minimizer.unitig_labels on the arcs
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max.  Then one profiled
run of sg_graph: the device time of every kernel (kmu_profile_get).  The graph itself: arcs, reduced records, contained reads, the
classes and the histogram of the out-degrees before and after the reduction.  The host route beside it: the records copied to the
host (timed), and reference_graph of tests/test_string_graph_abi.py on the records among the first --host-reads reads (timed; it is
Python loops), which must equal the device on the same records.  One JSON line.

  scripts/bench_string_graph.py [--reads 20000] [--mean-len 5000] [--dense-genome 1000000] [--dense-cov 30] [--dense-len 5000]
                                [--fuzz 100] [--repeats 5] [--host-reads 300] [--out FILE]
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
    ap.add_argument("--dense-genome", type=int, default=1_000_000)
    ap.add_argument("--dense-cov", type=int, default=30)
    ap.add_argument("--dense-len", type=int, default=5000)
    ap.add_argument("--fuzz", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-reads", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer, synth
    from test_string_graph_abi import reference_graph
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds, band = 21, 10, 5000, 500, 3, 64
    graph = dict(min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=700, fuzz=args.fuzz)
    ctx = lib.Context(0)
    res = {"k": k, "w": w, "band": band, "graph": graph, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def workload(name, bases, off):
        n_reads = int(off.shape[0]) - 1
        chains, aln = minimizer.read_alignments(ctx, bases, off, k, w, max_gap=max_gap, band_chain=band_chain, min_seeds=min_seeds, band=band)
        print("%s: %d reads, %d chains" % (name, n_reads, int(chains.shape[0])), file=sys.stderr, flush=True)
        arcs, arc_off, classes, reads = ctx.sg_graph(chains, aln, off, **graph)
        routes = {"sg_classify": lambda: ctx.sg_classify(chains, aln, off, **graph),
                  "sg_graph": lambda: ctx.sg_graph(chains, aln, off, **graph),
                  "unitig_labels": lambda: minimizer.unitig_labels(ctx, arcs, n_reads)}
        for f in routes.values():  # warm-up
            timed(f)
        t = {n: [] for n in routes}
        for _ in range(args.repeats):
            for n, f in routes.items():
                t[n].append(timed(f)[0])
        out = {"reads": n_reads, "bases": int(off[-1].item()), "chains": int(chains.shape[0]), "ms": {n: stat(v) for n, v in t.items()}}
        ctx.profile_enable(True)
        ctx.profile_reset()
        routes["sg_graph"]()
        ctx.synchronize()
        out["kernels_ms"] = {n: round(v[1], 4) for n, v in ctx.profile_get().items()}
        ctx.profile_enable(False)
        # the graph
        h_arcs, h_off = arcs.cpu().numpy().reshape(-1).view(np.dtype(A.SG_ARC_DTYPE)), arc_off.cpu().numpy().view(np.uint64)
        h_cls, h_reads = classes.cpu().numpy(), reads.cpu().numpy().reshape(-1).view(np.dtype(A.SG_READ_DTYPE))
        deg = (h_off[1:] - h_off[:-1]).astype(np.int64)
        alive = np.stack([h_reads["out_fwd"], h_reads["out_rev"]], axis=1).reshape(-1).astype(np.int64)
        labels = routes["unitig_labels"]().cpu().numpy()
        bins = [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 1 << 30]
        out["graph"] = {"arcs": int(h_arcs.shape[0]), "reduced_records": int(len(set(h_arcs["rec"][h_arcs["flags"] != 0].tolist()))),
                        "surviving_arcs": int((h_arcs["flags"] == 0).sum()), "unique_arcs": int(h_arcs["unique"].sum()),
                        "contained_reads": int((h_reads["flags"] & 1).sum()),
                        "classes": {name: int((h_cls == c).sum()) for c, name in enumerate(A.SG_CLASS_NAMES)},
                        "degree_bins": bins[:-1], "out_degree_hist": np.histogram(deg, bins)[0].tolist(),
                        "surviving_degree_hist": np.histogram(alive, bins)[0].tolist(), "max_out_degree": int(deg.max()) if len(deg) else 0,
                        "unitigs_of_two_or_more_reads": int((np.bincount(labels.astype(np.int64)) > 1).sum())}
        print("%s: %d arcs; the host route" % (name, out["graph"]["arcs"]), file=sys.stderr, flush=True)
        # the host route: the copies, and the reference on the records among the first reads
        t_copy, (h_chains, h_aln, h_offsets) = timed(lambda: (chains.cpu().numpy().reshape(-1).view(np.dtype(A.CHAIN_DTYPE)),
                                                              aln.cpu().numpy().reshape(-1).view(np.dtype(A.CHAIN_ALN_DTYPE)),
                                                              off.cpu().numpy().view(np.uint64)))
        n_host = min(args.host_reads, n_reads)
        keep = (h_chains["read_a"] < n_host) & (h_chains["read_b"] < n_host)
        sub_chains, sub_aln, sub_off = np.ascontiguousarray(h_chains[keep]), np.ascontiguousarray(h_aln[keep]), h_offsets[:n_host + 1]
        t0 = time.perf_counter()
        want = reference_graph(sub_chains, sub_aln, sub_off, **graph)
        t_ref = (time.perf_counter() - t0) * 1e3
        t_dev, got = timed(lambda: ctx.sg_graph(sub_chains, sub_aln, sub_off, **graph))
        out["host_route"] = {"copy_records_ms": t_copy, "record_bytes": int(h_chains.nbytes + h_aln.nbytes), "reference_reads": n_host,
                             "reference_records": int(keep.sum()), "reference_arcs": int(want[0].shape[0]), "reference_ms": t_ref,
                             "device_on_the_same_records_ms": t_dev,
                             "reference_equals_device": bool(all(g.tobytes() == w_.tobytes() for g, w_ in zip(got, want)))}
        res[name] = out

    bases, off, _ = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    workload("sparse", bases, off)
    del bases, off
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
