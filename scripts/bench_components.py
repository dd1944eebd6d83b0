#!/usr/bin/env python3
"""kmu_components timed against what a caller had without it.

Two shapes:
  overlaps   the batch of scripts/bench_anchor_overlaps.py (device-resident anchors of ONT-shaped reads, k = 21, nbkmer 16, window
             500 / overlap 250, n_keys 4, both strands, band 1): its overlap records, on the device, clustered at min_score 2
  giant      a random graph of average degree 8 over --nodes nodes (one giant component), edges as pairs on the device
and two routes from the edges to (label, cluster, size, members):
  device     ctx.components on the resident edges; only the count crosses to the host
  host       today's route: the edges copied to the host, a union-find over them in Python (numpy arrays turned into lists, one loop
             over the edges), then numpy for the numbers, sizes and member lists; scipy.sparse.csgraph.connected_components beside it
             when scipy imports (labels only)
The device call is timed with events on the context's stream after a warm-up (--repeats runs: median / min / max) and the kernels of
one call with kmu_profile_get; the host route is timed once with the host clock (it takes seconds).  The labels of the routes are
compared.  One JSON line.

  scripts/bench_components.py [--reads 20000] [--mean-len 5000] [--nodes 1000000] [--repeats 5] [--out FILE]
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


def host_union_find(np, n_nodes, u, v):
    """(label, cluster, size, members) by the rules of include/kmu.h: the smaller root stays"""
    parent = list(range(n_nodes))
    for a, b in zip(u.tolist(), v.tolist()):
        if a == b or a >= n_nodes or b >= n_nodes:
            continue
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            if a < b:
                parent[b] = a
            else:
                parent[a] = b
    label = np.array(parent, np.int64)
    while True:  # flatten
        up = label[label]
        if np.array_equal(up, label):
            break
        label = up
    roots = np.flatnonzero(label == np.arange(n_nodes))
    rank = np.zeros(n_nodes, np.int64)
    rank[roots] = np.arange(roots.size)
    cluster = rank[label]
    return label, cluster, np.bincount(cluster, minlength=roots.size), np.argsort(cluster, kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--mean-len", type=int, default=5000)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import anchor, lib, synth
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        connected_components = None
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.current_stream(0)
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "scipy": connected_components is not None, "cases": []}

    def device_ms(fn):
        with torch.cuda.stream(stream):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
        return a.elapsed_time(b), out

    def case(name, n_nodes, d_edges, weight_at, min_weight, extra):
        def device():
            return ctx.components(d_edges, n_nodes, weight_at=weight_at, min_weight=min_weight)
        torch.cuda.synchronize()  # the edges are there before the context's stream reads them
        device_ms(device)
        t_dev = [device_ms(device)[0] for _ in range(args.repeats)]
        got = device()
        ctx.profile_enable(True)
        ctx.profile_reset()
        device()
        ctx.synchronize()
        prof = {k: round(v[1], 4) for k, v in ctx.profile_get().items() if v[0]}
        ctx.profile_enable(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        words = d_edges.cpu().numpy().view(np.uint32)
        keep = np.ones(words.shape[0], bool) if weight_at == 0 else words[:, weight_at] >= min_weight
        u, v = words[keep, 0].astype(np.int64), words[keep, 1].astype(np.int64)
        t_copy = (time.perf_counter() - t0) * 1e3
        label, cluster, size, members = host_union_find(np, n_nodes, u, v)
        t_host = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(got.label.cpu().numpy().view(np.uint32), label) and got.n_components == size.size and
                    np.array_equal(got.cluster.cpu().numpy().view(np.uint32), cluster) and
                    np.array_equal(got.size.cpu().numpy().view(np.uint32), size) and
                    np.array_equal(got.members.cpu().numpy().view(np.uint32), members))
        c = {"shape": name, "nodes": n_nodes, "edges": int(d_edges.shape[0]), "edges_that_count": int(u.size),
             "components": int(size.size), "largest": int(size.max()), "device_ms": stat(t_dev), "host_ms": t_host, "host_copy_ms": t_copy,
             "results_equal": same, "device_over_host": stat(t_dev)["median"] / t_host, "kernels_ms": prof,
             "hook_ms": prof.get("k_cc_hook", 0.0), "rest_ms": round(sum(x for k, x in prof.items() if k != "k_cc_hook"), 4)}
        if connected_components is not None:
            t0 = time.perf_counter()
            g = coo_matrix((np.ones(u.size, np.int8), (u, v)), shape=(n_nodes, n_nodes))
            n_sp, _ = connected_components(g, directed=False)
            c["scipy_ms"] = (time.perf_counter() - t0) * 1e3
            c["scipy_components_equal"] = bool(n_sp == size.size)
        c.update(extra)
        res["cases"].append(c)

    # the overlap records of bench_anchor_overlaps
    k, nbkmer, window, overlap = 21, 16, 500, 250
    bases, off, _ = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    params = anchor.AnchorsGeneratorParameters("bench", window, nbkmer, k, overlap)
    p = params.sketch_params()
    p.mem = A.MEM_DEVICE
    hashes, _, _, row_off = ctx.read_anchors(bases, off, p, window, overlap, want_counts=False)
    hashes = hashes.contiguous()
    h_group = np.repeat(np.arange(args.reads, dtype=np.uint32), np.diff(row_off.astype(np.int64)))
    group = torch.from_numpy(h_group.view(np.int32)).to(dev)
    pairs, dist = ctx.anchor_match(hashes, hashes, n_keys=4, min_common=1, group_q=group, group_db=group)
    rec = ctx.anchor_overlaps(pairs, dist, row_off.astype(np.uint64), strands=2, band=1, min_score=1, upper=True).contiguous()
    case("overlaps", args.reads, rec, 4, 2, {"reads": args.reads, "window_pairs": int(pairs.shape[0]), "min_score": 2})
    del bases, hashes, pairs, dist, rec

    # one giant component
    g = torch.Generator(device=dev)
    g.manual_seed(0xCC)
    edges = torch.randint(0, args.nodes, (4 * args.nodes, 2), dtype=torch.int32, device=dev, generator=g)
    case("giant", args.nodes, edges, 0, 0, {"average_degree": 8})

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    if not all(c["results_equal"] for c in res["cases"]):
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
