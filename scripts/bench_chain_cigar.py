#!/usr/bin/env python3
"""kmu_chain_cigar timed: the alignment path of every chain of the workload of scripts/bench_chain_align.py.

Device-resident ONT-shaped reads (kmerutils_amd.synth: 8 % errors), k = 21, w = 10, KMU_FHASH_CANON_INVHASH; chains with max_gap
5000, band 500, min_seeds 3, each read pair once.  At band 64 and at band 256, on the resident reads and records:
  chain_align          Context.chain_align, the yardstick
  cigar_count          kmu_chain_cigar with ops_out == NULL: records, offsets and the number of runs
  cigar_count_write    Context.chain_cigar: the count call, then the call that writes
  cigar_one_call       Context.chain_cigar(aln=...): ops sized by 2 edit + 1 runs per chain from the records of chain_align, one call
Host clock around synchronised calls; a warm-up of each, then --repeats runs in alternation; median / min / max.  Then, per band,
one profiled one-call run: the device time of every kernel (kmu_profile_get), the batches (launches of k_cigar_sweep), the trace
bytes of all chains, the runs, the ratio of k_cigar_sweep to k_chain_align and of k_cigar_walk to k_cigar_sweep; and the chain with
the most anti-diagonals on its own.
  host      for context: the reference of tests/test_chain_cigar_abi.py (reference_cigar: the banded values of the whole matrix in
            numpy, then the walk in Python) at band 64 on the chains whose read_a is below --host-reads and whose segments are at most
            --host-max-len bases (the reference keeps the full matrix), run once, and compared with the device's records and runs.
One JSON line.

  scripts/bench_chain_cigar.py [--reads 20000] [--mean-len 5000] [--repeats 5] [--host-reads 200] [--host-max-len 4000] [--out FILE]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--host-max-len", type=int, default=4000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer, synth
    from test_chain_cigar_abi import reference_cigar
    dev = torch.device("cuda", 0)
    k, w, max_gap, band_chain, min_seeds = 21, 10, 5000, 500, 3
    bases, off, lens = synth.ont_reads_device(args.reads, args.reads * args.mean_len, 50_000_000, 0xA7, dev)
    ctx = lib.Context(0)
    res = {"reads": args.reads, "bases": int(off[-1].item()), "k": k, "w": w, "max_gap": max_gap, "band_chain": band_chain,
           "min_seeds": min_seeds, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "trace_default_bytes": A.CIGAR_TRACE_DEFAULT}

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
    n_chains, n_reads = int(chains.shape[0]), int(off.shape[0]) - 1
    d_aln = torch.zeros((max(n_chains, 1), 4), dtype=torch.int32, device=dev)
    d_opoff = torch.zeros(n_chains + 1, dtype=torch.int64, device=dev)

    def count_only(band):
        p, total = A.CigarParams(band, 0, 0), C.c_uint64(0)
        ctx._check(ctx.L.kmu_chain_cigar(ctx.h, chains.data_ptr(), n_chains, bases.data_ptr(), off.data_ptr(), n_reads, bases.data_ptr(),
                                         off.data_ptr(), n_reads, C.byref(p), A.MEM_DEVICE, d_aln.data_ptr(), d_opoff.data_ptr(), None, 0,
                                         C.byref(total)))
        return int(total.value)

    plain = {band: ctx.chain_align(chains, bases, off, band=band) for band in (64, 256)}
    routes = {}
    for band in (64, 256):
        routes["chain_align_band%d" % band] = lambda band=band: ctx.chain_align(chains, bases, off, band=band)
        routes["cigar_count_band%d" % band] = lambda band=band: count_only(band)
        routes["cigar_count_write_band%d" % band] = lambda band=band: ctx.chain_cigar(chains, bases, off, band=band)
        routes["cigar_one_call_band%d" % band] = lambda band=band: ctx.chain_cigar(chains, bases, off, band=band, aln=plain[band])
    for f in routes.values():  # warm-up
        timed(f)
    t = {n: [] for n in routes}
    for _ in range(args.repeats):
        for n, f in routes.items():
            t[n].append(timed(f)[0])

    rec = chains.cpu().numpy().view(np.uint32).reshape(-1, 10)
    m, n = (rec[:, 7] - rec[:, 6]).astype(np.int64), (rec[:, 9] - rec[:, 8]).astype(np.int64)
    res.update({"chains": n_chains, "segment_bases_max": int(np.maximum(m, n).max()) if n_chains else 0,
                "ms": {name: stat(v) for name, v in t.items()}})

    def profiled(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = fn()
        ctx.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        return out, {name: round(v[1], 4) for name, v in prof.items()}, {name: v[0] for name, v in prof.items()}

    results = {}
    for band in (64, 256):
        _, prof_align, _ = profiled(lambda: ctx.chain_align(chains, bases, off, band=band))
        (aln, ops, op_off), prof, launches = profiled(lambda: ctx.chain_cigar(chains, bases, off, band=band, aln=plain[band]))
        aln_h = aln.cpu().numpy().view(np.uint32).reshape(-1, 4)
        results[band] = (aln_h, ops.cpu().numpy().view(np.uint32), op_off.cpu().numpy().view(np.uint64))
        done = (aln_h[:, 3] & A.ALN_DONE) != 0
        lo = np.minimum(0, n - m) - band
        steps = (m + n + (lo & 1)) // 2 + 1
        cpl = np.where(aln_h[:, 2] <= 128, 1, np.where(aln_h[:, 2] <= 256, 2, np.where(aln_h[:, 2] <= 512, 4, 8)))
        trace = ((steps * cpl + 7) // 8 * 256)[done]
        res["band%d" % band] = {
            "kernels_ms": prof, "k_chain_align_ms": prof_align["k_chain_align"], "batches": launches.get("k_cigar_sweep", 0),
            "pair_steps": int(steps[done].sum()), "trace_bytes": int(trace.sum()), "trace_bytes_max_chain": int(trace.max()) if trace.size else 0,
            "runs": int(ops.shape[0]), "runs_bound_2_edit_plus_1": int((2 * aln_h[done, 0].astype(np.int64) + 1).sum()),
            "share_path": float(((aln_h[:, 3] & A.ALN_PATH) != 0).mean()) if n_chains else 0.0,
            "sweep_over_chain_align": prof["k_cigar_sweep"] / prof_align["k_chain_align"] if prof_align["k_chain_align"] else 0.0,
            "walk_over_sweep": prof["k_cigar_walk"] / prof["k_cigar_sweep"] if prof.get("k_cigar_sweep") else 0.0}
        if launches.get("k_cigar_sweep", 0) > 1:  # what the cut into batches costs: the same call with a budget that holds all chains
            _, prof_one, launches_one = profiled(lambda: ctx.chain_cigar(chains, bases, off, band=band, aln=plain[band],
                                                                         max_trace_bytes=int(trace.sum())))
            res["band%d" % band]["one_batch"] = {"kernels_ms": prof_one, "batches": launches_one.get("k_cigar_sweep", 0)}

    # the tail: the chain with the most anti-diagonals on its own
    if n_chains:
        longest = int(np.argmax(m + n))
        one = chains[longest:longest + 1].contiguous()
        timed(lambda: ctx.chain_cigar(one, bases, off, band=64))
        (_, one_ops, _), prof, _ = profiled(lambda: ctx.chain_cigar(one, bases, off, band=64, aln=plain[64][longest:longest + 1]))
        _, prof_align, _ = profiled(lambda: ctx.chain_align(one, bases, off, band=64))
        res["longest_chain_alone"] = {"m": int(m[longest]), "n": int(n[longest]), "runs": int(one_ops.shape[0]), "kernels_ms": prof,
                                      "k_chain_align_ms": prof_align["k_chain_align"]}

    # the host route on a sub-sample: numpy and a Python loop, run once
    h_bases, h_off = bases.cpu().numpy(), off.cpu().numpy().view(np.uint64)
    sub = np.nonzero((rec[:, 0] < args.host_reads) & (np.maximum(m, n) <= args.host_max_len))[0]
    h_chains = np.ascontiguousarray(rec[sub]).view(np.dtype(A.CHAIN_DTYPE)).reshape(-1)
    t0 = time.perf_counter()
    want = reference_cigar(h_chains, h_bases, h_off, band=64)
    host_ms = (time.perf_counter() - t0) * 1e3
    aln_h, ops_h, off_h = results[64]
    equal = bool(np.array_equal(aln_h[sub], want[0].view(np.uint32).reshape(-1, 4)))
    for at, c in enumerate(sub.tolist()):
        equal = equal and np.array_equal(ops_h[int(off_h[c]):int(off_h[c + 1])], want[1][int(want[2][at]):int(want[2][at + 1])])
    res["host"] = {"reads": args.host_reads, "max_len": args.host_max_len, "chains": int(sub.size), "ms_numpy_and_python": host_ms,
                   "pair_steps": int(((m + n) // 2 + 1)[sub].sum()), "records_and_runs_equal_on_the_sub_sample": equal}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
