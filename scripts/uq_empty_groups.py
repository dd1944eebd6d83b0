#!/usr/bin/env python3
"""How many of k_multiset_uq's register-slot groups a read leaves empty, on the read lengths of a bench.py workload (host only).

A thread of k_multiset_uq holds UQ_KREG = 20 key slots, worked in five groups of four; group g of a workgroup stands for places
[4 T g, 4 T (g + 1)) of the read (T = 512 threads in the first shape, 1024 in the second).  A read of nk k-mers whose first base
lies at place `lead` of its first staged word (offsets[r] mod 16, seq_lead) fills the first ceil((nk + lead) / (4 T)) groups.

    python scripts/uq_empty_groups.py [--workload ont_k31] [--reads N] > profiles/uq_empty_groups.txt

The lengths are the ones bench.py's _gen draws (synth.ont_reads_device takes them from a host generator seeded by the
workload's seed alone: the rank's read_seed, seed * 1000 + rank, moves the bases, not the lengths)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UQ_KREG = 20
SHAPES = (("first <512>", 512), ("second <1024>", 1024))


def lengths(cfg):
    from kmerutils_amd import synth
    rng = np.random.default_rng(cfg["seed"] ^ 0x5EED)  # as ont_reads_device
    if cfg["fixed_len"]:
        return np.full(cfg["n_reads"], int(cfg["fixed_len"]), dtype=np.int64)
    return synth.ont_lengths(cfg["n_reads"], rng, mean_target=cfg["total_bases"] / cfg["n_reads"])


def table(lens, k):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    lead = off[:-1] & 15
    nk = np.maximum(lens - k + 1, 0)
    span = nk + lead
    rows, taken = [], nk == 0  # a read without a k-mer is nobody's
    for name, threads in SHAPES:
        per_group = 4 * threads
        mine = ~taken & (span <= UQ_KREG * threads)
        taken |= mine
        touched = -(-span[mine] // per_group)
        groups = UQ_KREG // 4
        hist = np.bincount(touched, minlength=groups + 1)[1:]
        turns = groups * int(mine.sum())
        rows.append(dict(name=name, threads=threads, reads=int(mine.sum()), kmers=int(nk[mine].sum()), mean_nk=float(nk[mine].mean()) if mine.any() else 0.0,
                         hist=hist.tolist(), mean_touched=float(touched.mean()) if mine.any() else 0.0,
                         empty_share=float(1.0 - touched.sum() / turns) if turns else 0.0))
    rest = ~taken
    return rows, int(rest.sum()), int(nk[rest].sum()), int(nk.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ont_k31")
    ap.add_argument("--reads", type=int, default=0, help="a smaller sample with the same length law")
    args = ap.parse_args()
    import bench
    bargs = argparse.Namespace(workload=args.workload, genome=0, reads=args.reads, bases=0, sketch_size=0)
    cfg = bench.workload_cfg(bargs)
    lens = lengths(cfg)
    rows, n_rest, k_rest, k_all = table(lens, cfg["k"])
    print("# k_multiset_uq: register-slot groups a read fills (scripts/uq_empty_groups.py, host arithmetic on the workload's lengths)")
    print("# workload %s: %d reads, %d bases, k = %d, seed 0x%X; lead = offsets[r] mod 16" % (cfg["name"], len(lens), int(lens.sum()), cfg["k"], cfg["seed"]))
    print("# a group-turn = one of the five groups of one read's turn; empty = no thread of the workgroup has a k-mer in it")
    for r in rows:
        print("%-14s reads %7d (%5.1f %%)  k-mers %5.1f %%  mean nk %7.0f  reads filling 1..5 groups %s  mean filled %.2f  empty group-turns %.1f %%" % (
            r["name"], r["reads"], 100.0 * r["reads"] / len(lens), 100.0 * r["kmers"] / k_all, r["mean_nk"], r["hist"], r["mean_touched"], 100.0 * r["empty_share"]))
    print("%-14s reads %7d (%5.1f %%)  k-mers %5.1f %%  (beyond both shapes: the general list-emitting kernel)" % (
        "rest", n_rest, 100.0 * n_rest / len(lens), 100.0 * k_rest / k_all))


if __name__ == "__main__":
    main()
