#!/usr/bin/env python3
"""How many wave-turns of the multiset kernels' slot groups have no k-mer at all, on the read lengths of a bench.py workload (host only).

A wave-turn = one wave working one group of four register slots of one read.  In k_multiset_uq, group g of a thread stands for places
4 (tid + T g) .. + 3, so wave w of the workgroup owns the 256 consecutive places from 4 (T g + 64 w) on.  A read of `span` places
(its k-mers behind the lead of its first staged word) ends inside one wave; the group skip issues the whole groups [0, ceil(span / 4 T)),
and of those wave-turns ceil(span / 256) hold a k-mer.  The others are wholly idle.

In phase B of k_multiset_long slot q of thread t is entry 1024 q + t of a sub-list of n_p keys: in the group the sub-list ends in,
wave w holds an entry when 1024 q0 + 64 w < n_p.  The sub-lists are taken at their expected length nk / P (lengths only: the hash
decides the real ones).

    python scripts/uq_idle_waves.py [--workload ont_k31] [--reads N] > profiles/uq_idle_waves.txt

The lengths are taken as scripts/uq_empty_groups.py takes them."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

UQ_KREG = 20
SHAPES = (("first shape <512>", 512), ("second shape <1024>", 1024))
LONG_THREADS, PMH_LONG_TP = 1024, 16384


def uq_wave_turns(span, threads):
    """(issued, needed) wave-turns of reads of `span` places (array, every span in 1 .. UQ_KREG * threads) in a shape of `threads` threads"""
    span = np.asarray(span, dtype=np.int64)
    issued = -(-span // (4 * threads)) * (threads // 64)  # whole groups, every wave of them
    needed = -(-span // 256)                              # waves whose first place lies in front of the read's end
    return issued, needed


def long_wave_turns(n_p):
    """(issued, needed) wave-turns of phase B for sub-lists of n_p keys (array, 1 .. UQ_KREG * 1024)"""
    n_p = np.asarray(n_p, dtype=np.int64)
    waves = LONG_THREADS // 64
    groups = -(-n_p // (4 * LONG_THREADS))
    rem = n_p - (groups - 1) * 4 * LONG_THREADS  # entries of the last group: its first slot holds min(rem, 1024) of them
    last = -(-np.minimum(rem, LONG_THREADS) // 64)
    return groups * waves, (groups - 1) * waves + last


def spans(lens, k):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    nk = np.maximum(np.asarray(lens, dtype=np.int64) - k + 1, 0)
    return nk, nk + (off[:-1] & 15)


def table(lens, k):
    nk, span = spans(lens, k)
    rows, taken = [], nk == 0  # a read without a k-mer is nobody's
    for name, threads in SHAPES:
        mine = ~taken & (span <= UQ_KREG * threads)
        taken |= mine
        issued, needed = uq_wave_turns(span[mine], threads)
        rows.append((name, int(mine.sum()), int(issued.sum()), int(needed.sum())))
    rest = nk[~taken]
    P = -(-rest // PMH_LONG_TP)
    issued, needed = long_wave_turns(np.repeat(-(-rest // np.maximum(P, 1)), P)) if len(rest) else (np.zeros(0, np.int64),) * 2
    rows.append(("k_multiset_long, phase B", len(rest), int(issued.sum()), int(needed.sum())))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ont_k31")
    ap.add_argument("--reads", type=int, default=0, help="a smaller sample with the same length law")
    args = ap.parse_args()
    import bench
    import uq_empty_groups
    cfg = bench.workload_cfg(argparse.Namespace(workload=args.workload, genome=0, reads=args.reads, bases=0, sketch_size=0))
    lens = uq_empty_groups.lengths(cfg)
    print("# multiset kernels: wave-turns of the issued slot groups without a k-mer (scripts/uq_idle_waves.py, host arithmetic on the workload's lengths)")
    print("# workload %s: %d reads, %d bases, k = %d, seed 0x%X; lead = offsets[r] mod 16" % (cfg["name"], len(lens), int(lens.sum()), cfg["k"], cfg["seed"]))
    print("# a wave-turn = one wave on one group of four register slots of a read; issued = the groups the group skip leaves; needed = a k-mer in it")
    print("# k_multiset_long: sub-lists at their expected length nk / P")
    for name, reads, issued, needed in table(lens, cfg["k"]):
        print("%-26s reads %7d  wave-turns per read: issued %6.2f  needed %6.2f  wholly idle %4.1f %%" % (
            name, reads, issued / max(1, reads), needed / max(1, reads), 100.0 * (1.0 - needed / max(1, issued))))


if __name__ == "__main__":
    main()
