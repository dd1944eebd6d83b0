#!/usr/bin/env python3
"""The sub-lists k_multiset_long cuts its reads into, on the read lengths of a bench.py workload (host only).

A read of more than 20 480 places (nk k-mers behind the lead of its first staged word) is cut into P = ceil(nk / T_P) sub-lists by key
hash (pmh_long_parts, pmh_long_part_of; T_P = PMH_LONG_TP = 16 384).  A sub-list of n keys is Binomial(nk, 1 / P): expected nk / P,
sigma sqrt(nk (1 / P) (1 - 1 / P)); it must stay within the 20 480 keys a workgroup's registers hold.  Of n unique keys in bitmaps of
2^18 bits, n^2 / 2^18 are expected to share a bit with another and be collected (of UQ2_COLL = 2 048 places).

    python scripts/long_read_parts.py [--workload ont_k31] [--reads N] [--tp 16384] > profiles/long_read_parts.txt

The lengths are taken as scripts/uq_empty_groups.py takes them."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

UQ_KEYS, UQ_COLL, BM_BITS, DEF_PARTS, LONG_SEQ_KMERS = 20480, 2048, 18, 32, 1 << 18


def parts(nk, tp):
    return -(-nk // tp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ont_k31")
    ap.add_argument("--reads", type=int, default=0, help="a smaller sample with the same length law")
    ap.add_argument("--tp", type=int, default=16384, help="PMH_LONG_TP")
    args = ap.parse_args()
    import bench
    import uq_empty_groups
    cfg = bench.workload_cfg(argparse.Namespace(workload=args.workload, genome=0, reads=args.reads, bases=0, sketch_size=0))
    lens = uq_empty_groups.lengths(cfg)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    nk = np.maximum(lens - cfg["k"] + 1, 0)
    long_ = nk + (off[:-1] & 15) > UQ_KEYS
    nk = nk[long_]
    P = parts(nk, args.tp)
    print("# k_multiset_long: sub-lists per read (scripts/long_read_parts.py, host arithmetic on the workload's lengths)")
    print("# workload %s: %d reads, k = %d, seed 0x%X; T_P = %d; reads of more than %d places: %d, %d k-mers, mean %.0f, longest %d" % (
        cfg["name"], len(lens), cfg["k"], cfg["seed"], args.tp, UQ_KEYS, len(nk), int(nk.sum()), nk.mean() if len(nk) else 0.0, int(nk.max()) if len(nk) else 0))
    print("# sub-list: expected nk / P keys, sigma sqrt(nk (1/P)(1 - 1/P)); collected: n^2 / 2^%d of n unique keys (places: %d)" % (BM_BITS, UQ_COLL))
    fall = 0
    for p in np.unique(P):
        sel = nk[P == p]
        worst = int(sel.max())
        n_exp = worst / p
        n_5s = n_exp + 5.0 * np.sqrt(worst / p * (1.0 - 1.0 / p))
        back = int(p) > DEF_PARTS or n_5s > UQ_KEYS or n_5s * n_5s / (1 << BM_BITS) > UQ_COLL
        fall += int(back) * len(sel)
        print("P %2d  reads %6d  k-mers %10d (%5.1f %%)  largest read: sub-list expected %6.0f, +5 sigma %6.0f of %d; collected expected %5.0f, at +5 sigma %5.0f of %d%s" % (
            p, len(sel), int(sel.sum()), 100.0 * sel.sum() / max(1, nk.sum()), n_exp, n_5s, UQ_KEYS, n_exp * n_exp / (1 << BM_BITS),
            n_5s * n_5s / (1 << BM_BITS), UQ_COLL, "  FALLS BACK" if back else ""))
    print("mean P %.2f; reads expected to fall back to the general kernel (unique keys; a repetitive read collects more): %d" % (P.mean() if len(P) else 0.0, fall))
    pm = parts(LONG_SEQ_KMERS, args.tp)
    print("longest read the per-sequence route keeps: %d k-mers, P = %d of at most %d, sub-list expected %.0f" % (LONG_SEQ_KMERS, pm, DEF_PARTS, LONG_SEQ_KMERS / pm))


if __name__ == "__main__":
    main()
