#!/usr/bin/env python3
"""Model of k_pmh_points' a-priori q_max bound: keys that reach the expensive half of a first point, and the share
of reads that fail the bound and start over, per c.  No GPU: first points of weight-1 keys are drawn as uniform (h, slot) pairs
(Exp01 at lambda = ln(m / (m - 1)) is uniform to 0.5 %), the running bound is refreshed every 16 chunks of 64 keys as in the kernel.

    python scripts/sim_pmh_tau.py [--m 200] [--reads 2000] [--c 2.3 3.5 4.6 6.9]

Read lengths: log-normal around the headline's mean (4.38 Gbases / 746 333 reads), sigma 0.9 (an ONT-like shape; the bench's
generator is not imported here, so the eligible share is approximate)."""
import argparse
import math

import numpy as np


def one_read(rng, n, m, tau):
    """-> (keys that passed the cheap test, bound held)"""
    h = rng.random(n)
    slot = rng.integers(0, m, n)
    mins = np.full(m, np.inf)
    bound = tau
    survivors = 0
    for c0 in range(0, n, 64):
        if (c0 // 64) % 16 == 0:
            bound = min(mins.max(), tau)
        hh, ss = h[c0:c0 + 64], slot[c0:c0 + 64]
        keep = hh < bound
        survivors += int(keep.sum())
        np.minimum.at(mins, ss[keep], hh[keep])
    return survivors, tau == math.inf or mins.max() < tau


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--c", type=float, nargs="*", default=[2.3, 3.5, 4.6, 6.9])
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    mean, sigma = 4.38e9 / 746_333, 0.9
    lens = np.maximum(200, rng.lognormal(math.log(mean) - sigma * sigma / 2, sigma, a.reads)).astype(np.int64)
    total = int(lens.sum())
    base = sum(one_read(rng, int(n), a.m, math.inf)[0] for n in lens)
    print("m = %d, %d reads, %d keys; running bound alone: %.3f of the keys pass the cheap test" % (a.m, a.reads, total, base / total))
    print("%6s %10s %10s %10s %12s" % ("c", "eligible", "redone", "e^-c", "survivors"))
    for c in a.c:
        tau_num = a.m * (math.log(a.m) + c)
        surv = redone = elig = 0
        for n in lens:
            n = int(n)
            tau = tau_num / n if n >= int(tau_num) and tau_num / n < 1.0 else math.inf
            s, ok = one_read(rng, n, a.m, tau)
            if tau != math.inf:
                elig += 1
            if not ok:  # the read starts over with the running bound alone
                redone += 1
                s += one_read(rng, n, a.m, math.inf)[0]
            surv += s
        print("%6.1f %10.3f %10.4f %10.4f %12.3f" % (c, elig / a.reads, redone / max(1, elig), math.exp(-c), surv / total))


if __name__ == "__main__":
    main()
