#!/usr/bin/env python3
"""kmu_sig_knn (fused compare + selection) against what a user had before it: row slabs of kmu_sig_equal_matrix on device
tensors + torch.topk(k + 1) per slab + removal of the self entry.  Self-join of N rows (default 262 144), m = 200, u32,
k = 10, group = row, signatures resident in HBM (graded similarity: rows over an alphabet of 4 values, copies of earlier
rows with a random fraction of slots changed; fixed seed).  Device events around synchronised calls, three warm-up calls,
then the two alternate; one JSON line.  The eq multiset of every row is compared between the two once, untimed."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from kmerutils_amd import lib

N, M, K = int(os.environ.get("N", 262144)), int(os.environ.get("M", 200)), int(os.environ.get("K", 10))
SLAB, RUNS = int(os.environ.get("SLAB", 4096)), int(os.environ.get("RUNS", 5))
VALU_PER_COMPARE = 2.5   # issue slots: per two slots 2 v_cmp_ne + v_cndmask + a half-rate v_addc_co (disassembly, scripts/asm_mix.py)
VALU_ISSUE_PEAK = 1.03e9 * 4 * 256 * 64   # lane-operations per second: measured issue rate (profiles/r03_valu_issue.txt)
dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(0x4B4E4E)
sig = torch.randint(0, 4, (N, M), dtype=torch.int32, device=dev, generator=g)
half = N // 2                      # the second half: copies of rows of the first half, a random fraction of slots redrawn
src = torch.randint(0, half, (N - half,), device=dev, generator=g)
frac = torch.rand(N - half, 1, device=dev, generator=g)
redraw = torch.randint(0, 4, (N - half, M), dtype=torch.int32, device=dev, generator=g)
sig[half:] = torch.where(torch.rand(N - half, M, device=dev, generator=g) < frac, redraw, sig[src])
del redraw, frac
grp = torch.arange(N, dtype=torch.int32, device=dev)
ctx = lib.Context(0)


def fused():
    return ctx.sig_knn(sig, sig, K, grp, grp)


def baseline():
    out = torch.empty((N, K), dtype=torch.int16, device=dev)
    for r0 in range(0, N, SLAB):
        r1 = min(N, r0 + SLAB)
        eq = ctx.sig_equal_matrix(sig[r0:r1], sig)
        val, idx = torch.topk(eq, K + 1, dim=1)
        own = idx == torch.arange(r0, r1, device=dev)[:, None]
        # drop the self entry (or, if ties pushed it out, the last one): K values per row stay
        drop = torch.where(own.any(1), own.int().argmax(1), torch.full((r1 - r0,), K, device=dev))
        keep = torch.arange(K + 1, device=dev)[None, :] != drop[:, None]
        out[r0:r1] = val[keep].view(r1 - r0, K)
    return out


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = f()
    ctx.synchronize()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


for _ in range(3):
    timed(fused)
t_f, t_b = [], []
for _ in range(RUNS):
    dt, (idx, eq) = timed(fused)
    t_f.append(dt)
    dt, beq = timed(baseline)
    t_b.append(dt)
same = bool(torch.equal(torch.sort(eq.int(), 1).values, torch.sort(beq.int(), 1).values))
no_self = bool((idx != grp[:, None]).all())
ctx.profile_enable(True)
fused()
prof = ctx.profile_get()
med_f, med_b = statistics.median(t_f), statistics.median(t_b)
cps = N * N * M / (med_f / 1e3)
print(json.dumps({"workload": "knn_self_join", "n": N, "m": M, "k": K, "slab_rows": SLAB, "runs": RUNS,
                  "fused_ms": {"median": med_f, "min": min(t_f), "max": max(t_f)},
                  "baseline_ms": {"median": med_b, "min": min(t_b), "max": max(t_b)},
                  "fused_not_above_baseline": med_f <= med_b, "same_eq_multiset_per_row": same, "no_row_lists_itself": no_self,
                  "compares_per_s": cps, "valu_ops_per_compare": VALU_PER_COMPARE,
                  "share_of_integer_issue_peak": cps * VALU_PER_COMPARE / VALU_ISSUE_PEAK,
                  "kernels_ms": {k: v[1] for k, v in prof.items()}, "device": torch.cuda.get_device_name(0)}))
