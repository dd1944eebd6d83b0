#!/usr/bin/env python3
"""kmu_sketch_groups against the loop it replaces: one kmu_sketch(..., ALL_SEQS) call per group over the same device-resident
data (existing code, the yardstick).  Seeded synthetic workloads:
  genomes          512 groups x 50 contigs x 40 kbases (1.0 Gbases), Kmer64bit k = 21, ProbMinHash3a m = 1000, u64
  proteomes        2000 groups x 3000 proteins x ~330 residues, KmerAA64bit k = 7, SuperMinHash2 m = 1000
  genomes_optdens  the genomes layout, OptDens f64 m = 1000
  genomes_hll      the genomes layout, HLL (SetSketch registers) u16 m = 4096
  chromosomes_hll  64 groups x 8 sequences x 2 Mbases (1.0 Gbases; every sequence above 2^20 k-mers), HLL u16 m = 4096
(KMU_LIB=<another build of the library> times that build on the same workloads: the second yardstick of a change to the route.)
Per workload: row equality of the two ways first, then warm-up, then timed runs of the two ways in alternation (host clock
around a call that ends in a device synchronise), median / min / max of each, and the per-kernel profile of one grouped call
(in a run of its own, after the timing).  Every workload runs in a child process under its own time limit; a failed step
stops the script.  One JSON line per workload, a text report in --out.

  scripts/bench_groups.py [--out profiles/groups_batch.txt] [--repeats 5] [--scale 1.0] [--step-timeout 900] [--only NAME]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("genomes", "proteomes", "genomes_optdens", "genomes_hll", "chromosomes_hll")


def make_workload(name, scale, dev):
    """-> bases (u8), offsets (i64), group_offsets (i64) on the device, SketchParams"""
    import torch
    from kmerutils_amd import _abi as A
    g = torch.Generator(device=dev)
    if name != "proteomes":
        g.manual_seed(0x6E0)
        n_groups, per, length = (max(2, int(64 * scale)), 8, 2_000_000) if name == "chromosomes_hll" else (max(2, int(512 * scale)), 50, 40_000)
        n_seq = n_groups * per
        lens = torch.full((n_seq,), length, dtype=torch.int64, device=dev)
        alpha = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
        algo, sig, m = {"genomes": (A.ALGO_PROB3A, A.SIG_U64, 1000), "genomes_optdens": (A.ALGO_OPTDENS, A.SIG_F64, 1000)}.get(
            name, (A.ALGO_HLL, A.SIG_U16, 4096))
        p = A.SketchParams(algo, A.KMER64BIT, 21, m, sig, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0,
                           A.MODE_ALL_SEQS, A.INPUT_ASCII, A.MEM_DEVICE, 0)
    else:
        g.manual_seed(0x9207)
        n_groups, per = max(2, int(2000 * scale)), 3000
        n_seq = n_groups * per
        z = torch.randn(n_seq, generator=g, device=dev, dtype=torch.float32)
        lens = torch.clamp(torch.exp(5.7 + 0.5 * z), 20, 5000).to(torch.int64)  # median 300, mean ~ 335 residues
        alpha = torch.tensor(list(b"ACDEFGHIKLMNPQRSTVWY"), dtype=torch.uint8, device=dev)
        p = A.SketchParams(A.ALGO_SUPER2, A.KMERAA64BIT, 7, 1000, A.SIG_U64, A.HASHER_NOHASH, A.FHASH_IDENTITY_RAW, 0,
                           A.MODE_ALL_SEQS, A.INPUT_ASCII, A.MEM_DEVICE, 0)
    offsets = torch.zeros(n_seq + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    total = int(offsets[-1].item())
    bases = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    step = 1 << 28
    for s in range(0, total, step):
        e = min(total, s + step)
        bases[s:e] = alpha[torch.randint(0, alpha.numel(), (e - s,), generator=g, device=dev)]
    bases[total:] = 0
    go = torch.arange(0, n_seq + 1, per, dtype=torch.int64, device=dev)
    return bases, offsets, go, p, total


def run_step(name, repeats, scale):
    import torch
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0)
    bases, offsets, go, p, total = make_workload(name, scale, dev)
    n_groups = go.numel() - 1
    h_go = go.cpu().tolist()
    m = p.sketch_size
    tdt = torch.int16 if p.sig_type == A.SIG_U16 else torch.int64  # (f64 rows compared as their bits)
    out_g = torch.zeros((n_groups, m), dtype=tdt, device=dev)
    out_l = torch.zeros((n_groups, m), dtype=tdt, device=dev)
    slices = [offsets[h_go[i]:h_go[i + 1] + 1] for i in range(n_groups)]
    rows = [out_l[i:i + 1] for i in range(n_groups)]

    def grouped():
        ctx.sketch_groups(bases, offsets, go, p, out=out_g)
        ctx.synchronize()

    def loop():
        for i in range(n_groups):
            ctx.sketch(bases, slices[i], p, out=rows[i])
        ctx.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0
    # the same rows, both ways (this is also the warm-up of every shape the timed runs use)
    t_first = {"grouped": timed(grouped), "loop": timed(loop)}
    sys.stderr.write("%s: %d symbols in %d groups; first calls: grouped %.1f ms, loop %.1f ms\n" %
                     (name, total, n_groups, t_first["grouped"] * 1e3, t_first["loop"] * 1e3))
    sys.stderr.flush()
    if not torch.equal(out_g, out_l):
        bad = (out_g != out_l).any(dim=1).nonzero().flatten().tolist()
        raise SystemExit("%s: rows differ between kmu_sketch_groups and the ALL_SEQS loop: groups %s" % (name, bad[:10]))
    timed(grouped)
    times = {"grouped": [], "loop": []}
    for it in range(repeats):  # alternating: drift of the box hits both alike
        times["grouped"].append(timed(grouped))
        times["loop"].append(timed(loop))
        sys.stderr.write("%s: run %d: grouped %.1f ms, loop %.1f ms\n" % (name, it, times["grouped"][-1] * 1e3, times["loop"][-1] * 1e3))
        sys.stderr.flush()
    ctx.profile_enable(True)
    ctx.profile_reset()
    grouped()
    prof = ctx.profile_get()
    ctx.profile_enable(False)

    def stat(v):
        v = sorted(v)
        return {"median_s": v[len(v) // 2], "min_s": v[0], "max_s": v[-1], "n": len(v)}
    res = {"workload": name, "groups": n_groups, "sequences": offsets.numel() - 1, "symbols": total, "repeats": repeats,
           "rows_equal": True, "first_call_s": t_first, "grouped": stat(times["grouped"]), "loop": stat(times["loop"]),
           "grouped_profile_ms": {k: {"launches": n, "ms": round(ms, 3)} for k, (n, ms) in sorted(prof.items())}}
    res["speedup_median"] = res["loop"]["median_s"] / res["grouped"]["median_s"]
    res["library"] = os.path.basename(lib.SO_PATH)
    print(json.dumps(res))


def box_state():
    """clocks and load of the box, as the tools report them (read-only queries)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showuse"], capture_output=True, text=True, timeout=60)
        keep = [ln for ln in r.stdout.splitlines() if "GPU[0]" in ln]
        return keep or [ln for ln in r.stdout.splitlines() if ln.strip()][:20]
    except Exception as e:  # noqa: BLE001 -- a report line, not a result
        return ["rocm-smi not available: %r" % (e,)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--step", choices=WORKLOADS, default=None, help="(internal) run one workload in this process")
    a = ap.parse_args()
    if a.step:
        run_step(a.step, a.repeats, a.scale)
        return 0
    lines = ["kmu_sketch_groups against a loop of kmu_sketch(ALL_SEQS) calls, device-resident data (scripts/bench_groups.py, scale %g)" % a.scale,
             "box before:"] + ["  " + ln for ln in box_state()]
    rc = 0
    for name in WORKLOADS:
        if a.only and name not in a.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--repeats", str(a.repeats), "--scale", str(a.scale)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # (the child's progress lines go straight to stderr)
        if r.returncode != 0:
            lines += ["%s: FAILED (exit %d)" % (name, r.returncode)] + r.stdout.splitlines()[-5:]
            rc = r.returncode
            break  # nothing more is started on the GPU after a failed step
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(res))
        lines.append("")
        lines.append("%s (%s): %d groups, %d sequences, %d symbols; rows equal: %s" %
                     (name, res["library"], res["groups"], res["sequences"], res["symbols"], res["rows_equal"]))
        for way in ("grouped", "loop"):
            s = res[way]
            lines.append("  %-8s median %9.2f ms   min %9.2f   max %9.2f   (n = %d; first call %.2f ms)" %
                         (way, s["median_s"] * 1e3, s["min_s"] * 1e3, s["max_s"] * 1e3, s["n"], res["first_call_s"][way] * 1e3))
        lines.append("  loop / grouped (medians): %.2f" % res["speedup_median"])
        lines.append("  kernels of one grouped call (kmu_profile_get):")
        for k, v in res["grouped_profile_ms"].items():
            lines.append("    %-26s %3d launch(es) %10.3f ms" % (k, v["launches"], v["ms"]))
    lines += ["", "box after:"] + ["  " + ln for ln in box_state()]
    text = "\n".join(lines) + "\n"
    sys.stderr.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
