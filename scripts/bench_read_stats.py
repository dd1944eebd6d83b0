#!/usr/bin/env python3
"""The read statistics, timed beside what one had to do without them.

Device-resident ONT-shaped synthetic reads (kmerutils_amd.synth.ont_reads_device: 20 000 reads, about 100 Mbases).  Host clock
around synchronous calls on the context's stream, median / min / max of --repeats runs after a warm-up:
  read_stats_ms         kmu_read_stats with all outputs (per-read records, the 101 x 4 table, the length histogram, the totals)
  count_non_acgt_ms     kmu_count_non_acgt on the same batch: one walk over the same bytes, one number per read
  kernel_ms             per launch, by HIP events: the kernels of kmu_read_stats and of kmu_count_non_acgt (where a call's time goes)
  host_bincount_ms      the bases copied to the host and numpy.bincount per read: the only other way to the composition of a read
  read_qual_stats_ms    kmu_read_qual_stats on quality bytes laid out as the bases are
  ingest_fastq_ms / ingest_fastq_qual_ms   the two ingests of a FASTQ text synthesised from the same reads (resident on the device)
Every device time is also given as the share of the HBM rate (--hbm-gbs, 8000 GB/s by default) that reading the bytes once at that
speed amounts to.  One JSON line, also written to --out.

  scripts/bench_read_stats.py [--reads 20000] [--bases 100000000] [--genome 50000000] [--repeats 5] [--hbm-gbs 8000] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000)
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kmerutils_amd import lib, synth
    dev = torch.device("cuda", 0)
    bases, off, lens = synth.ont_reads_device(args.reads, args.bases, args.genome, 0xC4, dev)
    n_bases = int(lens.sum())
    ctx = lib.Context(0)

    def timed(fn):
        ts = []
        for i in range(args.repeats + 1):  # (the first run warms up: workspaces, pages)
            ctx.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            torch.cuda.synchronize()
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        return stat(ts)

    def hbm_share(ms, n_bytes):
        return n_bytes / (ms * 1e-3) / (args.hbm_gbs * 1e9)

    res = {"reads": args.reads, "bases": n_bases, "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "hbm_gbs": args.hbm_gbs}
    n_buckets, _ = lib.len_hist_layout(1_000_000, 3)
    into = (torch.zeros((args.reads, 12), dtype=torch.int32, device=dev), torch.zeros((101, 4), dtype=torch.int64, device=dev),
            torch.zeros(n_buckets, dtype=torch.int64, device=dev))
    res["read_stats_ms"] = timed(lambda: ctx.read_stats(bases, off, into=into))
    res["count_non_acgt_ms"] = timed(lambda: ctx.count_non_acgt(bases, off))
    h_off = off.cpu().numpy()

    def host_way():
        h = bases.cpu().numpy()
        return [np.bincount(h[h_off[i]:h_off[i + 1]], minlength=256) for i in range(args.reads)]
    res["host_bincount_ms"] = timed(host_way)
    # where the time of a call goes: the kernels' own times by HIP events (the rest is the host's: memsets, launches, the read-back)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(args.repeats):
        ctx.read_stats(bases, off, into=into)
        ctx.count_non_acgt(bases, off)
    res["kernel_ms"] = {name: round(ms / n, 4) for name, (n, ms) in ctx.profile_get().items()}
    ctx.profile_enable(False)
    info = ctx.read_stats(bases, off, into=into)[3]
    assert info["n_bases"] == n_bases and info["n_other"] == 0 and sum(info["n_base"]) == n_bases
    # qualities: bytes over the whole class range, laid out as the bases are; and a FASTQ text of the same reads
    g = torch.Generator(device=dev)
    g.manual_seed(0xC5)
    quals = torch.randint(0x21, 0x4B, (n_bases + 64,), dtype=torch.uint8, device=dev, generator=g)[:n_bases]
    res["read_qual_stats_ms"] = timed(lambda: ctx.read_qual_stats(quals, off))
    h_bases, h_quals = bases.cpu().numpy()[:n_bases], quals.cpu().numpy()
    parts = []
    for i in range(args.reads):
        parts += [b"@r%d\n" % i, h_bases[h_off[i]:h_off[i + 1]].tobytes(), b"\n+\n", h_quals[h_off[i]:h_off[i + 1]].tobytes(), b"\n"]
    text = np.frombuffer(b"".join(parts), np.uint8)
    d_text = torch.zeros(text.size + 64, dtype=torch.uint8, device=dev)
    d_text[:text.size] = torch.from_numpy(text.copy()).to(dev)
    d_text = d_text[:text.size]
    res["text_bytes"] = int(text.size)
    res["ingest_fastq_ms"] = timed(lambda: ctx.ingest_fastq(d_text))
    res["ingest_fastq_qual_ms"] = timed(lambda: ctx.ingest_fastq_qual(d_text))
    got = ctx.ingest_fastq_qual(d_text)
    assert torch.equal(got[0], bases[:n_bases]) and torch.equal(got[1], quals)
    for name, n_bytes in (("read_stats_ms", n_bases), ("count_non_acgt_ms", n_bases), ("read_qual_stats_ms", n_bases),
                          ("ingest_fastq_ms", text.size), ("ingest_fastq_qual_ms", text.size)):
        res[name.replace("_ms", "_hbm_share")] = round(hbm_share(res[name]["median"], n_bytes), 4)
    res["read_stats_over_count_non_acgt"] = round(res["read_stats_ms"]["median"] / res["count_non_acgt_ms"]["median"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
