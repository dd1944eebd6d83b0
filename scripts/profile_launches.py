#!/usr/bin/env python3
"""The timed kernel names and launch counts of one small call per family of entry points: one JSON line {call: {name: launches}}.
Two builds of the library that print the same line time the same kernels the same number of times (KMU_LIB picks the library).
Inputs: a few dozen synthetic reads of a few kilobases, fixed seeds, host arrays."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kmerutils_amd import _abi as A  # noqa: E402
from kmerutils_amd import lib, synth  # noqa: E402

DNA_FH = A.FHASH_CANON_INVHASH


def sketch_params(algo, k=31, m=200, sig=A.SIG_U64, mode=A.MODE_PER_SEQ):
    return A.SketchParams(algo, A.KMER64BIT, k, m, sig, A.HASHER_NOHASH, DNA_FH, 0, mode, 0, 0, 0)


def fastq_of(bases, off):
    recs = []
    for i in range(len(off) - 1):
        seq = bases[int(off[i]):int(off[i + 1])].tobytes()
        recs.append(b"@r%d\n%s\n+\n%s\n" % (i, seq, b"I" * len(seq)))
    return b"".join(recs)


def main():
    ctx = lib.Context(0)
    ctx.profile_enable(True)
    out = {}

    def record(name, fn):
        ctx.profile_reset()
        res = fn()
        ctx.synchronize()
        out[name] = {k: v[0] for k, v in sorted(ctx.profile_get().items())}
        return res

    bases, off = synth.ont_reads(48, 400_000, 0xA1, mean_len=3000)
    short_b, short_o = synth.uniform_reads(40, 150, 0xA2)
    pmh = sketch_params(A.ALGO_PROB3A)
    record("sketch_pmh3a_per_read", lambda: ctx.sketch(bases, off, pmh))
    record("sketch_pmh3a_short_reads", lambda: ctx.sketch(short_b, short_o, pmh))
    record("sketch_pmh3a_all_seqs", lambda: ctx.sketch(bases, off, sketch_params(A.ALGO_PROB3A, mode=A.MODE_ALL_SEQS)))
    record("sketch_super_per_read", lambda: ctx.sketch(bases, off, sketch_params(A.ALGO_SUPER, k=21, m=64, sig=A.SIG_F64)))
    record("sketch_super_all_seqs",
           lambda: ctx.sketch(bases, off, sketch_params(A.ALGO_SUPER, k=21, m=64, sig=A.SIG_F64, mode=A.MODE_ALL_SEQS)))
    record("sketch_optdens_per_read", lambda: ctx.sketch(bases, off, sketch_params(A.ALGO_OPTDENS, k=21, m=64, sig=A.SIG_F64)))
    record("sketch_optdens_all_seqs",
           lambda: ctx.sketch(bases, off, sketch_params(A.ALGO_OPTDENS, k=21, m=64, sig=A.SIG_F64, mode=A.MODE_ALL_SEQS)))
    groups = np.array([0, 10, 11, 30, 48], np.uint64)
    record("sketch_groups_pmh3a", lambda: ctx.sketch_groups(bases, off, groups, sketch_params(A.ALGO_PROB3A, mode=A.MODE_ALL_SEQS)))
    record("sketch_groups_optdens",
           lambda: ctx.sketch_groups(bases, off, groups, sketch_params(A.ALGO_OPTDENS, k=21, m=64, sig=A.SIG_F64, mode=A.MODE_ALL_SEQS)))

    counter = None
    for path in ("partitioned", "direct"):
        os.environ["KMU_COUNT_PATH"] = path
        c = ctx.counter(A.KMER64BIT, 31, 8, 1 << 20)
        record("count_add_reads_" + path, lambda: c.add_reads(bases, off))
        if counter is None:
            counter = c
        else:
            c.close()
    os.environ.pop("KMU_COUNT_PATH")
    record("count_dump", lambda: counter.dump(1))
    record("count_histogram", lambda: counter.histogram())
    record("count_read_profile", lambda: counter.read_profile(bases, off))
    counter.close()

    record("kmer_hashes", lambda: ctx.kmer_hashes(bases, off, A.KMER64BIT, 31, DNA_FH))
    record("nthash", lambda: ctx.nthash(bases, off, 31))
    record("ingest_fastq", lambda: ctx.ingest_fastq(fastq_of(bases, off)))

    bk = sketch_params(A.ALGO_BOTTOMK, k=21, m=32)
    hashes, _, _, rows = record("read_anchors", lambda: ctx.read_anchors(bases, off, bk, 1000, 200))
    pairs, dist = record("anchor_match", lambda: ctx.anchor_match(hashes, hashes, n_keys=4))
    index = record("anchor_index_create", lambda: ctx.anchor_index(hashes, n_keys=4))
    record("anchor_index_match", lambda: index.match(hashes, max_occ=8))
    record("anchor_index_occupancy", lambda: index.occupancy(16))
    index.close()
    overlaps = record("anchor_overlaps", lambda: ctx.anchor_overlaps(pairs, dist, rows))
    record("components", lambda: ctx.components(overlaps, len(off) - 1))

    sig = ctx.sketch(bases, off, pmh)
    idx, eq = record("sig_knn", lambda: ctx.sig_knn(sig, sig, 4, group_q=np.arange(len(sig), dtype=np.uint32),
                                                    group_db=np.arange(len(sig), dtype=np.uint32)))
    record("components_knn", lambda: ctx.components_knn(idx, eq, min_eq=1))
    ctx.close()
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
