"""`parsefastq -f reads.fastq kmer --count -s 31` on the GPU path.

Mirror of the counting branch of the reference's tool (src/bin/parsefastq.rs:205-236): the FASTQ file is parsed and
filtered on the device, every canonical k-mer of the accepted reads is counted (`count_kmer_threaded_one_to_many`,
src/base/kmercount.rs:881-974) and the k-mers seen at least twice are written to `<file>.multi_kmer.bin` in the
reference's dump format (`threaded_dump_kmer_counter` / `dump_kmer_counter`, kmercount.rs:467-531, :653-791).  The
k-mer type follows the tool: Kmer64bit for 16 < k <= 32 (here: <= 31, k = 32 is broken upstream), Kmer16b32bit for
k == 16, Kmer32bit for k <= 14.

`--repeated [--filter-bits N]` counts through the Bloom prefilter (kmercount.count_repeated_kmers' order of calls): two passes
over the reads, the k-mers seen once stay off the table, and the dump is byte for byte that of the plain count.

`--stats` is what the reference's tool does before it counts (parsefastq.rs:193-203): `get_base_count_par(reads, 1000000, 3)`, then
`bases.histo` and `readlen.histo` in --outdir, and for a FASTQ text `quality.histo`, eight lines `class<TAB>number of bases` of the
kept reads' qualities (remap_quality8).  Off by default: a run without it writes what it always wrote.  This tool has no task word
(it always counted), so `--stats --no-count` is the statistics alone, what the C++ tool does for `--stats` without a `kmer` task.
"""
import argparse
import os
import sys
import time

import numpy as np

from . import _abi as A
from . import formats, lib


def kmer_type_for(k):
    if 16 < k <= 31:
        return A.KMER64BIT, 8
    if k == 16:
        return A.KMER16B32BIT, 4
    if 1 <= k <= 14:
        return A.KMER32BIT, 4
    raise ValueError("no k-mer type for k = %d (parsefastq.rs:215-236)" % k)


def write_stats(ctx, bases, quals, offsets, outdir):
    """parsefastq.rs:193-203: bases.histo, readlen.histo (its refusal of fewer than 100 reads is discarded, as upstream) and, where
    there are qualities, quality.histo"""
    from . import statutils
    dist = statutils.get_base_count_par((bases, offsets), 1000000, 3, ctx=ctx)
    print("nb read outside max size for histogram %d" % dist.histo_out, file=sys.stderr)  # statutils.rs:338-341
    dist.ascii_dump_acgt_distribution(os.path.join(outdir, "bases.histo"))
    dist.ascii_dump_readlen_distribution(os.path.join(outdir, "readlen.histo"))
    if quals is not None:
        _, hist = ctx.read_qual_stats(quals, offsets, want=("hist",))
        with open(os.path.join(outdir, "quality.histo"), "w") as f:
            for c in range(A.RS_QUAL_CLASSES):
                f.write("%d\t%d\n" % (c, hist[c]))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="parsefastq", description=__doc__.splitlines()[0])
    ap.add_argument("-f", "--file", required=True)
    ap.add_argument("-s", "--kmer_size", type=int, default=16)
    ap.add_argument("--outdir", default=".", help="directory of <file>.multi_kmer.bin (the tool writes to the cwd)")
    ap.add_argument("--unique", action="store_true", help="dump the 16-mers seen exactly once with their positions "
                    "(KmerProcessing::Unicity, parsefastq.rs:238-247) instead of counting")
    ap.add_argument("--histo", metavar="FILE", help="after the count: the count spectrum, one `count<TAB>number of distinct "
                    "k-mers` line per non-empty bin, ascending")
    ap.add_argument("--repeated", action="store_true", help="count through the Bloom prefilter (count_repeated_kmers): two passes "
                    "over the reads, the k-mers seen once stay off the table; the dump is that of the plain count")
    ap.add_argument("--filter-bits", type=int, default=16, metavar="N", help="with --repeated: filter bits per k-mer occurrence")
    ap.add_argument("--stats", action="store_true", help="before the count: bases.histo, readlen.histo and (FASTQ) quality.histo in "
                    "--outdir (get_base_count_par, parsefastq.rs:193-203)")
    ap.add_argument("--no-count", action="store_true", help="with --stats: write the statistics and stop (this tool has no `kmer` task "
                    "word to leave out, as the C++ tool has)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.no_count and (not args.stats or args.unique or args.repeated or args.histo):
        ap.error("--no-count goes with --stats alone")
    if args.repeated and args.histo:
        ap.error("--histo with --repeated: the table holds no singletons, bin 1 would be meaningless")
    if args.repeated and args.unique:
        ap.error("--repeated goes with the count, not with --unique")
    kmer_type, val_bytes = kmer_type_for(args.kmer_size)
    ctx = lib.Context(args.device)
    t0 = time.time()
    text = np.fromfile(args.file, dtype=np.uint8)
    quals = None
    if args.stats and text.size and text[0] == ord("@"):
        bases, quals, offsets, info = ctx.ingest_fastq_qual(text)
    else:
        bases, offsets, info = ctx.ingest_fastx(text)
    print(" nb rec loaded = %d \nnb_bases %d\nnb_bad_bases %d\nnb_bad_read %d" %
          (info.n_kept, info.n_bases, info.nb_bad_bases, info.nb_bad_reads), file=sys.stderr)  # io.rs:63-68
    if args.stats:
        write_stats(ctx, bases, quals, offsets, args.outdir)
    if args.no_count:
        ctx.close()
        return 0
    if args.unique:  # filter1_kmer_16b32bit + dump_in_file_once_kmer16b32bit -> <file>.once_kmer.bin
        from . import kmercount
        flt = kmercount.KmerFilter1(16, max(1024, int(info.kept_bases)), ctx=ctx)
        if info.n_kept:
            flt.insert_reads((bases, offsets))
        out = os.path.join(args.outdir, os.path.basename(args.file) + ".once_kmer.bin")
        print("dumping unique kmers in file : %s " % out, file=sys.stderr)
        n = flt.dump_in_file_once_kmer16b32bit(out, (bases, offsets)) if info.n_kept else formats.dump_once_kmers(out, [], [], [], 16)
        print("dump_in_file_once_kmer16b32bit, number of kmer dumped : %d " % n, file=sys.stderr)
        ctx.close()
        return 0
    nk = int(np.maximum(np.diff(offsets.astype(np.int64)) - args.kmer_size + 1, 0).sum())
    if args.repeated and info.n_kept:  # the filter, the number of occurrences that pass it, the table for those alone
        kf = ctx.kfilter(kmer_type, args.kmer_size, lib.kfilter_cells_for(nk, args.filter_bits) or A.KFILTER_MAX_CELLS)
        kf.add_reads(bases, offsets)
        passing = kf.n_passing(bases, offsets)
        counter = ctx.counter(kmer_type, args.kmer_size, 8, max(passing, 1024))
        counter.add_reads_filtered(kf, bases, offsets)
        print("prefilter: %d of %d k-mer occurrences passed, filter bytes %d, estimated distinct %.0f" %
              (passing, nk, kf.info()["bytes"], kf.info()["est_distinct"]), file=sys.stderr)
        kf.close()
    else:
        counter = ctx.counter(kmer_type, args.kmer_size, 8, max(nk, 1024))
        if info.n_kept:
            counter.add_reads(bases, offsets)
    kmers, counts = counter.dump(2)
    out = os.path.join(args.outdir, os.path.basename(args.file) + ".multi_kmer.bin")  # parsefastq.rs:207-211
    print("dumping multiple kmers in file : %s " % out, file=sys.stderr)
    n = formats.dump_kmer_counter(out, kmers, counts, args.kmer_size, val_bytes)
    print("dump_kmer_counter, number of kmer dumped : %d (distinct %d, unique %d), elapsed time (s) %.3f" %
          (n, counter.nb_distinct(), counter.nb_unique(), time.time() - t0), file=sys.stderr)
    if args.histo:
        hist = counter.histogram()
        with open(args.histo, "w") as f:
            for v in np.flatnonzero(hist):
                f.write("%d\t%d\n" % (v, hist[v]))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
