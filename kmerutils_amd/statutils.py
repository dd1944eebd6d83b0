"""Read statistics on the GPU path: mirror of the reference's src/statutils.rs.

`get_base_count_par` (statutils.rs:276-347) gives the table of per-read base percentages and the read-length histogram of a read
set; kmu_read_stats computes both on the device in one call.  The two dumps write the files parsefastq leaves behind:
`bases.histo` (ascii_dump_acgt_distribution, statutils.rs:84-113) and `readlen.histo` (ascii_dump_readlen_distribution,
statutils.rs:118-190, followed step by step).

The length histogram has HdrHistogram's bucket layout (include/kmu.h).  `value_at_quantile` is written from that layout: the
`hdrhistogram` crate's source was not at hand to check its rule to the letter, so `readlen.histo` is NOT claimed to be byte for
byte the reference's; `bases.histo` has no such caveat.
"""
import math
from decimal import Decimal

import numpy as np

from . import _abi as A
from . import lib


def rust_display(x):
    """a float as Rust's `{}` prints it: the shortest decimal that reads back to the same value, never an exponent, no `.0`"""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    s = format(Decimal(repr(x)), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


class ReadBaseDistribution:
    """statutils.rs:38-50.  acgt_distribution: float64 [101, 4], the reads whose base (column A C G T) sits at a percentage (row)
    over the number of reads.  The read sizes: `len_hist`, the counts of the length buckets of (maxreadlen, prec), with histo_out
    the reads beyond them; non_acgt the bytes that are no base."""

    def __init__(self, pct_hist, len_hist, nb_reads, histo_out, non_acgt, maxreadlen, prec):
        self.prec = min(int(prec), 5)  # (statutils.rs:59-66)
        self.upper_histo = int(maxreadlen)
        self.nb_reads = int(nb_reads)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.acgt_distribution = np.asarray(pct_hist, np.float64).reshape(A.RS_PCT_ROWS, 4) * (np.float64(1.) / np.float64(self.nb_reads))
        self.len_hist = np.asarray(len_hist, np.uint64)
        self.histo_out = int(histo_out)
        self.non_acgt = int(non_acgt)

    def readsize_len(self):
        """Histogram::len(): the number of recorded lengths"""
        return int(self.len_hist.sum())

    def value_at_quantile(self, q):
        """the highest length of the first bucket whose running count reaches max(1, ceil(q * recorded)); 0 for an empty histogram.
        (Written from the bucket layout, not checked against the hdrhistogram crate: see the module's note.)"""
        total = self.readsize_len()
        if total == 0:
            return 0
        need = max(1, min(total, int(math.ceil(min(float(q), 1.0) * total))))
        running = np.cumsum(self.len_hist)
        bucket = int(np.searchsorted(running, np.uint64(need), side="left"))
        return lib.len_bucket_range(self.prec, bucket)[1]

    def ascii_dump_acgt_distribution(self, name):
        """101 lines `a c  g  t ` (statutils.rs:96-103)"""
        with open(name, "w") as f:
            for row in self.acgt_distribution:
                f.write("%s %s  %s  %s \n" % tuple(rust_display(v) for v in row))

    def readlen_distribution_lines(self):
        """the lines of ascii_dump_readlen_distribution, or the OSError it returns instead of writing"""
        nb_entries = self.readsize_len()
        if nb_entries == 0:
            return OSError("histogram error!, empty histogram")
        maxlen = nb_entries  # (statutils.rs:127: the number of entries, not a length)
        print("ascii_dump_readlen_distribution nb_entries %d  maxlen %d" % (nb_entries, maxlen))
        if nb_entries < 100:
            print("Error : ascii_dump_readlen_distribution nb_entries too small : %d" % nb_entries)
            return OSError("histogram error!")
        nbslot = nb_entries // 100
        readsize = [self.value_at_quantile(i / nbslot) for i in range(nbslot + 1)]
        nb_points = 1000
        lines = []
        first_i = current_i = 0
        for j in range(nb_points):
            threshold = (maxlen * j) // nb_points
            while readsize[current_i] < threshold and current_i < nbslot:
                current_i += 1
            if current_i < nbslot and current_i > first_i:
                lines.append("%d  %d \n" % (readsize[current_i], ((current_i - first_i) * nb_entries) // nbslot))
            first_i = current_i
        return lines

    def ascii_dump_readlen_distribution(self, name):
        """statutils.rs:118-190: `readsize  nb reads ` lines at regular quantiles.  A histogram of fewer than 100 entries is
        refused: nothing is written and the error is returned (None otherwise)."""
        lines = self.readlen_distribution_lines()
        if isinstance(lines, OSError):
            return lines
        with open(name, "w") as f:
            f.writelines(lines)
        return None


def get_base_count_par(reads, maxreadlen, prec, ctx=None):
    """statutils.rs:276-347 on the device: reads = (bases, offsets), numpy on the host or torch on the device.  (The reference also
    writes `bases.histo` into the working directory here; the caller does that, where it wants the file.)"""
    from .sketching import default_context
    ctx = ctx or default_context()
    bases, offsets = reads
    prec = min(int(prec), 5)
    _, pct_hist, len_hist, info = ctx.read_stats(bases, offsets, maxreadlen, prec, want=("pct", "len"))
    if lib._is_torch(pct_hist):
        pct_hist, len_hist = pct_hist.cpu().numpy().view(np.uint64), len_hist.cpu().numpy().view(np.uint64)
    return ReadBaseDistribution(pct_hist, len_hist, info["n_reads"], info["histo_out"], info["n_other"], maxreadlen, prec)
