"""A plain restatement of the super-k-mer record (kmerutils_amd/csrc/kmu_smer.h) for the tests: numpy and Python only, nothing of
the product.  The record is 96 bits in three 32-bit words; the first base sits in bits 31..30 of word 0, codes A 0, C 1, G 2, T 3,
n_kmers + k - 1 <= 46 bases, zeros behind the last base, and bits 3..0 of word 2 hold n_kmers - 1."""
import numpy as np

CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}  # ACGT, acgt
REC_KMERS = 16


def pack_record(bases, k):
    """(w0, w1, w2) of the record that holds the L = len(bases) - k + 1 k-mers of `bases` (1 <= L <= 16)"""
    L = len(bases) - k + 1
    assert 1 <= L <= REC_KMERS and len(bases) <= 46
    v = 0
    for t, b in enumerate(bytes(bases)):
        v |= CODE[b] << (94 - 2 * t)
    v |= L - 1
    return (v >> 64) & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF, v & 0xFFFFFFFF


def canon_kmers(bases, k):
    """canonical value of every k-mer of `bases`: the forward value and its reverse complement base by base, the smaller of the two"""
    out = np.zeros(max(len(bases) - k + 1, 0), np.uint64)
    mask, f, r = (1 << (2 * k)) - 1, 0, 0
    for t, b in enumerate(bytes(bases)):
        c = CODE[b]
        f = ((f << 2) | c) & mask              # the base enters the forward value at the bottom ...
        r = (r >> 2) | ((3 - c) << (2 * k - 2))  # ... and its complement the reverse complement at the top
        if t >= k - 1:
            out[t - k + 1] = min(f, r)
    return out


def ideal_records(owners_in_read_order, read_kmer_counts, n_parts):
    """int64[n_parts]: the fewest records a sender can emit.  Within every read the maximal runs of consecutive k-mers that share an
    owner; a run of n k-mers needs ceil(n / 16) records, all for its owner."""
    own = np.asarray(owners_in_read_order).astype(np.int64)
    nk = np.asarray(read_kmer_counts, np.int64)
    assert own.size == int(nk.sum())
    if own.size == 0:
        return np.zeros(n_parts, np.int64)
    start = np.zeros(own.size, bool)
    start[0] = True
    start[1:] = own[1:] != own[:-1]
    first = np.cumsum(nk)[:-1]  # the first k-mer of every read but the first (reads without k-mers repeat a position)
    start[first[first < own.size]] = True
    at = np.flatnonzero(start)
    run = np.diff(np.append(at, own.size))
    return np.bincount(own[at], weights=(run + REC_KMERS - 1) // REC_KMERS, minlength=n_parts).astype(np.int64)
