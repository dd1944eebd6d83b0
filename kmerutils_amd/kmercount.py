"""Host-side mirror of the reference's counting interface (src/base/kmercount.rs) on top of libkmu.

  KmerCountT            trait, kmercount.rs:48-59    insert_kmer / get_count / get_nb_distinct / get_nb_unique
  KmerCounter           kmercount.rs:70-123
  KmerCounterPool       kmercount.rs:424-565         one counter per thread -> here one counter per GPU
  count_kmer_threaded_one_to_many   kmercount.rs:881-974
  KmerPrefilter, count_repeated_kmers   (the role of the cuckoo filter of k-mers seen once, kmercount.rs:70-123: a Bloom
                        prefilter built in a first pass keeps them off the table)
The reference's cuckoo + counting-Bloom pair is approximate and randomised per process; the device table is exact,
i.e. the reference's own contract without its ~3 % false positives (counts saturate at 2^nb_bits - 1).
"""
import numpy as np

from . import _abi as A
from . import lib
from .sketching import _as_arrays, default_context


class KmerCounter:
    """KmerCounter::new(fpr, capacity, nb_bits), kmercount.rs:83-98 (fpr is accepted and ignored: the table is exact)"""

    def __init__(self, kmer_size, capacity, nb_bits=8, fpr=0.03, kmer_type=None, ctx=None):
        self.ctx = ctx or default_context()
        self.kmer_type = kmer_type if kmer_type is not None else A.kmer_type_for_k(kmer_size)
        self.kmer_size = kmer_size
        self._c = lib.Counter(self.ctx, self.kmer_type, kmer_size, nb_bits, capacity)

    def insert_kmer(self, compressed_values):
        """KmerCountT::insert_kmer for one value or an array of `get_compressed_value()` values"""
        v = np.atleast_1d(np.asarray(compressed_values, dtype=np.uint64)).copy()
        self._c.add_kmers(v)

    def insert_reads(self, vseq):
        """every canonical k-mer of every read: kmer.reverse_complement().min(kmer), kmercount.rs:313,938"""
        bases, offsets = _as_arrays(vseq)
        self._c.add_reads(bases, offsets)

    def insert_reads_filtered(self, prefilter, vseq):
        """the occurrences of the reads whose k-mer the KmerPrefilter puts in class 2 (may occur twice or more); returns their
        number.  After a filter built from the same reads, get_nb_unique counts the singletons that slipped through it."""
        bases, offsets = _as_arrays(vseq)
        return self._c.add_reads_filtered(prefilter.raw, bases, offsets)

    def get_count(self, compressed_values):
        v = np.atleast_1d(np.asarray(compressed_values, dtype=np.uint64)).copy()
        return self._c.query(v)

    def get_nb_distinct(self):
        return self._c.nb_distinct()

    def get_nb_unique(self):
        return self._c.nb_unique()

    def get_above2_count(self, compressed_values):
        """KmerCounter::get_above2_count (kmercount.rs:100-105): the count if the k-mer was seen at least twice, else 0"""
        c = self.get_count(compressed_values)
        return np.where(c >= 2, c, 0).astype(np.uint32)

    def above2_entries(self):
        """(kmer, count) with count >= 2, sorted by k-mer: what dump_kmer_counter writes (kmercount.rs:500-525)"""
        return self._c.dump(2)

    def eliminate_once_kmer(self):
        """kmercount.rs:110-117: forget the k-mers seen once"""
        self._c.eliminate_once()

    def get_count_histogram(self):
        """the count spectrum: hist[v] = distinct k-mers whose count (saturated at 2^nb_bits - 1) is v; hist[0] is 0"""
        return self._c.histogram()

    def get_reads_abundance(self, vseq, solid_min=2):
        """(counts, stats) of the reads against this counter: the count of the canonical k-mer at every k-mer start
        (counts[offsets[i] + p]) and one A.READ_ABUNDANCE_DTYPE record per read (n_kmers, n_absent, n_once, n_solid -- count >=
        solid_min --, min, median, max, sum)"""
        bases, offsets = _as_arrays(vseq)
        return self._c.read_profile(bases, offsets, solid_min)

    def get_count_nb_bits(self):
        return self._c.p.counter_bits

    @property
    def raw(self):
        return self._c


def count_kmer_threaded_one_to_many(seqvec, nb_threads, count_size, kmer_size, capacity=None, ctx=None):
    """kmercount.rs:881-974.  `nb_threads` is accepted for signature compatibility (the GPU needs no key-space
    dispatch inside one device); `count_size` = bits per counter (8 or 16).  Returns a KmerCounter."""
    bases, offsets = _as_arrays(seqvec)
    if capacity is None:
        capacity = max(1024, int(offsets[-1]))
    kc = KmerCounter(kmer_size, capacity, count_size, ctx=ctx)
    kc.insert_reads((bases, offsets))
    return kc


class KmerPrefilter:
    """The count prefilter (kmu_kfilter): a two-plane Bloom filter that tells the canonical k-mers inserted once from those that
    may have been inserted twice or more.  It stands where the reference keeps its cuckoo filter of k-mers seen once
    (kmercount.rs:70-123): built in a first pass over the reads, it lets a second pass count only what may occur twice.  No k-mer
    inserted twice is ever missed; a k-mer inserted once passes for "more" at the Bloom rate of the first plane."""

    def __init__(self, kmer_size, nb_cells, nb_hashes=4, kmer_type=None, ctx=None):
        self.ctx = ctx or default_context()
        self.kmer_type = kmer_type if kmer_type is not None else A.kmer_type_for_k(kmer_size)
        self.kmer_size = kmer_size
        self._f = lib.KFilter(self.ctx, self.kmer_type, kmer_size, nb_cells, nb_hashes)

    @staticmethod
    def cells_for(expected_distinct, bits_per_kmer=16):
        """cells for that many distinct k-mers at bits_per_kmer bits each (16 bits, 4 hashes: 0.5 % of the singletons pass)"""
        n = lib.kfilter_cells_for(expected_distinct, bits_per_kmer)
        if n == 0:
            raise ValueError("more cells than a filter can have (2^32 - 1)")
        return n

    def insert_reads(self, vseq):
        """one occurrence of every canonical k-mer of every read"""
        bases, offsets = _as_arrays(vseq)
        self._f.add_reads(bases, offsets)

    def insert_kmer(self, compressed_values):
        """one occurrence of one canonical `get_compressed_value()` value, or of every value of an array"""
        self._f.add_kmers(np.atleast_1d(np.asarray(compressed_values, dtype=np.uint64)).copy())

    def seen_class(self, compressed_values):
        """0: never inserted; 1: inserted exactly once; 2: may have been inserted twice or more (uint8 per value)"""
        return self._f.query(np.atleast_1d(np.asarray(compressed_values, dtype=np.uint64)).copy())

    def info(self):
        """n_cells, bytes, n_hashes, kmer_size, n_added, bits_a, bits_b and est_distinct, the estimate of the distinct k-mers"""
        return self._f.info()

    def merge(self, other):
        """this filter becomes the filter of both inputs (same parameters): ranks that each filtered a shard"""
        self._f.merge(other._f)

    def words(self):
        """the planes as uint64 words A0 B0 A1 B1 ..."""
        return self._f.export()

    def nb_passing(self, vseq):
        """how many k-mer occurrences of the reads are class 2: what KmerCounter.insert_reads_filtered is going to add"""
        bases, offsets = _as_arrays(vseq)
        return self._f.n_passing(bases, offsets)

    @property
    def raw(self):
        return self._f


def count_repeated_kmers(seqvec, kmer_size, count_size, bits_per_kmer=16, nb_hashes=4, capacity=None, ctx=None):
    """The counts of the k-mers seen at least twice, without a table slot for (nearly) every singleton: returns
    (KmerCounter, KmerPrefilter).  Two passes over the reads: the filter, sized from the number of k-mer occurrences at
    bits_per_kmer bits each, then the table, which gets the occurrences of class-2 k-mers only.  Every count held is exact and
    every k-mer seen at least twice is held, so get_above2_count and above2_entries answer as after
    count_kmer_threaded_one_to_many; a k-mer that is absent occurred 0 or 1 times, and get_nb_unique counts the singletons that
    slipped through the filter.

    capacity: the distinct k-mers the table is made for.  Default: the number P of passing occurrences, which can never overflow
    (R repeated and F slipped k-mers make P >= 2 R + F >= R + F).  A caller may pass something tighter from
    info().est_distinct - (info()["n_added"] - P): the distinct k-mers of the reads less the occurrences that did not pass, each of
    them a k-mer of its own."""
    bases, offsets = _as_arrays(seqvec)
    ctx = ctx or default_context()
    off_h = offsets.cpu().numpy() if lib._is_torch(offsets) else np.asarray(offsets)
    occurrences = int(np.maximum(np.diff(off_h.astype(np.int64)) - kmer_size + 1, 0).sum())
    kf = KmerPrefilter(kmer_size, KmerPrefilter.cells_for(occurrences, bits_per_kmer), nb_hashes, ctx=ctx)
    kf.insert_reads((bases, offsets))
    passing = kf.nb_passing((bases, offsets))
    kc = KmerCounter(kmer_size, max(1024, passing if capacity is None else int(capacity)), count_size, ctx=ctx)
    kc.insert_reads_filtered(kf, (bases, offsets))
    return kc, kf


class KmerFilter1:
    """KmerFilter1 (kmercount.rs:985-1089): which 16-mers occur exactly once, and where.  Upstream keeps two cuckoo filters
    (approximate, randomised); here the exact device table answers the same questions.  `insert_reads` stands for the loop
    of filter1_kmer_16b32bit (generate, canonicalise, insert)."""

    def __init__(self, size=16, capacity=1 << 20, ctx=None):
        if size != 16:
            raise ValueError("KmerFilter1 holds Kmer16b32bit")
        self.kmer_size = size
        self.ctx = ctx or default_context()
        self._c = lib.Counter(self.ctx, A.KMER16B32BIT, 16, 8, capacity)

    def insert_kmer16b32bit(self, canonical_values):
        self._c.add_kmers(np.atleast_1d(np.asarray(canonical_values, dtype=np.uint64)).copy())

    def insert_reads(self, vseq):
        bases, offsets = _as_arrays(vseq)
        self._c.add_reads(bases, offsets)

    def get_nb_once(self):
        """once_f.len()"""
        return self._c.nb_unique()

    def once_positions(self, vseq):
        """(kmin, numseq, numkmer) of every occurrence of a once-k-mer in the reads, in file order"""
        bases, offsets = _as_arrays(vseq)
        return self._c.once_positions(bases, offsets)

    def dump_in_file_once_kmer16b32bit(self, fname, seqvec):
        """kmercount.rs:1031-1082; returns the number of k-mers dumped"""
        from . import formats
        k, s, p = self.once_positions(seqvec)
        return formats.dump_once_kmers(fname, np.asarray(k), np.asarray(s), np.asarray(p), 16, 4)


def filter1_kmer_16b32bit(seqvec, ctx=None):
    """kmercount.rs:1093-1123: a KmerFilter1 fed with the canonical 16-mers of every sequence"""
    bases, offsets = _as_arrays(seqvec)
    f = KmerFilter1(16, max(1024, int(offsets[-1])), ctx=ctx)
    f.insert_reads((bases, offsets))
    return f
