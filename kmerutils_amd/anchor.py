"""Read anchors: bottom-k sketches of overlapping windows of reads (the reference's src/anchor.rs, without its redis storage).

`gen_read_anchors` runs kmu_read_anchors over a batch of reads; `ReadAnchors` / `SliceAnchor` are views over the arrays it
returns, named like the reference's structs; `anchors_by_minhash` is the inverse index min hash -> [(readnum, slicepos)] that
the reference's `redis_dump` stores under MINHASH_1, as a plain dict on the host; `match_read_anchors` is the join that index
exists for, on the device (kmu_anchor_match), and `rows_to_slices` names its rows; `read_overlaps` goes on from the matched
slices to read pairs (kmu_anchor_overlaps), and `read_clusters` from those to the sets of reads that belong together
(kmu_components).  All three take `max_occ`, the repeat mask of the anchor index (ctx.anchor_index), and `max_occ_for_fraction`
chooses it from the index's occupancy histogram.
"""
import numpy as np

from . import _abi as A
from . import parsefastq


class AnchorsGeneratorParameters:
    """AnchorsGeneratorParameters::new(fasta_name, window, nbkmer, kmer_size, overlap) (anchor.rs:29-78)"""

    def __init__(self, fasta_name, window, nbkmer, kmer_size, overlap):
        self.fasta_name = str(fasta_name)
        self.window = int(window)
        self.nbkmer = int(nbkmer)
        self.kmer_size = int(kmer_size)
        self.overlap = int(overlap)

    def get_fasta_name(self):
        return self.fasta_name

    def get_window(self):
        return self.window

    def get_nbkmer(self):
        return self.nbkmer

    def get_kmer_size(self):
        return self.kmer_size

    def get_overlap(self):
        return self.overlap

    def get_stride(self):
        """window - overlap: the distance between the starts of two consecutive slices (anchor.rs:318)"""
        return self.window - self.overlap

    def sketch_params(self, hasher=A.HASHER_INT64HASH, fhash=A.FHASH_VALUE_MASKED):
        """the kmu_sketch_params of these anchors; the defaults are the reference's MinInvHashCountKmer: forward k-mers,
        int64_hash(get_compressed_value()), u8 counts.  fhash=A.FHASH_CANON_VALUE gives strand-independent anchors."""
        kmer_type, _ = parsefastq.kmer_type_for(self.kmer_size)
        return A.SketchParams(A.ALGO_BOTTOMK, kmer_type, self.kmer_size, self.nbkmer, A.SIG_U64, hasher, fhash, 0,
                              A.MODE_PER_SEQ, A.INPUT_ASCII, A.MEM_HOST, 0)

    def __str__(self):
        return "slice size : %d nb kmer : %d kmer size : %d overlap : %d" % (self.window, self.nbkmer, self.kmer_size, self.overlap)


class SliceAnchor:
    """SliceAnchor (anchor.rs:97-105): one window of a read.  readnum, slicepos (first base of the slice in its read) and
    minhash: the (hash, count) pairs of the slice, ascending by hash; empty for a slice that holds no k-mer."""

    def __init__(self, params, readnum, slicepos, hashes, counts, n):
        self.params = params
        self.readnum = int(readnum)
        self.slicepos = int(slicepos)
        self._hashes, self._counts, self._n = hashes, counts, int(n)

    @property
    def minhash(self):
        c = self._counts
        return [(int(self._hashes[t]), int(c[t]) if c is not None else None) for t in range(self._n)]

    def get_minhash_key(self):
        """the smallest hash of the slice: its key in the inverse index (get_minhash_key_for_redis, anchor.rs:149-158)"""
        if self._n == 0:
            raise IndexError("slice %d:%d holds no k-mer" % (self.readnum, self.slicepos))
        return int(self._hashes[0])


class ReadAnchors:
    """ReadAnchors (anchor.rs:265-329): the slices of one read, a view over rows [row_begin, row_end) of the arrays"""

    def __init__(self, params, readnum, hashes, counts, n, row_begin, row_end):
        self.slice_params = params
        self.readnum = int(readnum)
        self._hashes, self._counts, self._n = hashes, counts, n
        self._rows = (int(row_begin), int(row_end))

    def get_nb_slice(self):
        return self._rows[1] - self._rows[0]

    @property
    def anchors(self):
        stride = self.slice_params.get_stride()
        b, e = self._rows
        return [SliceAnchor(self.slice_params, self.readnum, (r - b) * stride, self._hashes[r],
                            self._counts[r] if self._counts is not None else None, self._n[r]) for r in range(b, e)]

    def __len__(self):
        return self.get_nb_slice()

    def __getitem__(self, s):
        return self.anchors[s]


def _host(x):
    """a numpy view of the bits of a result array (device tensors come back as int64 / int32)"""
    if x is None:
        return None
    if type(x).__module__.startswith("torch"):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x)
    return x.view({8: np.uint64, 4: np.uint32}[x.dtype.itemsize])


def gen_read_anchors(ctx, bases, offsets, params, first_readnum=0, hasher=A.HASHER_INT64HASH, fhash=A.FHASH_VALUE_MASKED,
                     want_counts=True):
    """ReadAnchors::generate_anchors for every read of a batch, in one library call: a list of ReadAnchors, read i of the batch
    numbered first_readnum + i.  `bases` / `offsets`: numpy arrays or torch cuda tensors (the rows come back to the host)."""
    hashes, counts, n, rows = ctx.read_anchors(bases, offsets, params.sketch_params(hasher, fhash), params.get_window(),
                                               params.get_overlap(), want_counts=want_counts)
    hashes, counts, n = _host(hashes), _host(counts), _host(n)
    return [ReadAnchors(params, first_readnum + i, hashes, counts, n, rows[i], rows[i + 1]) for i in range(len(rows) - 1)]


def anchors_by_minhash(hashes, n, row_offsets, stride, first_readnum=0):
    """The inverse index of `redis_dump` (MINHASH_1, anchor.rs:187-197): {smallest hash of a slice: [(readnum, slicepos), ...]}
    in row order.  hashes [rows, nbkmer], n [rows], row_offsets [n_reads + 1] as kmu_read_anchors gives them; slices with n = 0
    are skipped (their minhash[0] does not exist)."""
    hashes, n = _host(hashes), _host(n)
    row_offsets = np.asarray(row_offsets).astype(np.int64)
    index = {}
    for i in range(len(row_offsets) - 1):
        for r in range(int(row_offsets[i]), int(row_offsets[i + 1])):
            if n[r] == 0:
                continue
            index.setdefault(int(hashes[r, 0]), []).append((first_readnum + i, (r - int(row_offsets[i])) * int(stride)))
    return index


def rows_to_slices(rows, row_offsets, stride, first_readnum=0):
    """(readnum, slicepos) of anchor rows: row r of a batch laid out by kmu_anchor_layout belongs to the read i with
    row_offsets[i] <= r < row_offsets[i + 1], numbered first_readnum + i, and starts at base (r - row_offsets[i]) * stride of it.
    Pure numpy; `rows` of any shape, two int64 arrays of that shape back."""
    rows = np.asarray(rows).astype(np.int64)
    row_offsets = np.asarray(row_offsets).astype(np.int64)
    read = np.searchsorted(row_offsets, rows, side="right") - 1
    return read + int(first_readnum), (rows - row_offsets[read]) * int(stride)


def max_occ_for_fraction(hist, frac):
    """The `max_occ` that drops the most frequent seeds: the smallest c such that at most `frac` of the distinct keys have an
    occupancy above c.  hist: AnchorIndex.occupancy(n_bins) -- hist[c] = keys carried by c database rows, the last bin folded;
    choose n_bins above max_occupancy, or the answer cannot pass the last bin.  Pure numpy.  frac = 0 gives the largest occupancy
    present (nothing is masked), frac >= 1 and an empty histogram give 0 -- which, as max_occ, also means "no mask"."""
    hist = np.asarray(hist).astype(np.int64)
    total = int(hist.sum())
    if total == 0:
        return 0
    above = total - np.cumsum(hist)  # above[c] = keys with occupancy > c; above[-1] = 0
    return int(np.nonzero(above <= max(float(frac), 0.0) * total)[0][0])


def _self_join(ctx, hashes, group, n_keys, min_common, max_occ):
    """the window pairs of a batch against itself: ctx.anchor_match, or with a repeat mask an index of the batch"""
    if not max_occ:
        return ctx.anchor_match(hashes, hashes, n_keys=n_keys, min_common=min_common, group_q=group, group_db=group)
    with ctx.anchor_index(hashes, n_keys=n_keys, group_db=group) as index:
        return index.match(hashes, group_q=group, min_common=min_common, max_occ=max_occ)


def match_read_anchors(ctx, hashes, row_offsets, params, n_keys=1, min_common=1, first_readnum=0, max_occ=0):
    """The slices of a batch that share one of their n_keys smallest hashes and belong to different reads: kmu_anchor_match as a
    self-join of the rows `hashes` (ctx.read_anchors: numpy, or torch on the device -- the join then runs on the resident rows)
    with group = read of the row.  What a lookup of every slice in the reference's inverse index (redis_dump, anchor.rs:187-197)
    finds, with mininvhash_distance for each hit.  Returns an int64 array [n, 6] of records (readnum_a, slicepos_a, readnum_b,
    slicepos_b, common, total), ordered by row a, shared hash, row b; (a, b) and (b, a) are both there.  max_occ > 0: hashes that
    are keys of more than max_occ slices seed no pair (kmu_anchor_index_match on an index of the batch)."""
    row_offsets = np.asarray(row_offsets).astype(np.int64)
    group = _read_groups(hashes, row_offsets)
    pairs, dist = _self_join(ctx, hashes, group, n_keys, min_common, max_occ)
    pairs, dist = _host(pairs).astype(np.int64), _host(dist).astype(np.int64)
    out = np.zeros((pairs.shape[0], 6), np.int64)
    out[:, 0], out[:, 1] = rows_to_slices(pairs[:, 0], row_offsets, params.get_stride(), first_readnum)
    out[:, 2], out[:, 3] = rows_to_slices(pairs[:, 1], row_offsets, params.get_stride(), first_readnum)
    out[:, 4:6] = dist[:, 0:2]
    return out


def _read_groups(hashes, row_offsets):
    """the read of every row, as the group array of a self-join (on the device when the rows are)"""
    group = np.ascontiguousarray(rows_to_slices(np.arange(int(hashes.shape[0])), row_offsets, 1)[0].astype(np.uint32))
    if type(hashes).__module__.startswith("torch") and hashes.is_cuda:
        import torch
        group = torch.from_numpy(group.view(np.int32)).to(hashes.device)
    return group


def read_overlaps(ctx, hashes, row_offsets, params, n_keys=1, min_common=1, strands=2, band=1, min_score=2, first_readnum=0,
                  max_occ=0):
    """Which reads of a batch overlap: the self-join of match_read_anchors followed by kmu_anchor_overlaps, each read pair once
    (read a in front of read b in the batch).  With `hashes` on the device the matched slices never leave it.  The weight of a
    matched pair of slices is its `common`; `band` + 1 neighbouring diagonals vote together; strands=2 also looks for read b on
    the opposite strand (rows made with fhash=A.FHASH_CANON_VALUE), where the diagonal is the SUM of the two slice numbers.
    Returns an int64 array [n, 8] of records (readnum_a, readnum_b, strand, offset in bases = diag * stride, score, votes, first
    and last slicepos_a of the band), ordered by readnum_a, readnum_b.  max_occ > 0: the repeat mask of match_read_anchors."""
    row_offsets = np.asarray(row_offsets).astype(np.int64)
    group = _read_groups(hashes, row_offsets)
    pairs, dist = _self_join(ctx, hashes, group, n_keys, min_common, max_occ)
    rec = ctx.anchor_overlaps(pairs, dist, row_offsets.astype(np.uint64), strands=strands, band=band, min_score=min_score, upper=True)
    if type(rec).__module__.startswith("torch"):
        rec = rec.cpu().numpy()
    rec = np.ascontiguousarray(rec).view(np.dtype(A.OVERLAP_DTYPE)).reshape(-1)
    stride = params.get_stride()
    out = np.zeros((rec.shape[0], 8), np.int64)
    out[:, 0] = rec["read_a"].astype(np.int64) + int(first_readnum)
    out[:, 1] = rec["read_b"].astype(np.int64) + int(first_readnum)
    out[:, 2] = rec["strand"]
    out[:, 3] = rec["diag"].astype(np.int64) * stride
    out[:, 4] = rec["score"]
    out[:, 5] = rec["votes"]
    out[:, 6] = rec["slice_a_min"].astype(np.int64) * stride
    out[:, 7] = rec["slice_a_max"].astype(np.int64) * stride
    return out


def read_clusters(ctx, hashes, row_offsets, params, n_keys=1, min_common=1, strands=2, band=1, min_score=2, first_readnum=0,
                  max_occ=0, by="score", want_members=False):
    """Which reads of a batch belong together: the self-join and the vote of read_overlaps, then the connected components of the
    graph whose nodes are the reads and whose edges are the overlap records that count (kmu_components on the records as they
    are: stride 8).  by="score": a record counts iff its score >= min_score (word 4); by="votes": iff its votes >= min_score (word
    5; the vote itself then drops nothing).  With `hashes` on the device neither the matched slices nor the records leave it.
    Returns (cluster int64 [n_reads], sizes int64 [n_clusters]): the cluster of every read -- clusters are numbered in the order
    of their first read -- and the number of reads in each; a read that overlaps nothing is a cluster of one.  want_members=True
    adds the read numbers (from first_readnum) ordered by (cluster, read): cluster c is members[sizes[:c].sum():][:sizes[c]]."""
    if by not in ("score", "votes"):
        raise ValueError("by must be 'score' or 'votes'")
    row_offsets = np.asarray(row_offsets).astype(np.int64)
    n_reads = int(row_offsets.shape[0]) - 1
    group = _read_groups(hashes, row_offsets)
    pairs, dist = _self_join(ctx, hashes, group, n_keys, min_common, max_occ)
    rec = ctx.anchor_overlaps(pairs, dist, row_offsets.astype(np.uint64), strands=strands, band=band,
                              min_score=min_score if by == "score" else 0, upper=True)
    want = ("cluster", "size", "members") if want_members else ("cluster", "size")
    res = ctx.components(rec, n_reads, weight_at=4 if by == "score" else 5, min_weight=min_score, want=want)
    cluster, sizes = _host(res.cluster).astype(np.int64), _host(res.size).astype(np.int64)
    if not want_members:
        return cluster, sizes
    return cluster, sizes, _host(res.members).astype(np.int64) + int(first_readnum)
