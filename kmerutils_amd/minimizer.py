"""Window minimizers of reads: base-resolution seeds, and the hits between them.

`read_minimizers` runs kmu_read_minimizers over a batch of reads and returns a `Minimizers` record; `read_syncmers` runs
kmu_read_syncmers and returns a `Syncmers` record, which everything below takes in a Minimizers record's place; `seed_hits` joins the
minimizers of different reads that carry the same hash.  The join is the anchor index as it is (ctx.anchor_index /
AnchorIndex.match): every minimizer is a row of ONE hash (m = 1, n_keys = 1) and its read is its group, so a hit is a pair of rows
of different reads with that hash in common.  A hash equal to UINT64_MAX is the padding of the index's rows: such a minimizer is
an empty row there and seeds nothing.  `seed_pairs` is that join as raw entry pairs; `chain_hits` hands them to kmu_seed_chains
(Context.seed_chains): one colinear chain of seeds per read pair, at base resolution; `read_chains` goes from reads to chains.
With all=True both hand them to kmu_seed_chains_all instead: every chain of every read pair; `rank_chains` (kmu_chain_rank) then says
which chains of a query read are primary, `chain_mapq` turns that into mapping qualities on the host, `map_reads` goes from reads
and contigs to (chains, rank), and `paf_lines(..., rank=rank)` writes the qualities and the tp / s2 tags.
`align_chains` hands the chains and the reads to kmu_chain_align (Context.chain_align): the banded edit distance and the matching
columns of every chain's two segments; `read_alignments` goes from reads to (chains, alignments), and `paf_lines` writes the two
record arrays as PAF text on the host.  `cigar_chains` hands the same to kmu_chain_cigar (Context.chain_cigar): the records and the
path of every alignment as CIGAR runs; `read_cigars` goes from reads to (chains, aln, ops, op_offsets), `cigar_strings` writes the
runs as text, and `paf_lines(..., cigar=(ops, op_offsets))` appends them as the cg:Z: tag.  `pileup_chains` hands the chains, their
records and their runs to kmu_chain_pileup (Context.chain_pileup): for every base of every read, how many partners were aligned
over it and what they had there; `read_pileups` goes from reads to (chains, aln, pile, call, reads) -- the self-join pileup and the
calls of kmu_pile_call -- without the runs leaving where the reads live, and `pile_depth` is the depth column of a table.
`insertions_chains` hands the same chains and runs, with the slots Context.pile_ins_plan gave every base, to kmu_chain_pile_ins
(Context.chain_pile_ins): which letters the partners have where most of them have extra bases; `consensus_reads` turns table,
calls and slots into the corrected reads (kmu_pile_consensus), a new batch of bases and offsets; `correct_reads` goes from reads
to (cons_bases, cons_offsets, reads) in one call, and what it returns goes straight back into `read_minimizers` or the counter.
`classify_chains` and `overlap_graph` hand the chains and their records to kmu_sg_classify / kmu_sg_graph (Context.sg_classify,
Context.sg_graph): the class of every overlap, the contained reads and the transitively reduced string graph; `read_graph` goes
from reads to the graph, `unitig_labels` groups the reads of one unitig and `gfa_lines` writes the graph as GFA text on the host.
`unitig_paths` and `unitig_sequences` hand the arcs to kmu_sg_unitigs / kmu_sg_unitig_seqs (Context.sg_unitigs,
Context.sg_unitig_seqs): the reads of every unitig in walk order with their coordinates, and the unitig's bases; `read_unitigs`
goes from reads to unitig sequences, and `unitig_gfa_lines` writes them as GFA `S` and `a` lines on the host.
`clean_graph` hands the arcs to kmu_sg_clean (Context.sg_clean) before the layout: short dead ends are removed and simple bubbles
popped, round after round while something goes; `layout_reads` marks the removed reads for `unitig_paths`, and `read_graph` and
`read_unitigs` do both when given max_tip_reads or max_bubble_reads.
`unitig_read_chains` hands the layout and the self-join's containment records to kmu_sg_unitig_chains (Context.sg_unitig_chains):
one chain record per read saying where it lies on which unitig; `polish_unitigs` runs cigar_chains, pileup_chains, pile_call,
pile_ins_plan, insertions_chains and consensus_reads on those records with the unitig batch as the q side -- the consensus of every
unitig over its reads --, `polished_unitigs` gives the unitig records their new lengths, and `read_contigs` goes from reads to
polished unitigs.
"""
import collections
import math

import numpy as np

from . import _abi as A

# the minimizers of a batch (Context.read_minimizers): entries offsets[i] .. offsets[i + 1] belong to read i, ascending in
# position; hashes / pos / read / strand are numpy arrays or torch cuda tensors; k, w, fhash say how they were chosen
Minimizers = collections.namedtuple("Minimizers", "hashes pos read strand offsets k w fhash")


def read_minimizers(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, kmer_type=None):
    """The (w, k) minimizers of every read of a batch as a Minimizers record; the k-mer type defaults to the reference's choice
    for k.  The ntHash orders have no strand: the record's strand is then None."""
    if kmer_type is None:
        kmer_type = A.kmer_type_for_k(k)
    nthash = fhash in (A.FHASH_CANON_NTHASH, A.FHASH_CANON_NTHASH_8B)
    want = ("pos", "read") if nthash else ("pos", "read", "strand")
    hashes, pos, read, strand, moff = ctx.read_minimizers(bases, offsets, kmer_type, k, fhash, w, want=want)
    return Minimizers(hashes, pos, read, strand, moff, int(k), int(w), int(fhash))


# the syncmers of a batch (Context.read_syncmers): the arrays of a Minimizers record; k, s, t, fhash say how they were chosen.
# seed_pairs, seed_hits and chain_hits take either record: they read hashes, pos, read, strand, offsets and k only.
Syncmers = collections.namedtuple("Syncmers", "hashes pos read strand offsets k s t fhash")


def read_syncmers(ctx, bases, offsets, k, s, t=0, fhash=A.FHASH_CANON_INVHASH, s_fhash=None, kmer_type=None, s_kmer_type=None):
    """The (k, s, t) syncmers of every read of a batch as a Syncmers record: the k-mers whose smallest s-mer sits at offset t or
    k - s - t (t = 0: closed, 2 t == k - s: open).  The order of the s-mers defaults to `fhash`, the k-mer types to the reference's
    choices for k and for s.  The ntHash orders have no strand: the record's strand is then None."""
    if kmer_type is None:
        kmer_type = A.kmer_type_for_k(k)
    if s_kmer_type is None:
        s_kmer_type = A.kmer_type_for_k(s)
    if s_fhash is None:
        s_fhash = fhash
    nthash = fhash in (A.FHASH_CANON_NTHASH, A.FHASH_CANON_NTHASH_8B)
    want = ("pos", "read") if nthash else ("pos", "read", "strand")
    hashes, pos, read, strand, soff = ctx.read_syncmers(bases, offsets, kmer_type, k, fhash, s, t, s_kmer_type, s_fhash, want=want)
    return Syncmers(hashes, pos, read, strand, soff, int(k), int(s), int(t), int(fhash))


def _seeds(ctx, bases, offsets, k, w, fhash, syncmer):
    """the seeds of read_chains and map_reads: window minimizers, or syncmers when a pair (s, t) is given"""
    if syncmer is None:
        return read_minimizers(ctx, bases, offsets, k, w, fhash)
    s, t = syncmer
    return read_syncmers(ctx, bases, offsets, k, s, t, fhash)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _gather6(pairs, q, db):
    """(read_a, pos_a, strand_a, read_b, pos_b, strand_b) of the row pairs, int64, where the arrays live"""
    cols = []
    if _is_torch(pairs):
        import torch
        idx = pairs.long() & 0xFFFFFFFF
        for side, m in ((0, q), (1, db)):
            i = idx[:, side]
            for x in (m.read, m.pos, m.strand):
                cols.append(torch.zeros_like(i) if x is None else x[i].long() & 0xFFFFFFFF)
        return torch.stack(cols, dim=1) if cols[0].numel() else torch.zeros((0, 6), dtype=torch.int64, device=pairs.device)
    idx = np.asarray(pairs).astype(np.int64)
    for side, m in ((0, q), (1, db)):
        i = idx[:, side]
        for x in (m.read, m.pos, m.strand):
            cols.append(np.zeros(i.shape, np.int64) if x is None else np.asarray(x)[i].astype(np.int64))
    return np.stack(cols, axis=1) if idx.shape[0] else np.zeros((0, 6), np.int64)


def seed_pairs(ctx, q, db=None, max_occ=0):
    """The index join behind seed_hits and chain_hits: the raw pairs (entry of q, entry of db) of minimizers that share a hash,
    uint32 [n, 2] (int32 holding the same bits for torch), ordered by the entry of q, then the entry of db.  db=None is the
    self-join (a minimizer never pairs with one of its own read); max_occ as in seed_hits."""
    own = db is None
    if own:
        db = q
    rows_q, rows_db = q.hashes.reshape(-1, 1), db.hashes.reshape(-1, 1)
    with ctx.anchor_index(rows_db, n_keys=1, group_db=db.read if own else None) as index:
        pairs, _ = index.match(rows_q, group_q=q.read if own else None, min_common=1, max_occ=int(max_occ))
    return pairs


def seed_hits(ctx, q, db=None, max_occ=0):
    """Minimizers of different reads that share a hash.  q, db: Minimizers records (numpy, or torch on the device -- the join
    then runs on the resident arrays and the hits stay there).  db=None is the self-join of a batch: a minimizer never hits one
    of its own read, and (a, b) and (b, a) are both there.  With a db of its own every equal hash is a hit (the two batches
    number their reads independently).  max_occ > 0: a hash that more than max_occ minimizers of db carry seeds nothing (the
    repeat mask of the anchor index).  Returns an int64 array [n, 6] of records (read_a, pos_a, strand_a, read_b, pos_b,
    strand_b), a of q and b of db, ordered by the entry of q, then the entry of db; a record's strands are 0 where the minimizers
    were made without.  A hash equal to UINT64_MAX seeds nothing: it is the padding of the index's rows."""
    return _gather6(seed_pairs(ctx, q, db, max_occ), q, q if db is None else db)


def chain_hits(ctx, q, db=None, max_occ=0, max_gap=5000, band=500, min_seeds=3, min_score=0, upper=None, all=False):
    """From minimizers to one chain per read pair (kmu_seed_chains on the pairs of seed_pairs): which reads overlap, on which
    strand, from where to where on both reads in bases, with how many seeds and which score.  q, db: Minimizers records of
    read_minimizers (their offsets say how many reads there are, q.k is the span of a seed); db=None is the self-join, and
    `upper` then defaults to True: each read pair once, read_a < read_b.  max_gap / band / min_seeds / min_score: the chaining
    rules of include/kmu.h.  all=True: every chain of every read pair and strand (kmu_seed_chains_all), which is what mapping
    reads onto contigs or a reference needs; the string graph keeps taking the one-per-pair records.  Returns a structured array
    of A.CHAIN_DTYPE for numpy records; for torch records an int32 tensor [n, 10] holding the same bits, on the device, where the
    hits never left it."""
    if upper is None:
        upper = db is None
    pairs = seed_pairs(ctx, q, db, max_occ)
    chain = ctx.seed_chains_all if all else ctx.seed_chains
    return chain(pairs, q, db, span=q.k, max_gap=max_gap, band=band, min_seeds=min_seeds, min_score=min_score, upper=upper)


def read_chains(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band=500, min_seeds=3, min_score=0,
                all=False, syncmer=None):
    """From the reads of a batch to the chains between them in one call: read_minimizers, then the self-join of chain_hits.
    syncmer=(s, t) seeds with read_syncmers(k, s, t) instead; w is then unused."""
    q = _seeds(ctx, bases, offsets, k, w, fhash, syncmer)
    return chain_hits(ctx, q, None, max_occ, max_gap, band, min_seeds, min_score, all=all)


def rank_chains(ctx, chains, n_reads_q, mask_permille=500):
    """Primary and secondary chains of every query read (kmu_chain_rank, Context.chain_rank): rank, parent, sub_score and n_sub
    per chain, aligned with `chains` (include/kmu.h has the rules).  numpy records give a structured array of A.CHAIN_RANK_DTYPE;
    torch records an int32 tensor [n, 4] holding the same bits, on the device."""
    return ctx.chain_rank(chains, n_reads_q, mask_permille=mask_permille)


def chain_mapq(chains, rank):
    """The mapping quality of every chain, on the host, from numpy records of A.CHAIN_DTYPE and A.CHAIN_RANK_DTYPE: for a primary
    min(60, floor(40 * (1 - sub_score / score) * min(1, n_seeds / 10) * ln(score))), the formula of the minimap2 paper, in
    doubles; 0 for a secondary and for a score of 0.  Returns an int64 array."""
    chains, rank = np.asarray(chains), np.asarray(rank)
    out = np.zeros(chains.shape[0], np.int64)
    for c, (score, n_seeds, sub, parent) in enumerate(zip(chains["score"].tolist(), chains["n_seeds"].tolist(),
                                                          rank["sub_score"].tolist(), rank["parent"].tolist())):
        if parent == c and score > 0:
            out[c] = min(60, int(math.floor(40.0 * (1.0 - sub / score) * min(1.0, n_seeds / 10.0) * math.log(score))))
    return out


def map_reads(ctx, bases_q, offsets_q, bases_db, offsets_db, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band=500,
              min_seeds=3, min_score=0, mask_permille=500, syncmer=None):
    """From a batch of reads and a batch of contigs (or a reference) to every chain of every read on them and which of them to
    believe: read_minimizers of both, chain_hits(all=True), rank_chains.  Returns (chains, rank).  syncmer=(s, t) seeds both
    batches with read_syncmers(k, s, t) instead; w is then unused."""
    q = _seeds(ctx, bases_q, offsets_q, k, w, fhash, syncmer)
    db = _seeds(ctx, bases_db, offsets_db, k, w, fhash, syncmer)
    chains = chain_hits(ctx, q, db, max_occ, max_gap, band, min_seeds, min_score, all=True)
    return chains, rank_chains(ctx, chains, len(q.offsets) - 1, mask_permille)


def align_chains(ctx, chains, bases_q, offsets_q, bases_db=None, offsets_db=None, band=64):
    """The alignment record of every chain (kmu_chain_align): edit, matches, n_diags and the flags A.ALN_DONE / A.ALN_EXACT of the
    banded global alignment of the two segments the chain names (include/kmu.h has the rules).  chains: the records of chain_hits;
    bases_* / offsets_*: the reads the minimizers were taken of (db=None: the self-join).  numpy records give a structured array
    of A.CHAIN_ALN_DTYPE; torch records an int32 tensor [n, 4] holding the same bits, on the device."""
    return ctx.chain_align(chains, bases_q, offsets_q, bases_db, offsets_db, band=band)


def read_alignments(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band_chain=500, min_seeds=3,
                    min_score=0, band=64):
    """From the reads of a batch to the chains between them and their alignments in one call: read_chains (band_chain is its
    band), then align_chains with `band`.  Returns (chains, aln)."""
    chains = read_chains(ctx, bases, offsets, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score)
    return chains, align_chains(ctx, chains, bases, offsets, band=band)


def cigar_chains(ctx, chains, bases_q, offsets_q, bases_db=None, offsets_db=None, band=64, max_trace_bytes=0, aln=None):
    """The alignment record and the alignment path of every chain (kmu_chain_cigar): (aln, ops, op_offsets) as Context.chain_cigar
    returns them -- the records of align_chains with A.ALN_PATH where a chain's runs were written, the runs len << 4 | code of
    chain c in ops[op_offsets[c]:op_offsets[c + 1]].  Arguments as align_chains; max_trace_bytes and aln as Context.chain_cigar."""
    return ctx.chain_cigar(chains, bases_q, offsets_q, bases_db, offsets_db, band=band, max_trace_bytes=max_trace_bytes, aln=aln)


def read_cigars(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band_chain=500, min_seeds=3,
                min_score=0, band=64, max_trace_bytes=0):
    """From the reads of a batch to the chains between them, their alignments and the alignments' paths in one call: read_chains
    (band_chain is its band), then cigar_chains with `band`.  Returns (chains, aln, ops, op_offsets)."""
    chains = read_chains(ctx, bases, offsets, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score)
    return (chains,) + tuple(cigar_chains(ctx, chains, bases, offsets, band=band, max_trace_bytes=max_trace_bytes))


def pileup_chains(ctx, chains, aln, ops, op_offsets, bases_q, offsets_q, bases_db=None, offsets_db=None, sides=A.PILE_Q | A.PILE_DB,
                  into=None):
    """The votes of every chain's runs onto the bases of both reads (kmu_chain_pileup): (pile_q, pile_db) as Context.chain_pileup
    returns them -- uint32 [n_bases, A.PILE_COLS], one row per base, columns A.PILE_A .. A.PILE_ENDS; one shared table in the
    self-join (db=None).  chains, aln, ops, op_offsets: the chains and what cigar_chains gave for them; sides and into as
    Context.chain_pileup."""
    return ctx.chain_pileup(chains, aln, ops, op_offsets, bases_q, offsets_q, bases_db, offsets_db, sides=sides, into=into)


def read_pileups(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band_chain=500, min_seeds=3,
                 min_score=0, band=64, max_trace_bytes=0, min_depth=3):
    """From the reads of a batch to the pileup of every read and its calls in one call: read_cigars, then the self-join of
    pileup_chains (every read collects the votes of all its partners in one table), then Context.pile_call with `min_depth`.
    Returns (chains, aln, pile, call, reads)."""
    chains, aln, ops, op_offsets = read_cigars(ctx, bases, offsets, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, band,
                                               max_trace_bytes)
    pile, _ = pileup_chains(ctx, chains, aln, ops, op_offsets, bases, offsets)
    call, reads = ctx.pile_call(pile, bases, offsets, min_depth=min_depth)
    return chains, aln, pile, call, reads


def insertions_chains(ctx, chains, aln, ops, op_offsets, bases_q, offsets_q, ins_len_q, n_slots_q, bases_db=None, offsets_db=None,
                      ins_len_db=None, n_slots_db=None, sides=A.PILE_Q | A.PILE_DB, into=None):
    """The letters of every chain's gap runs, voted into the insertion slots of both reads (kmu_chain_pile_ins): (ins_q, ins_db) as
    Context.chain_pile_ins returns them -- uint32 [n_slots, A.INS_COLS], one count per letter of every slot; one shared table in
    the self-join (db=None).  chains, aln, ops, op_offsets: as pileup_chains takes them; ins_len_* / n_slots_*: the plan of
    Context.pile_ins_plan for each batch; sides and into as Context.chain_pile_ins."""
    return ctx.chain_pile_ins(chains, aln, ops, op_offsets, bases_q, offsets_q, ins_len_q, n_slots_q, bases_db, offsets_db, ins_len_db,
                              n_slots_db, sides=sides, into=into)


def consensus_reads(ctx, pile, call, ins_len, n_slots, ins, bases, offsets):
    """The corrected reads of a batch (kmu_pile_consensus): (cons_bases, cons_offsets), a new ASCII batch -- per base the called
    letter, the read's own byte where there is no call, nothing for a DEL call, and behind it the emitted insertion slots."""
    return ctx.pile_consensus(pile, call, ins_len, n_slots, ins, bases, offsets)


def correct_reads(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band_chain=500, min_seeds=3,
                  min_score=0, band=64, max_trace_bytes=0, min_depth=3, max_ins=16):
    """From the reads of a batch to their corrected versions in one call: read_cigars, the self-join of pileup_chains,
    Context.pile_call with `min_depth`, Context.pile_ins_plan with `max_ins`, the self-join of insertions_chains, consensus_reads.
    Returns (cons_bases, cons_offsets, reads), reads being the summaries of pile_call.  Runs, tables and slots stay where the
    reads live."""
    chains, aln, ops, op_offsets = read_cigars(ctx, bases, offsets, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, band,
                                               max_trace_bytes)
    pile, _ = pileup_chains(ctx, chains, aln, ops, op_offsets, bases, offsets)
    call, reads = ctx.pile_call(pile, bases, offsets, min_depth=min_depth)
    ins_len, n_slots = ctx.pile_ins_plan(pile, call, max_ins=max_ins)
    ins, _ = insertions_chains(ctx, chains, aln, ops, op_offsets, bases, offsets, ins_len, n_slots)
    cons_bases, cons_offsets = consensus_reads(ctx, pile, call, ins_len, n_slots, ins, bases, offsets)
    return cons_bases, cons_offsets, reads


def _segment_rows(segs, offsets):
    """(first row, end row) of every segment in its batch: offsets[read] + start / end, where the segments live (int64 for torch,
    uint64 for numpy)"""
    if _is_torch(segs):
        off = offsets.long() if _is_torch(offsets) else None
        if off is None or off.device != segs.device:
            import torch
            off = torch.from_numpy(np.asarray(offsets.cpu() if _is_torch(offsets) else offsets).astype(np.int64)).to(segs.device)
        s = segs.long() & 0xFFFFFFFF
        beg = off[s[:, 0]]
        return (beg + s[:, 1]).contiguous(), (beg + s[:, 2]).contiguous()
    beg = np.asarray(offsets).astype(np.uint64)[segs["read"]]
    return beg + segs["start"].astype(np.uint64), beg + segs["end"].astype(np.uint64)


def trim_reads(ctx, pile, bases, offsets, min_depth=3, min_span=None, min_len=100, longest=False):
    """The reads of a batch cut down to their supported segments (kmu_pile_segments, kmu_extract_ranges): every kept segment -- rows
    with depth >= min_depth, consecutive rows linked by a spanning depth >= min_span (None: min_depth), at least min_len long --
    becomes a read of the new batch, so uncovered ends go, and a chimera comes out as its parts.  longest=True keeps one segment
    per read.  Returns (trim_bases, trim_offsets, segs, reads): the new ASCII batch, the segments its reads are (Context.pile_segments)
    and the summary of every input read.  The ranges are computed where the table lives."""
    segs, _, reads = ctx.pile_segments(pile, offsets, min_depth=min_depth, min_span=min_span, min_len=min_len, longest=longest)
    begin, end = _segment_rows(segs, offsets)
    trim_bases, trim_offsets = ctx.extract_ranges(bases, begin, end)
    return trim_bases, trim_offsets, segs, reads


def correct_trim_reads(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band_chain=500, min_seeds=3,
                       min_score=0, band=64, max_trace_bytes=0, min_depth=3, max_ins=16, min_span=None, min_len=100, longest=False):
    """correct_reads and trim_reads in one call, on one table: read_cigars, the self-join of pileup_chains, Context.pile_call,
    Context.pile_ins_plan, the self-join of insertions_chains and consensus_reads as correct_reads does them; then
    Context.pile_segments on the same table, Context.pile_consensus_pos of every segment's first row and end row, and
    Context.extract_ranges on the consensus batch.  Returns (out_bases, out_offsets, segs, reads, trims): the corrected, trimmed
    and split reads, the segments (in raw read coordinates) they are, the summaries of pile_call and those of pile_segments.
    Tables and runs stay where the reads live."""
    chains, aln, ops, op_offsets = read_cigars(ctx, bases, offsets, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, band,
                                               max_trace_bytes)
    pile, _ = pileup_chains(ctx, chains, aln, ops, op_offsets, bases, offsets)
    call, reads = ctx.pile_call(pile, bases, offsets, min_depth=min_depth)
    ins_len, n_slots = ctx.pile_ins_plan(pile, call, max_ins=max_ins)
    ins, _ = insertions_chains(ctx, chains, aln, ops, op_offsets, bases, offsets, ins_len, n_slots)
    cons_bases, _ = consensus_reads(ctx, pile, call, ins_len, n_slots, ins, bases, offsets)
    segs, _, trims = ctx.pile_segments(pile, offsets, min_depth=min_depth, min_span=min_span, min_len=min_len, longest=longest)
    first, last = _segment_rows(segs, offsets)
    n = int(first.shape[0])
    if _is_torch(first):
        import torch
        rows = torch.cat([first, last])
    else:
        rows = np.concatenate([first, last])
    pos = ctx.pile_consensus_pos(pile, call, ins_len, n_slots, ins, bases, offsets, rows)
    out_bases, out_offsets = ctx.extract_ranges(cons_bases, pos[:n].contiguous() if _is_torch(pos) else pos[:n],
                                                pos[n:].contiguous() if _is_torch(pos) else pos[n:])
    return out_bases, out_offsets, segs, reads, trims


def classify_chains(ctx, chains, aln, offsets, min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=0, fuzz=10):
    """The class of every chain record of a self-join and the contained reads (kmu_sg_classify): (classes, reads) as
    Context.sg_classify returns them.  chains, aln: the records of read_alignments (aln=None: no identity test); offsets: the
    batch's.  The thresholds are those of include/kmu.h: an overlap is at least min_overlap long on both reads; it is internal when
    its overhang is above max_hang or above int_permille thousandths of its length."""
    return ctx.sg_classify(chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz)


def overlap_graph(ctx, chains, aln, offsets, min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=0, fuzz=10):
    """The string graph of a self-join (kmu_sg_graph): (arcs, arc_offsets, classes, reads) as Context.sg_graph returns them -- the
    dovetails between reads that are not contained as a bidirected graph (vertex 2r: read r forward, 2r + 1: reverse complement),
    transitively reduced with `fuzz`."""
    return ctx.sg_graph(chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz)


def clean_graph(ctx, arcs, reads, n_reads, max_tip_reads=4, max_bubble_reads=8, rounds=1):
    """Tips removed and simple bubbles popped (kmu_sg_clean): (arcs, reads, stats) as Context.sg_clean returns them.  The call is
    repeated on its own output while a round removed something, at most `rounds` times; the stats are summed over the rounds, except
    n_arcs_left, which is the last round's.  rounds=0 returns the inputs as they are, with zero stats."""
    total = dict.fromkeys(A.SG_CLEAN_STATS, 0)
    for _ in range(int(rounds)):
        arcs, reads, stats = ctx.sg_clean(arcs, reads, n_reads, max_tip_reads, max_bubble_reads)
        for name in A.SG_CLEAN_STATS:
            total[name] = stats[name] if name == "n_arcs_left" else total[name] + stats[name]
        if not stats["n_tip_reads"] and not stats["n_bubble_reads"]:
            break
    return arcs, reads, total


def layout_reads(reads):
    """A copy of the summaries in which every read that carries A.SG_READ_TIP or A.SG_READ_BUBBLE also carries
    A.SG_READ_CONTAINED: unitig_paths then leaves the removed reads off the layout (numpy records, or the int32 [n_reads, 4] tensor)."""
    removed = A.SG_READ_TIP | A.SG_READ_BUBBLE
    if _is_torch(reads):
        out = reads.clone()
        out[:, 0] |= ((out[:, 0] & removed) != 0).to(out.dtype) * A.SG_READ_CONTAINED
        return out
    out = np.array(reads, copy=True)
    out["flags"] |= ((out["flags"] & removed) != 0).astype(np.uint32) * np.uint32(A.SG_READ_CONTAINED)
    return out


def read_graph(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band_chain=500, min_seeds=3, min_score=0,
               band=64, min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=0, fuzz=10, max_tip_reads=0,
               max_bubble_reads=0, clean_rounds=1):
    """From the reads of a batch to their string graph in one call: read_alignments, then overlap_graph on its records.  Returns
    (arcs, arc_offsets, classes, reads); with torch cuda tensors nothing leaves the device.  With max_tip_reads or max_bubble_reads
    above 0 the arcs and the summaries are those of clean_graph (the arcs keep their places, so arc_offsets still holds)."""
    chains, aln = read_alignments(ctx, bases, offsets, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, band)
    arcs, arc_offsets, classes, reads = overlap_graph(ctx, chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz)
    if max_tip_reads or max_bubble_reads:
        arcs, reads, _ = clean_graph(ctx, arcs, reads, int(reads.shape[0]), max_tip_reads, max_bubble_reads, clean_rounds)
    return arcs, arc_offsets, classes, reads


def unitig_labels(ctx, arcs, n_reads):
    """Which reads lie on one unitig: Context.components over the 2 n_reads vertices with the arcs whose `unique` is 1 as edges
    (stride 8, weight_at 6, min_weight 1), which finds every unitig once per strand; a read's label is the smaller of the labels
    of its two vertices.  arcs: the records of overlap_graph.  Returns uint32 [n_reads] (int32 for torch), where the arcs live."""
    edges = arcs if _is_torch(arcs) else np.ascontiguousarray(arcs).reshape(-1).view(np.uint32).reshape(-1, 8)
    label = ctx.components(edges, 2 * int(n_reads), weight_at=6, min_weight=1, want=(), count=False).label
    if _is_torch(label):
        import torch
        return torch.minimum(label[0::2], label[1::2])
    return np.minimum(label[0::2], label[1::2])


def unitig_paths(ctx, arcs, reads, offsets):
    """The unitigs of a string graph as ordered paths (kmu_sg_unitigs): (unitigs, path, place) as Context.sg_unitigs returns them --
    which reads lie on every unitig, in which order and orientation, and where each ends.  arcs, reads: the records and the
    summaries of overlap_graph (reads=None: no read is contained)."""
    return ctx.sg_unitigs(arcs, reads, offsets)


def unitig_sequences(ctx, unitigs, path, bases, offsets):
    """The bases of every unitig (kmu_sg_unitig_seqs): (seq, seq_offsets) as Context.sg_unitig_seqs returns them.  On error-free
    reads a unitig's sequence is the genome stretch it covers; on corrected reads (correct_reads, then read_graph on the new batch)
    it is a draft contig."""
    return ctx.sg_unitig_seqs(unitigs, path, bases, offsets)


def read_unitigs(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band_chain=500, min_seeds=3, min_score=0,
                 band=64, min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=0, fuzz=10, max_tip_reads=0,
                 max_bubble_reads=0, clean_rounds=1):
    """From the reads of a batch to their unitigs in one call: read_graph, unitig_paths, unitig_sequences.  Returns (unitigs, path,
    place, seq, seq_offsets); with torch cuda tensors nothing leaves the device.  With max_tip_reads or max_bubble_reads above 0
    the graph is cleaned first and the removed reads are on no unitig (layout_reads)."""
    arcs, _, _, reads = read_graph(ctx, bases, offsets, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, band, min_overlap,
                                   max_hang, int_permille, min_identity_permille, fuzz, max_tip_reads, max_bubble_reads, clean_rounds)
    if max_tip_reads or max_bubble_reads:
        reads = layout_reads(reads)
    unitigs, path, place = unitig_paths(ctx, arcs, reads, offsets)
    seq, seq_offsets = unitig_sequences(ctx, unitigs, path, bases, offsets)
    return unitigs, path, place, seq, seq_offsets


def unitig_read_chains(ctx, unitigs, path, place, chains, classes, offsets):
    """Where every read lies on which unitig, as chain records (kmu_sg_unitig_chains): (records, stats) as Context.sg_unitig_chains
    returns them.  unitigs, path, place: of unitig_paths; chains, classes: the self-join and the classes of overlap_graph for it, or
    None for both (then the contained reads stay unplaced); offsets: the batch's.  The records name the unitig batch of
    unitig_sequences as their q side and the reads as their db side: they go into cigar_chains and what follows it."""
    return ctx.sg_unitig_chains(unitigs, path, place, chains, classes, offsets)


def _polished_coordinates(ctx, tables, seq, seq_offsets, cons_offsets, path, place, records):
    """(ends, a_start, a_end) in the polished batch: every step's end and every map record's a coordinates through
    Context.pile_consensus_pos, as correct_trim_reads translates its segment ends; int64, where the arrays live.  A step's unitig is
    that of its read's place."""
    pile, call, ins_len, n_slots, ins = tables
    if _is_torch(path):
        import torch
        m32 = 0xFFFFFFFF
        off, cons = seq_offsets.long(), cons_offsets.long()
        u_step = place[:, 0].long()[path[:, 0].long() & m32] & m32
        u_rec = records[:, 0].long() & m32
        ends = (path[:, 2].long() & m32) | (path[:, 3].long() << 32)
        rows = torch.cat([off[u_step] + ends, off[u_rec] + (records[:, 6].long() & m32), off[u_rec] + (records[:, 7].long() & m32)]).contiguous()
        base = torch.cat([cons[u_step], cons[u_rec], cons[u_rec]])
        pos = ctx.pile_consensus_pos(pile, call, ins_len, n_slots, ins, seq, seq_offsets, rows).long() - base
    else:
        off, cons = np.asarray(seq_offsets).astype(np.int64), np.asarray(cons_offsets).astype(np.int64)
        u_step = place["unitig"][path["read"]].astype(np.int64)
        u_rec = records["read_a"].astype(np.int64)
        rows = np.concatenate([off[u_step] + path["end"].astype(np.int64), off[u_rec] + records["a_start"], off[u_rec] + records["a_end"]])
        pos = ctx.pile_consensus_pos(pile, call, ins_len, n_slots, ins, seq, seq_offsets, rows).astype(np.int64) - np.concatenate(
            [cons[u_step], cons[u_rec], cons[u_rec]])
    n, m = int(path.shape[0]), int(records.shape[0])
    return pos[:n], pos[n:n + m], pos[n + m:]


def polish_unitigs(ctx, unitigs, path, place, seq, seq_offsets, bases, offsets, chains=None, classes=None, band=64, max_trace_bytes=0,
                   min_depth=2, max_ins=16, rounds=1):
    """The consensus of every unitig over its reads: unitig_read_chains, then -- with the unitig batch (seq, seq_offsets) of
    unitig_sequences as the q side and the reads as the db side -- cigar_chains, pileup_chains and insertions_chains with
    sides=A.PILE_Q, Context.pile_call with `min_depth`, Context.pile_ins_plan with `max_ins` and consensus_reads.  chains, classes: the
    self-join and its classes, through which the contained reads vote too.  Returns (cons_seq, cons_offsets, new_path, summaries,
    map_records, aln): the polished batch; `path` with every end in polished coordinates (Context.pile_consensus_pos), so that
    unitig_gfa_lines(polished_unitigs(unitigs, cons_offsets), new_path, cons_seq, cons_offsets, names) holds; the summaries of
    pile_call; the map's records and their alignment records.  rounds > 1 translates the records' a coordinates the same way and
    runs the stages again on the polished batch; then map_records and aln are those of the last round.  With torch cuda tensors
    nothing leaves the device."""
    records, _ = unitig_read_chains(ctx, unitigs, path, place, chains, classes, offsets)
    summaries = aln = None
    for _ in range(max(int(rounds), 1)):
        aln, ops, op_offsets = cigar_chains(ctx, records, seq, seq_offsets, bases, offsets, band=band, max_trace_bytes=max_trace_bytes)
        pile, _ = pileup_chains(ctx, records, aln, ops, op_offsets, seq, seq_offsets, bases, offsets, sides=A.PILE_Q)
        call, summaries = ctx.pile_call(pile, seq, seq_offsets, min_depth=min_depth)
        ins_len, n_slots = ctx.pile_ins_plan(pile, call, max_ins=max_ins)
        ins, _ = insertions_chains(ctx, records, aln, ops, op_offsets, seq, seq_offsets, ins_len, n_slots, bases, offsets, sides=A.PILE_Q)
        cons_seq, cons_offsets = consensus_reads(ctx, pile, call, ins_len, n_slots, ins, seq, seq_offsets)
        ends, a_start, a_end = _polished_coordinates(ctx, (pile, call, ins_len, n_slots, ins), seq, seq_offsets, cons_offsets, path, place,
                                                     records)
        used = records
        if _is_torch(path):
            path, records = path.clone(), records.clone()
            path[:, 2:4] = ends.contiguous().view(path.dtype).reshape(-1, 2)
            records[:, 6], records[:, 7] = a_start.to(records.dtype), a_end.to(records.dtype)
        else:
            path, records = np.array(path, copy=True), np.array(records, copy=True)
            path["end"] = ends.astype(np.uint64)
            records["a_start"], records["a_end"] = a_start.astype(np.uint32), a_end.astype(np.uint32)
        seq, seq_offsets = cons_seq, cons_offsets
    return seq, seq_offsets, path, summaries, used, aln


def polished_unitigs(unitigs, cons_offsets):
    """A copy of the unitig records whose len is that of the polished batch (numpy records, or the int32 [n, 8] tensor)"""
    if _is_torch(unitigs):
        out = unitigs.clone()
        length = (cons_offsets[1:] - cons_offsets[:-1]).long().contiguous()
        out[:, 2:4] = length.view(out.dtype).reshape(-1, 2)
        return out
    out = np.array(unitigs, copy=True)
    out["len"] = np.diff(np.asarray(cons_offsets).astype(np.uint64))
    return out


def read_contigs(ctx, bases, offsets, k, w, fhash=A.FHASH_CANON_INVHASH, max_occ=0, max_gap=5000, band_chain=500, min_seeds=3, min_score=0,
                 band=64, min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=0, fuzz=10, max_tip_reads=0,
                 max_bubble_reads=0, clean_rounds=1, min_depth=2, max_ins=16, rounds=1):
    """From the reads of a batch to polished unitigs in one call: the stages of read_unitigs with the same keywords (its outputs are
    the same bytes; the chains and their classes are kept here, since the contained reads vote through them), then polish_unitigs.
    Returns (unitigs, path, place, cons_seq, cons_offsets, summaries): the unitig records with the polished lengths, the steps with
    polished ends, the places, the polished batch and the summaries of pile_call.  With torch cuda tensors nothing leaves the
    device."""
    chains, aln = read_alignments(ctx, bases, offsets, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, band)
    arcs, _, classes, reads = overlap_graph(ctx, chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz)
    if max_tip_reads or max_bubble_reads:
        arcs, reads, _ = clean_graph(ctx, arcs, reads, int(reads.shape[0]), max_tip_reads, max_bubble_reads, clean_rounds)
        reads = layout_reads(reads)
    unitigs, path, place = unitig_paths(ctx, arcs, reads, offsets)
    seq, seq_offsets = unitig_sequences(ctx, unitigs, path, bases, offsets)
    cons_seq, cons_offsets, new_path, summaries, _, _ = polish_unitigs(ctx, unitigs, path, place, seq, seq_offsets, bases, offsets, chains,
                                                                       classes, band, 0, min_depth, max_ins, rounds)
    return polished_unitigs(unitigs, cons_offsets), new_path, place, cons_seq, cons_offsets, summaries


def unitig_gfa_lines(unitigs, path, seq, seq_offsets, names):
    """The unitigs as GFA text, on the host: `S utg%06d{l|c} <seq> LN:i:<len>` for every unitig (l: linear, c: circular), each
    followed by `a <utg> <end - c> <read name> <+|-> <c>` for every step, c being the bytes the step contributes.  unitigs, path:
    numpy A.SG_UNITIG_DTYPE and A.SG_STEP_DTYPE records; seq, seq_offsets: of unitig_sequences, numpy."""
    text = np.asarray(seq).astype(np.uint8).tobytes().decode("latin-1")
    soff = np.asarray(seq_offsets).astype(np.int64)
    steps = np.asarray(path).tolist()
    lines = []
    for u, (first, length, n, flags, _, _) in enumerate(np.asarray(unitigs).tolist()):
        name = "utg%06d%s" % (u, "c" if flags & A.SG_UNITIG_CIRCULAR else "l")
        lines.append("S\t%s\t%s\tLN:i:%d" % (name, text[soff[u]:soff[u + 1]], length))
        before = 0
        for read, strand, end in steps[first:first + n]:
            lines.append("a\t%s\t%d\t%s\t%s\t%d" % (name, before, names[read], "-" if strand else "+", end - before))
            before = end
    return lines


def gfa_lines(arcs, names, offsets, reduced=False, reads=None):
    """The graph as GFA 1 text, on the host: `S name * LN:i:len` for every read (with reads, the summaries of overlap_graph: for
    every read that is not contained), then `L from +/- to +/- <ovl>M` for every surviving arc in the order of the records;
    reduced=True also writes the arcs that carry A.SG_ARC_REDUCED.  What clean_graph removed is never written: neither the reads
    with A.SG_READ_TIP or A.SG_READ_BUBBLE nor the arcs with A.SG_ARC_TIP or A.SG_ARC_BUBBLE.  arcs: numpy A.SG_ARC_DTYPE records."""
    off = np.asarray(offsets).astype(np.int64)
    lines = []
    gone = A.SG_READ_CONTAINED | A.SG_READ_TIP | A.SG_READ_BUBBLE
    for r in range(off.shape[0] - 1):
        if reads is None or not int(reads["flags"][r]) & gone:
            lines.append("S\t%s\t*\tLN:i:%d" % (names[r], off[r + 1] - off[r]))
    for v, t, _, ovl, _, flags, _, _ in np.asarray(arcs).tolist():
        if flags & (A.SG_ARC_TIP | A.SG_ARC_BUBBLE):
            continue
        if reduced or not flags & A.SG_ARC_REDUCED:
            lines.append("L\t%s\t%s\t%s\t%s\t%dM" % (names[v >> 1], "-" if v & 1 else "+", names[t >> 1], "-" if t & 1 else "+", ovl))
    return lines


def pile_depth(pile):
    """A + C + G + T + DEL of every row of a pileup table: how many partners were aligned over the base (int64; numpy or torch)"""
    if _is_torch(pile):
        return (pile[:, :A.PILE_INS].long() & 0xFFFFFFFF).sum(dim=1)
    return np.asarray(pile)[:, :A.PILE_INS].astype(np.int64).sum(axis=1)


_CIGAR_LETTERS = {A.CIGAR_I: "I", A.CIGAR_D: "D", A.CIGAR_EQ: "=", A.CIGAR_X: "X"}


def cigar_strings(ops, op_offsets, chains=None, extended=True):
    """The runs of kmu_chain_cigar as one CIGAR string per chain, on the host (a chain without runs gives ""): ops and op_offsets
    are numpy arrays.  extended=False merges `=` and `X` into `M`.  The runs follow the query A forwards; with `chains` given, the
    runs of a chain on strand 1 are written in reverse order, that is along the forward strand of the target as PAF's cg tag
    wants them."""
    ops, off = np.asarray(ops).astype(np.int64) & 0xFFFFFFFF, np.asarray(op_offsets).astype(np.int64)
    strands = np.zeros(off.shape[0] - 1, np.int64) if chains is None else np.asarray(chains)["strand"]
    out = []
    for c in range(off.shape[0] - 1):
        runs = [(int(v) >> 4, _CIGAR_LETTERS[int(v) & 15]) for v in ops[off[c]:off[c + 1]]]
        if strands[c]:
            runs.reverse()
        if not extended:
            merged = []
            for n, letter in runs:
                letter = "M" if letter in "=X" else letter
                if merged and merged[-1][1] == letter:
                    merged[-1] = (merged[-1][0] + n, letter)
                else:
                    merged.append((n, letter))
            runs = merged
        out.append("".join("%d%s" % r for r in runs))
    return out


def paf_lines(chains, aln, names_q, offsets_q, names_db=None, offsets_db=None, cigar=None, rank=None):
    """One PAF line per chain, on the host: chains (A.CHAIN_DTYPE) and aln (A.CHAIN_ALN_DTYPE) are numpy records of the same
    length, names_* the names of the reads, offsets_* their offsets (db=None: the self-join).  The 12 standard columns -- query
    name, length, start, end, strand, target name, length, start, end, matches, matches + edit, mapq 255 -- then NM:i:edit,
    s1:i:score and cm:i:n_seeds.  A record without A.ALN_DONE writes 0 matches, a block of max(m, n) and no NM tag.
    cigar=(ops, op_offsets), the runs of cigar_chains for the same chains: a record with A.ALN_PATH also gets cg:Z: with its runs
    along the target's forward strand (cigar_strings with `chains`).
    rank, the records of rank_chains for the same chains (A.CHAIN_RANK_DTYPE): column 12 is chain_mapq, and tp:A:P (primary) or
    tp:A:S (secondary) and s2:i:sub_score follow cm:i:; without it the lines are as above."""
    if names_db is None:
        names_db, offsets_db = names_q, offsets_q
    off_q, off_db = np.asarray(offsets_q).astype(np.int64), np.asarray(offsets_db).astype(np.int64)
    lines = []
    if cigar is not None:
        text = cigar_strings(cigar[0], cigar[1], chains)
        for line, a, cg in zip(paf_lines(chains, aln, names_q, offsets_q, names_db, offsets_db, rank=rank), np.asarray(aln).tolist(), text):
            lines.append(line + "\tcg:Z:" + cg if a[3] & A.ALN_PATH else line)
        return lines
    n = np.asarray(chains).shape[0]
    mapq = [255] * n if rank is None else chain_mapq(chains, rank).tolist()
    ranks = [None] * n if rank is None else np.asarray(rank).tolist()
    for i, (c, a) in enumerate(zip(np.asarray(chains).tolist(), np.asarray(aln).tolist())):
        read_a, read_b, strand, score, n_seeds, _, a_start, a_end, b_start, b_end = c
        edit, matches, _, flags = a
        done = bool(flags & A.ALN_DONE)
        cols = [names_q[read_a], int(off_q[read_a + 1] - off_q[read_a]), a_start, a_end, "-" if strand else "+",
                names_db[read_b], int(off_db[read_b + 1] - off_db[read_b]), b_start, b_end,
                matches if done else 0, matches + edit if done else max(a_end - a_start, b_end - b_start), mapq[i]]
        if done:
            cols.append("NM:i:%d" % edit)
        cols += ["s1:i:%d" % score, "cm:i:%d" % n_seeds]
        if ranks[i] is not None:
            cols += ["tp:A:%s" % ("P" if ranks[i][1] == i else "S"), "s2:i:%d" % ranks[i][2]]
        lines.append("\t".join(str(x) for x in cols))
    return lines
