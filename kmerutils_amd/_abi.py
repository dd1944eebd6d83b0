"""ctypes mirror of include/kmu.h (enums + parameter structs).  Shared by the product loader (lib.py) and by
the test-only oracle loader (oracle/oracle.py); holds no compute."""
import ctypes as C

# kmu_status
OK = 0
E_BAD_K, E_BAD_ALPHABET, E_EMPTY_SEQ, E_NON_ACGT, E_OOM, E_HIP, E_BAD_ARG, E_TABLE_FULL, E_UNSUPPORTED, E_NO_DEVICE = (
    -1, -2, -3, -4, -5, -6, -7, -8, -9, -10)
STATUS_NAMES = {0: "KMU_OK", -1: "KMU_E_BAD_K", -2: "KMU_E_BAD_ALPHABET", -3: "KMU_E_EMPTY_SEQ", -4: "KMU_E_NON_ACGT",
                -5: "KMU_E_OOM", -6: "KMU_E_HIP", -7: "KMU_E_BAD_ARG", -8: "KMU_E_TABLE_FULL",
                -9: "KMU_E_UNSUPPORTED", -10: "KMU_E_NO_DEVICE", -11: "KMU_E_RCCL"}
E_RCCL = -11

MEM_HOST, MEM_DEVICE = 0, 1
INPUT_ASCII, INPUT_PACKED2 = 0, 1
KMER32BIT, KMER16B32BIT, KMER64BIT, KMERAA32BIT, KMERAA64BIT = 0, 1, 2, 3, 4
(FHASH_IDENTITY_RAW, FHASH_VALUE_MASKED, FHASH_CANON_RAW, FHASH_CANON_INVHASH, FHASH_INVHASH_RAW, FHASH_CANON_VALUE,
 FHASH_CANON_NTHASH, FHASH_CANON_NTHASH_8B) = range(8)
ALGO_PROB3A, ALGO_SUPER, ALGO_SUPER2, ALGO_BOTTOMK, ALGO_PROB3, ALGO_OPTDENS, ALGO_REVOPTDENS, ALGO_HLL = 0, 1, 2, 3, 4, 5, 6, 7
SIG_U32, SIG_U64, SIG_F32, SIG_F64, SIG_U16 = 0, 1, 2, 3, 4
HASHER_NOHASH, HASHER_FNV1A, HASHER_INT64HASH = 0, 1, 2
MODE_PER_SEQ, MODE_ALL_SEQS = 0, 1
FLAG_RAND08 = 0x1
KNN_MAX_K = 64          # kmu_sig_knn: the longest neighbour list
KNN_NONE = 0xFFFFFFFF   # idx of a list entry that does not exist
ANCHOR_MAX_NBKMER = 256  # kmu_read_anchors: the largest sketch_size (nbkmer)
ANCHOR_TILE_KMERS = 768  # ... and the k-mers of a window it selects from at a time
ANCHOR_SORT_TILE = 1024  # kmu_anchor_match: the index entries one workgroup ranks per radix pass
OVL_MAX_BAND = 8         # kmu_anchor_overlaps: the widest band
OVL_UPPER = 1            # ... and its flag: only read pairs with read_a < read_b
MINIMIZER_MAX_W = 256    # kmu_read_minimizers: the widest window (in k-mers)
MINIMIZER_TILE = 1024    # ... and the windows one workgroup takes at a time
SYNCMER_TILE = 1024      # kmu_read_syncmers: the k-mer positions one wave takes at a time
CHAIN_LOOKBACK = 64      # kmu_seed_chains: the predecessors an anchor looks at
CHAIN_UPPER = 1          # ... and its flag: only read pairs with read_a < read_b
ALIGN_MAX_DIAGS = 1024   # kmu_chain_align: the widest band, in diagonals, one chain may need
ALIGN_CHUNK = 512        # ... the bases of progress between two stagings of its kernel
ALN_DONE, ALN_EXACT = 1, 2  # ... and the flags of its records
ALN_PATH = 4             # kmu_chain_cigar: the chain's runs were written
CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X = 1, 2, 7, 8  # ... the codes of its runs (BAM's), a run being len << 4 | code
CIGAR_MAX_RUN = (1 << 28) - 1                      # ... the longest run one uint32 holds
CIGAR_TRACE_DEFAULT = 8 << 30                      # ... the trace budget of max_trace_bytes = 0
PILE_COLS = 8            # kmu_chain_pileup: uint32 per row of a table, indexed by
PILE_A, PILE_C, PILE_G, PILE_T, PILE_DEL, PILE_INS, PILE_INS_BASES, PILE_ENDS = range(8)
PILE_Q, PILE_DB = 1, 2   # ... and its flags: vote onto the A side, onto the B side
CALL_NONE, CALL_INS, CALL_DIFF = 7, 8, 16  # kmu_pile_call: bits 0..2 of an uncalled base, and the two bits above the code
INS_COLS = 4             # kmu_chain_pile_ins: uint32 per insertion slot, one count per letter A C G T
INS_MAX = 255            # kmu_pile_ins_plan: the most slots a base can get
SEG_LONGEST = 1          # kmu_pile_segments flags: list only the longest kept segment of every read
TRIM_WHOLE, TRIM_ENDS, TRIM_SPLIT, TRIM_NONE = 0, 1, 2, 3   # kmu_read_trim.cls
SG_TILE = 1024           # records one wave of kmu_sg_graph compacts
SG_SKIP, SG_SHORT, SG_LOWID, SG_INTERNAL, SG_A_CONTAINED, SG_B_CONTAINED, SG_DOVETAIL = range(7)   # the class of a chain record
SG_CLASS_NAMES = ("skip", "short", "lowid", "internal", "a_contained", "b_contained", "dovetail")
SG_READ_CONTAINED = 1    # kmu_sg_read.flags
SG_ARC_REDUCED = 1       # kmu_sg_arc.flags
SG_NONE = 0xFFFFFFFF     # kmu_sg_place.unitig of a contained read
SG_UNITIG_CIRCULAR = 1   # kmu_sg_unitig.flags
SG_ARC_TIP, SG_ARC_BUBBLE = 2, 4     # kmu_sg_arc.flags, set by kmu_sg_clean
SG_READ_TIP, SG_READ_BUBBLE = 2, 4   # kmu_sg_read.flags, set by kmu_sg_clean
SG_CLEAN_MAX = 64        # the largest max_tip_reads / max_bubble_reads


def kmer_val_bytes(kmer_type):
    return 8 if kmer_type in (KMER64BIT, KMERAA64BIT) else 4


def kmer_type_for_k(k, aa=False):
    """The reference's choice of k-mer type for a k (kmer32bit.rs:68, kmer16b32bit.rs, kmer64bit.rs, kmeraa.rs)."""
    if aa:
        return KMERAA32BIT if k <= 6 else KMERAA64BIT
    if k <= 14:
        return KMER32BIT
    if k == 16:
        return KMER16B32BIT
    return KMER64BIT


class DeviceCfg(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("async_device", C.c_int32), ("stream", C.c_void_p),
                ("workspace_bytes", C.c_uint64)]


class SketchParams(C.Structure):
    _fields_ = [("algo", C.c_int32), ("kmer_type", C.c_int32), ("kmer_size", C.c_int32), ("sketch_size", C.c_int32),
                ("sig_type", C.c_int32), ("hasher", C.c_int32), ("fhash", C.c_int32), ("block_size", C.c_int32),
                ("mode", C.c_int32), ("input_kind", C.c_int32), ("mem", C.c_int32), ("flags", C.c_uint32)]


class HashParams(C.Structure):
    _fields_ = [("kmer_type", C.c_int32), ("kmer_size", C.c_int32), ("fhash", C.c_int32), ("input_kind", C.c_int32),
                ("mem", C.c_int32), ("flags", C.c_uint32)]


class CountParams(C.Structure):
    _fields_ = [("kmer_type", C.c_int32), ("kmer_size", C.c_int32), ("counter_bits", C.c_int32),
                ("flags", C.c_int32), ("capacity_hint", C.c_uint64)]


COUNT_DISTRIBUTED = 0x1
COUNT_OWNER_HASH = 0x2
COUNT_HINT_OCCURRENCES = 0x4
OWNER_HASH, OWNER_MINIMIZER = 0, 1
ROUTE_NONE, ROUTE_OCCURRENCES, ROUTE_MERGE, ROUTE_SUPERKMERS = 0, 1, 2, 3
SMER_REC_BYTES = 12
COMM_ID_BYTES = 128


class CommId(C.Structure):
    _fields_ = [("bytes", C.c_char * COMM_ID_BYTES)]


class CommStats(C.Structure):
    """kmu_comm_stats"""
    _fields_ = [("route", C.c_int32), ("sample_shift", C.c_int32), ("dup_ratio", C.c_double), ("kmers_local", C.c_uint64),
                ("bytes_occurrences", C.c_uint64), ("bytes_merge", C.c_uint64), ("bytes_sent", C.c_uint64),
                ("bytes_received", C.c_uint64), ("model_ms_occurrences", C.c_double), ("model_ms_merge", C.c_double),
                ("owner_kind", C.c_int32), ("exchanges", C.c_int32), ("records_local", C.c_uint64),
                ("exchange_ms", C.c_double), ("exchange_gbps_out", C.c_double), ("exchange_gbps_in", C.c_double)]


class CountTableInfo(C.Structure):
    """kmu_count_table_info_t"""
    _fields_ = [("nslots", C.c_uint64), ("table_bytes", C.c_uint64), ("bytes_per_slot", C.c_uint32),
                ("count_field_bits", C.c_uint32), ("count_ceiling", C.c_uint64)]


class ReadAbundance(C.Structure):
    """kmu_read_abundance: one read's k-mers against a counter (kmu_count_read_profile)"""
    _fields_ = [("n_kmers", C.c_uint32), ("n_absent", C.c_uint32), ("n_once", C.c_uint32), ("n_solid", C.c_uint32),
                ("min", C.c_uint16), ("median", C.c_uint16), ("max", C.c_uint16), ("reserved", C.c_uint16), ("sum", C.c_uint64)]


# the same record as a numpy dtype (np.dtype(READ_ABUNDANCE_DTYPE): 32 bytes, the field offsets of the structure)
READ_ABUNDANCE_DTYPE = [("n_kmers", "<u4"), ("n_absent", "<u4"), ("n_once", "<u4"), ("n_solid", "<u4"), ("min", "<u2"),
                        ("median", "<u2"), ("max", "<u2"), ("reserved", "<u2"), ("sum", "<u8")]


KFILTER_MAX_HASHES = 8            # kmu_kfilter: the most bits a key sets in its cell
KFILTER_MAX_CELLS = (1 << 32) - 1  # ... and the most 16-byte cells of a filter


class KFilterParams(C.Structure):
    """kmu_kfilter_params"""
    _fields_ = [("kmer_type", C.c_int32), ("kmer_size", C.c_int32), ("n_hashes", C.c_uint32), ("flags", C.c_uint32),
                ("n_cells", C.c_uint64)]


class KFilterInfo(C.Structure):
    """kmu_kfilter_info_t"""
    _fields_ = [("n_cells", C.c_uint64), ("bytes", C.c_uint64), ("n_hashes", C.c_uint32), ("kmer_size", C.c_uint32),
                ("n_added", C.c_uint64), ("bits_a", C.c_uint64), ("bits_b", C.c_uint64), ("est_distinct", C.c_double)]


# the same record as a numpy dtype (56 bytes, the field offsets of the structure)
KFILTER_INFO_DTYPE = [("n_cells", "<u8"), ("bytes", "<u8"), ("n_hashes", "<u4"), ("kmer_size", "<u4"), ("n_added", "<u8"),
                      ("bits_a", "<u8"), ("bits_b", "<u8"), ("est_distinct", "<f8")]


class Overlap(C.Structure):
    """kmu_overlap: one read pair of kmu_anchor_overlaps"""
    _fields_ = [("read_a", C.c_uint32), ("read_b", C.c_uint32), ("strand", C.c_uint32), ("diag", C.c_int32),
                ("score", C.c_uint32), ("votes", C.c_uint32), ("slice_a_min", C.c_uint32), ("slice_a_max", C.c_uint32)]


# the same record as a numpy dtype (32 bytes)
OVERLAP_DTYPE = [("read_a", "<u4"), ("read_b", "<u4"), ("strand", "<u4"), ("diag", "<i4"), ("score", "<u4"), ("votes", "<u4"),
                 ("slice_a_min", "<u4"), ("slice_a_max", "<u4")]


class SyncmerParams(C.Structure):
    """kmu_syncmer_params: the s-mers that order (type, s, fhash) and the offset t of kmu_read_syncmers"""
    _fields_ = [("s_kmer_type", C.c_int32), ("s", C.c_int32), ("s_fhash", C.c_int32), ("t", C.c_uint32)]


class ChainParams(C.Structure):
    """kmu_chain_params: how kmu_seed_chains chains and what it reports"""
    _fields_ = [("span", C.c_uint32), ("max_gap", C.c_uint32), ("band", C.c_uint32), ("min_seeds", C.c_uint32),
                ("min_score", C.c_uint32), ("max_pos", C.c_uint32), ("flags", C.c_uint32)]


class Chain(C.Structure):
    """kmu_chain: the chain of one read pair (kmu_seed_chains)"""
    _fields_ = [("read_a", C.c_uint32), ("read_b", C.c_uint32), ("strand", C.c_uint32), ("score", C.c_uint32),
                ("n_seeds", C.c_uint32), ("n_anchors", C.c_uint32), ("a_start", C.c_uint32), ("a_end", C.c_uint32),
                ("b_start", C.c_uint32), ("b_end", C.c_uint32)]


# the same record as a numpy dtype (40 bytes)
CHAIN_DTYPE = [("read_a", "<u4"), ("read_b", "<u4"), ("strand", "<u4"), ("score", "<u4"), ("n_seeds", "<u4"), ("n_anchors", "<u4"),
               ("a_start", "<u4"), ("a_end", "<u4"), ("b_start", "<u4"), ("b_end", "<u4")]


class RankParams(C.Structure):
    """kmu_rank_params: the overlap share that makes a chain secondary (kmu_chain_rank)"""
    _fields_ = [("mask_permille", C.c_uint32), ("flags", C.c_uint32)]


class ChainRank(C.Structure):
    """kmu_chain_rank_rec: rank, parent and secondaries of one chain inside its query read (kmu_chain_rank)"""
    _fields_ = [("rank", C.c_uint32), ("parent", C.c_uint32), ("sub_score", C.c_uint32), ("n_sub", C.c_uint32)]


# the same record as a numpy dtype (16 bytes)
CHAIN_RANK_DTYPE = [("rank", "<u4"), ("parent", "<u4"), ("sub_score", "<u4"), ("n_sub", "<u4")]


class AlignParams(C.Structure):
    """kmu_align_params: the band of kmu_chain_align"""
    _fields_ = [("band", C.c_uint32), ("flags", C.c_uint32)]


class CigarParams(C.Structure):
    """kmu_cigar_params: the band and the trace budget of kmu_chain_cigar"""
    _fields_ = [("band", C.c_uint32), ("flags", C.c_uint32), ("max_trace_bytes", C.c_uint64)]


class PileupParams(C.Structure):
    """kmu_pileup_params: the sides kmu_chain_pileup votes onto"""
    _fields_ = [("flags", C.c_uint32)]


class PileCallParams(C.Structure):
    """kmu_pile_call_params: the depth from which kmu_pile_call calls a base"""
    _fields_ = [("min_depth", C.c_uint32), ("flags", C.c_uint32)]


class InsPlanParams(C.Structure):
    """kmu_ins_plan_params: the most insertion slots kmu_pile_ins_plan gives a base"""
    _fields_ = [("max_ins", C.c_uint32), ("flags", C.c_uint32)]


class ConsensusParams(C.Structure):
    """kmu_consensus_params: kmu_pile_consensus has no options yet"""
    _fields_ = [("flags", C.c_uint32)]


class PileSegParams(C.Structure):
    """kmu_pile_seg_params: the depth, the spanning depth and the length from which kmu_pile_segments keeps a segment"""
    _fields_ = [("min_depth", C.c_uint32), ("min_span", C.c_uint32), ("min_len", C.c_uint32), ("flags", C.c_uint32)]


class PileSeg(C.Structure):
    """kmu_pile_seg: one kept segment, [start, end) in read coordinates"""
    _fields_ = [("read", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("rank", C.c_uint32)]


class ReadTrim(C.Structure):
    """kmu_read_trim: the summary of one read's kept segments (kmu_pile_segments)"""
    _fields_ = [("n_bases", C.c_uint32), ("n_good", C.c_uint32), ("n_segs", C.c_uint32), ("kept", C.c_uint32), ("best_start", C.c_uint32),
                ("best_end", C.c_uint32), ("inner_bad", C.c_uint32), ("cls", C.c_uint32)]


PILE_SEG_DTYPE = [("read", "<u4"), ("start", "<u4"), ("end", "<u4"), ("rank", "<u4")]
READ_TRIM_DTYPE = [("n_bases", "<u4"), ("n_good", "<u4"), ("n_segs", "<u4"), ("kept", "<u4"), ("best_start", "<u4"), ("best_end", "<u4"),
                   ("inner_bad", "<u4"), ("cls", "<u4")]


class SgParams(C.Structure):
    """kmu_sg_params: the thresholds of kmu_sg_classify and kmu_sg_graph"""
    _fields_ = [("min_overlap", C.c_uint32), ("max_hang", C.c_uint32), ("int_permille", C.c_uint32), ("min_identity_permille", C.c_uint32),
                ("fuzz", C.c_uint32), ("flags", C.c_uint32)]


class SgRead(C.Structure):
    """kmu_sg_read: the summary of one read in the string graph"""
    _fields_ = [("flags", C.c_uint32), ("n_records", C.c_uint32), ("out_fwd", C.c_uint32), ("out_rev", C.c_uint32)]


class SgArc(C.Structure):
    """kmu_sg_arc: one arc of the string graph"""
    _fields_ = [("from_", C.c_uint32), ("to", C.c_uint32), ("len", C.c_uint32), ("ovl", C.c_uint32), ("rec", C.c_uint32), ("flags", C.c_uint32),
                ("unique", C.c_uint32), ("zero", C.c_uint32)]


# the same records as numpy dtypes (16 and 32 bytes)
SG_READ_DTYPE = [("flags", "<u4"), ("n_records", "<u4"), ("out_fwd", "<u4"), ("out_rev", "<u4")]
SG_ARC_DTYPE = [("from", "<u4"), ("to", "<u4"), ("len", "<u4"), ("ovl", "<u4"), ("rec", "<u4"), ("flags", "<u4"), ("unique", "<u4"),
                ("zero", "<u4")]
# the records of kmu_sg_unitigs (16, 32 and 16 bytes)
SG_STEP_DTYPE = [("read", "<u4"), ("strand", "<u4"), ("end", "<u8")]
SG_UNITIG_DTYPE = [("first", "<u8"), ("len", "<u8"), ("n_reads", "<u4"), ("flags", "<u4"), ("min_read", "<u4"), ("zero", "<u4")]
SG_PLACE_DTYPE = [("unitig", "<u4"), ("rank", "<u4"), ("strand", "<u4"), ("zero", "<u4")]


class SgCleanParams(C.Structure):
    """kmu_sg_clean_params: the longest tip and the longest bubble branch kmu_sg_clean removes, in reads"""
    _fields_ = [("max_tip_reads", C.c_uint32), ("max_bubble_reads", C.c_uint32), ("flags", C.c_uint32), ("zero", C.c_uint32)]


SG_CLEAN_STATS = ("n_tips", "n_tip_reads", "n_spared", "n_bubbles", "n_bubble_reads", "n_arcs_tip", "n_arcs_bubble", "n_arcs_left")


class SgCleanStats(C.Structure):
    """kmu_sg_clean_stats: what one call of kmu_sg_clean removed and what it left"""
    _fields_ = [(name, C.c_uint64) for name in SG_CLEAN_STATS]


# the same record as a numpy dtype (64 bytes)
SG_CLEAN_STATS_DTYPE = [(name, "<u8") for name in SG_CLEAN_STATS]


class UmParams(C.Structure):
    """kmu_um_params: no flag bits yet"""
    _fields_ = [("flags", C.c_uint32), ("zero", C.c_uint32)]


UM_STATS = ("n_layout", "n_contained", "n_unplaced")


class UmStats(C.Structure):
    """kmu_um_stats: how many reads kmu_sg_unitig_chains placed from the layout, how many through a container, how many not"""
    _fields_ = [(name, C.c_uint64) for name in UM_STATS]


# the same record as a numpy dtype (24 bytes)
UM_STATS_DTYPE = [(name, "<u8") for name in UM_STATS]


class ReadPile(C.Structure):
    """kmu_read_pile: the summary of one read's rows (kmu_pile_call)"""
    _fields_ = [("n_bases", C.c_uint32), ("covered", C.c_uint32), ("n_diff", C.c_uint32), ("n_del", C.c_uint32),
                ("n_ins", C.c_uint32), ("max_depth", C.c_uint32), ("depth_sum", C.c_uint64)]


# the same record as a numpy dtype (32 bytes)
READ_PILE_DTYPE = [("n_bases", "<u4"), ("covered", "<u4"), ("n_diff", "<u4"), ("n_del", "<u4"), ("n_ins", "<u4"), ("max_depth", "<u4"),
                   ("depth_sum", "<u8")]


class ChainAln(C.Structure):
    """kmu_chain_aln: the alignment of one chain's two segments (kmu_chain_align)"""
    _fields_ = [("edit", C.c_uint32), ("matches", C.c_uint32), ("n_diags", C.c_uint32), ("flags", C.c_uint32)]


# the same record as a numpy dtype (16 bytes)
CHAIN_ALN_DTYPE = [("edit", "<u4"), ("matches", "<u4"), ("n_diags", "<u4"), ("flags", "<u4")]


class AnchorIndexInfo(C.Structure):
    """kmu_anchor_index_info_t: the sizes of an anchor index (kmu_anchor_index_info)"""
    _fields_ = [("ndb", C.c_uint32), ("m", C.c_uint32), ("n_keys", C.c_uint32), ("has_groups", C.c_uint32),
                ("n_entries", C.c_uint64), ("n_distinct", C.c_uint64), ("max_occupancy", C.c_uint32), ("pad", C.c_uint32),
                ("device_bytes", C.c_uint64)]


ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)


class IngestInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_kept", C.c_uint64), ("kept_bases", C.c_uint64), ("n_bases", C.c_uint64),
                ("nb_bad_bases", C.c_uint64), ("nb_bad_reads", C.c_uint64)]


RS_PCT_ROWS = 101            # kmu_read_stats: the rows of pct_hist (percentages 0 .. 100), four columns A C G T
RS_QUAL_CLASSES = 8          # kmu_read_qual_stats / kmu_quality_remap: the classes of remap_quality8
RS_NO_BUCKET = 0xFFFFFFFF    # kmu_read_comp.len_bucket of a read beyond the histogram


class ReadStatsParams(C.Structure):
    """kmu_read_stats_params: the layout of the length histogram"""
    _fields_ = [("sig_digits", C.c_int32), ("flags", C.c_int32), ("max_len", C.c_uint64)]


class ReadComp(C.Structure):
    """kmu_read_comp: the base composition of one read (kmu_read_stats)"""
    _fields_ = [("n_base", C.c_uint64 * 4), ("n_other", C.c_uint64), ("pct", C.c_uint8 * 4), ("len_bucket", C.c_uint32)]


READ_STATS_INFO = ("n_reads", "n_bases", "n_base", "n_other", "n_empty", "histo_out", "min_len", "max_len", "n_buckets")


class ReadStatsInfo(C.Structure):
    """kmu_read_stats_info: the totals of one kmu_read_stats call"""
    _fields_ = [(name, C.c_uint64 * 4 if name == "n_base" else C.c_uint64) for name in READ_STATS_INFO]


class ReadQual(C.Structure):
    """kmu_read_qual: the quality classes of one read (kmu_read_qual_stats)"""
    _fields_ = [("n_class", C.c_uint64 * 8), ("sum_q", C.c_uint64), ("min_q", C.c_uint8), ("max_q", C.c_uint8),
                ("median_class", C.c_uint8), ("pad", C.c_uint8 * 5)]


# the same records as numpy dtypes (48, 96 and 80 bytes, the field offsets of the structures)
READ_COMP_DTYPE = [("n_base", "<u8", (4,)), ("n_other", "<u8"), ("pct", "u1", (4,)), ("len_bucket", "<u4")]
READ_STATS_INFO_DTYPE = [(name, "<u8", (4,)) if name == "n_base" else (name, "<u8") for name in READ_STATS_INFO]
READ_QUAL_DTYPE = [("n_class", "<u8", (8,)), ("sum_q", "<u8"), ("min_q", "u1"), ("max_q", "u1"), ("median_class", "u1"), ("pad", "u1", (5,))]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double)]


SIG_NP = {SIG_U32: "uint32", SIG_U64: "uint64", SIG_F32: "float32", SIG_F64: "float64", SIG_U16: "uint16"}


class HllParams(C.Structure):
    """kmu_hll_params: SetSketchParams (b, a, q); m is the sketch size of the call"""
    _fields_ = [("b", C.c_double), ("a", C.c_double), ("q", C.c_uint32), ("reserved", C.c_uint32)]


NTHASH_CANONICAL, NTHASH_FORWARD, NTHASH_RCOMP = 0, 1, 2
NTHASH_TABLE_2B, NTHASH_TABLE_8B = 0, 1


class NthashParams(C.Structure):
    """kmu_nthash_params"""
    _fields_ = [("kmer_size", C.c_int32), ("table", C.c_int32), ("mode", C.c_int32), ("n_hashes", C.c_int32),
                ("input_kind", C.c_int32), ("mem", C.c_int32)]

# kmu_transport
TRANSPORT_DEFAULT, TRANSPORT_COPY = 0, 1
