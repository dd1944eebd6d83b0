"""ctypes binding of libkmu.so (the C-ABI of include/kmu.h).

The product path: every compute call goes to hand-written gfx950 kernels.  There is no CPU fallback -- if the
shared library is missing or no HIP device is present this module raises, loudly.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
# KMU_LIB names another build of the library (A/B experiments: scripts/ab_libs.sh, scripts/pmc_lib.sh) -- the product file
# is never overwritten by an experiment
SO_PATH = os.environ.get("KMU_LIB") or os.path.join(_HERE, "libkmu.so")
_lib = None


def _entry_points():
    """Every entry point include/kmu.h declares: name -> (argtypes, restype, plain).  The one list of them: load() declares each
    signature from it, SYMBOLS is its names (tests check the library exports all of them), and `plain` marks the calls that
    _StreamOrdered does not order behind torch's stream -- they touch no device buffer, or free a handle."""
    vp, u64p, u32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    ingest = [vp, vp, C.c_uint64, C.c_int, vp, C.c_uint64, vp, C.c_uint64, vp, C.POINTER(A.IngestInfo)]
    table = {}

    def d(name, argtypes, restype=C.c_int, plain=False):
        table[name] = (argtypes, restype, plain)
    d("kmu_version", [], C.c_char_p, plain=True)
    d("kmu_device_count", [], plain=True)
    d("kmu_create", [C.POINTER(A.DeviceCfg), C.POINTER(vp)], plain=True)
    d("kmu_destroy", [vp], None, plain=True)
    d("kmu_last_error", [vp], C.c_char_p, plain=True)
    d("kmu_synchronize", [vp])
    d("kmu_stream", [vp], vp, plain=True)
    d("kmu_profile_enable", [vp, C.c_int])
    d("kmu_profile_reset", [vp])
    d("kmu_profile_get", [vp, C.POINTER(A.KernelStat), C.c_int])
    d("kmu_count_non_acgt", [vp, vp, vp, C.c_uint32, C.c_int, vp])
    d("kmu_pack2b", [vp, vp, vp, C.c_uint32, C.c_int, vp, vp])
    d("kmu_kmer_hashes", [vp, C.POINTER(A.HashParams), vp, vp, vp, C.c_uint32, vp])
    d("kmu_kmer_hashes_range", [vp, C.POINTER(A.HashParams), vp, vp, vp, C.c_uint32, vp, vp, vp])
    d("kmu_kmer_distribution", [vp, C.POINTER(A.HashParams), vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, u64p])
    d("kmu_nthash", [vp, C.POINTER(A.NthashParams), vp, vp, vp, C.c_uint32, vp, vp])
    d("kmu_sketch_count", [vp, C.POINTER(A.SketchParams), vp, vp, vp, C.c_uint32, vp])
    d("kmu_host_alloc", [vp, C.c_uint64, C.POINTER(vp)])
    d("kmu_host_free", [vp, vp])
    d("kmu_count_nb_occurrences", [vp, u64p])
    d("kmu_count_nb_saturated", [vp, u64p])
    d("kmu_count_table_info", [vp, C.POINTER(A.CountTableInfo)])
    d("kmu_comm_get_id", [C.POINTER(A.CommId)], plain=True)
    d("kmu_comm_init", [vp, C.POINTER(A.CommId), C.c_int, C.c_int])
    d("kmu_comm_init_custom", [vp, C.c_int, C.c_int, A.ALLTOALLV_FN, A.ALLGATHER_FN, vp])
    d("kmu_comm_set_transport", [vp, C.c_int])
    d("kmu_comm_transport", [vp])
    d("kmu_comm_destroy", [vp], plain=True)
    d("kmu_comm_rank", [vp], plain=True)
    d("kmu_comm_nranks", [vp], plain=True)
    d("kmu_comm_allgather", [vp, vp, vp, C.c_uint64])
    d("kmu_comm_get_stats", [vp, C.POINTER(A.CommStats)], plain=True)
    d("kmu_count_finalize", [vp])
    d("kmu_kmer_owner", [C.c_int, vp, C.c_uint64, C.c_uint32, vp], plain=True)
    d("kmu_kmer_owner_minimizer", [C.c_int, vp, C.c_uint64, C.c_uint32, vp])
    d("kmu_count_owner_kind", [vp])
    d("kmu_count_extract_superkmers", [vp, vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(vp), vp, vp])
    d("kmu_count_add_superkmers", [vp, vp, C.c_uint64, C.c_int])
    d("kmu_sketch", [vp, C.POINTER(A.SketchParams), vp, vp, vp, C.c_uint32, vp, vp, vp])
    d("kmu_sketch_groups", [vp, C.POINTER(A.SketchParams), vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp])
    d("kmu_block_layout", [vp, C.c_uint32, C.c_uint32, vp], plain=True)
    d("kmu_anchor_layout", [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp], plain=True)
    d("kmu_read_anchors", [vp, C.POINTER(A.SketchParams), vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp])
    d("kmu_sketch_hashed", [vp, C.POINTER(A.SketchParams), vp, vp, C.c_uint32, vp, vp])
    d("kmu_count_create", [vp, C.POINTER(A.CountParams), C.POINTER(vp)])
    d("kmu_count_destroy", [vp], None, plain=True)
    d("kmu_count_reset", [vp])
    d("kmu_count_add_reads", [vp, vp, vp, vp, C.c_uint32, C.c_int, C.c_int])
    d("kmu_count_add_kmers", [vp, vp, C.c_uint64, C.c_int])
    d("kmu_count_query", [vp, vp, C.c_uint64, C.c_int, vp])
    d("kmu_count_nb_distinct", [vp, u64p])
    d("kmu_count_nb_unique", [vp, u64p])
    d("kmu_count_dump", [vp, C.c_uint32, vp, vp, C.c_uint64, u64p])
    d("kmu_count_export_part", [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, C.c_int, u64p])
    d("kmu_count_merge_entries", [vp, vp, vp, C.c_uint64, C.c_int])
    d("kmu_count_retain_part", [vp, C.c_uint32, C.c_uint32])
    d("kmu_count_extract_by_owner", [vp, vp, vp, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(vp), vp])
    d("kmu_sig_equal_pairs", [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp, C.c_uint64, C.c_int, vp])
    d("kmu_sig_equal_matrix", [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp])
    d("kmu_sig_knn", [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, vp, vp, C.c_int, vp, vp])
    d("kmu_minhash_distance_pairs", [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, C.c_int, vp])
    d("kmu_anchor_match", [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_int, vp, vp,
                           C.c_uint64, u64p])
    d("kmu_anchor_overlaps", [vp, vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                              C.c_uint32, C.c_int, vp, C.c_uint64, u64p])
    d("kmu_anchor_index_create", [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int, C.POINTER(vp)])
    d("kmu_anchor_index_destroy", [vp], None, plain=True)
    d("kmu_anchor_index_info", [vp, C.POINTER(A.AnchorIndexInfo)], plain=True)
    d("kmu_anchor_index_occupancy", [vp, vp, C.c_uint32, C.c_int])
    d("kmu_anchor_index_match", [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp, C.c_uint64, u64p])
    d("kmu_components", [vp, C.c_uint32, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp, u32p])
    d("kmu_components_knn", [vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp, vp, u32p])
    d("kmu_minimizer_layout", [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp], plain=True)
    d("kmu_read_minimizers", [vp, C.POINTER(A.HashParams), vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, u64p])
    d("kmu_read_syncmers", [vp, C.POINTER(A.HashParams), C.POINTER(A.SyncmerParams), vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, u64p])
    d("kmu_seed_chains", [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32,
                          C.POINTER(A.ChainParams), C.c_int, vp, C.c_uint64, u64p])
    d("kmu_seed_chains_all", [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32,
                              C.POINTER(A.ChainParams), C.c_int, vp, C.c_uint64, u64p])
    d("kmu_chain_rank", [vp, vp, C.c_uint64, C.c_uint32, C.POINTER(A.RankParams), C.c_int, vp])
    d("kmu_chain_align", [vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.POINTER(A.AlignParams), C.c_int, vp])
    d("kmu_chain_cigar", [vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.POINTER(A.CigarParams), C.c_int, vp, vp,
                          vp, C.c_uint64, u64p])
    d("kmu_chain_pileup", [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint32,
                           C.POINTER(A.PileupParams), C.c_int, vp, vp])
    d("kmu_pile_call", [vp, vp, vp, vp, C.c_uint32, C.POINTER(A.PileCallParams), C.c_int, vp, vp])
    d("kmu_pile_ins_plan", [vp, vp, vp, C.c_uint64, C.POINTER(A.InsPlanParams), C.c_int, vp, C.POINTER(C.c_uint64)])
    d("kmu_chain_pile_ins", [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint32,
                             C.POINTER(A.PileupParams), C.c_int, vp, C.c_uint64, vp, vp, C.c_uint64, vp])
    d("kmu_pile_consensus", [vp, vp, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, C.POINTER(A.ConsensusParams), C.c_int, vp, vp,
                             C.c_uint64, C.POINTER(C.c_uint64)])
    d("kmu_pile_segments", [vp, vp, vp, C.c_uint32, C.POINTER(A.PileSegParams), C.c_int, vp, vp, C.c_uint64, C.POINTER(C.c_uint64), vp])
    d("kmu_extract_ranges", [vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.c_int, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)])
    d("kmu_pile_consensus_pos", [vp, vp, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint32, C.POINTER(A.ConsensusParams), C.c_int, vp,
                                 C.c_uint64, vp])
    d("kmu_sg_classify", [vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.POINTER(A.SgParams), C.c_int, vp, vp])
    d("kmu_sg_graph", [vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.POINTER(A.SgParams), C.c_int, vp, vp, vp, C.c_uint64, vp,
                       C.POINTER(C.c_uint64)])
    d("kmu_sg_unitigs", [vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_int, vp, vp, vp, u64p, u64p])
    d("kmu_sg_unitig_seqs", [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_int, vp, vp, C.c_uint64, u64p])
    d("kmu_sg_clean", [vp, vp, C.c_uint64, vp, C.c_uint32, C.POINTER(A.SgCleanParams), C.c_int, vp, vp, C.POINTER(A.SgCleanStats)])
    d("kmu_sg_unitig_chains", [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.POINTER(A.UmParams),
                               C.c_int, vp, C.POINTER(A.UmStats), u64p])
    d("kmu_set_hll_params", [vp, C.POINTER(A.HllParams)])
    d("kmu_kmer_hashes_compact", [vp, C.POINTER(A.HashParams), vp, vp, vp, C.c_uint32, vp, C.c_uint64, u64p])
    d("kmu_sketch_partial_words", [C.POINTER(A.SketchParams)], C.c_uint32, plain=True)
    d("kmu_sketch_partial", [vp, C.POINTER(A.SketchParams), vp, vp, vp, C.c_uint32, vp])
    d("kmu_sketch_hashed_partial", [vp, C.POINTER(A.SketchParams), vp, vp, C.c_uint32, vp])
    d("kmu_sketch_merge_partials", [vp, C.POINTER(A.SketchParams), vp, C.c_uint32, vp])
    d("kmu_count_eliminate_once", [vp])
    d("kmu_count_once_positions", [vp, vp, vp, C.c_uint32, C.c_int, vp, vp, vp, C.c_uint64, u64p])
    d("kmu_count_histogram", [vp, vp, C.c_uint32, C.c_int])
    d("kmu_count_read_profile", [vp, vp, vp, C.c_uint32, C.c_int, C.c_uint32, vp, vp])
    d("kmu_kfilter_cells_for", [C.c_uint64, C.c_uint32], C.c_uint64, plain=True)
    d("kmu_kfilter_create", [vp, C.POINTER(A.KFilterParams), C.POINTER(vp)])
    d("kmu_kfilter_destroy", [vp], None, plain=True)
    d("kmu_kfilter_reset", [vp])
    d("kmu_kfilter_add_reads", [vp, vp, vp, C.c_uint32, C.c_int])
    d("kmu_kfilter_add_kmers", [vp, vp, C.c_uint64, C.c_int])
    d("kmu_kfilter_query", [vp, vp, C.c_uint64, C.c_int, vp])
    d("kmu_kfilter_info", [vp, C.POINTER(A.KFilterInfo)])
    d("kmu_kfilter_export", [vp, vp, C.c_int])
    d("kmu_kfilter_merge", [vp, vp])
    d("kmu_kfilter_select_reads", [vp, vp, vp, C.c_uint32, C.c_int, vp, C.c_uint64, u64p])
    d("kmu_count_add_reads_filtered", [vp, vp, vp, vp, C.c_uint32, C.c_int, u64p])
    d("kmu_dev_alloc", [vp, C.c_uint64, C.POINTER(vp)])
    d("kmu_dev_free", [vp, vp])
    d("kmu_copy_to_device", [vp, vp, vp, C.c_uint64])
    d("kmu_copy_to_host", [vp, vp, vp, C.c_uint64])
    d("kmu_ingest_fastq", ingest)
    d("kmu_ingest_fasta", ingest)
    d("kmu_ingest_fastx", ingest)
    d("kmu_ingest_fastq_qual", ingest[:6] + [vp, C.c_uint64] + ingest[6:])
    d("kmu_len_hist_layout", [C.c_uint64, C.c_int, u32p, u64p], plain=True)
    d("kmu_len_bucket_range", [C.c_int, C.c_uint32, u64p, u64p], plain=True)
    d("kmu_read_stats", [vp, C.POINTER(A.ReadStatsParams), vp, vp, C.c_uint32, C.c_int, vp, vp, vp, C.POINTER(A.ReadStatsInfo)])
    d("kmu_quality_remap", [vp, vp, C.c_uint64, C.c_int, vp])
    d("kmu_read_qual_stats", [vp, vp, vp, C.c_uint32, C.c_int, vp, vp])
    return table


_ENTRY_POINTS = _entry_points()
SYMBOLS = list(_ENTRY_POINTS)


# what Context.components / components_knn return: label [n] (the smallest node of every node's component), cluster [n] (dense
# ids in the order of the smallest member), size [n_components], members [n] (nodes by (cluster, node)) and n_components; a
# field that was not asked for is None
Components = collections.namedtuple("Components", "label cluster size members n_components")
COMPONENTS_WANT = ("cluster", "size", "members")
MINIMIZERS_WANT = ("pos", "read", "strand")  # the optional outputs of Context.read_minimizers
READ_STATS_WANT = ("comp", "pct", "len")     # the optional outputs of Context.read_stats
READ_QUAL_WANT = ("reads", "hist")           # the optional outputs of Context.read_qual_stats
PILE_CALL_WANT = ("call", "reads")           # the outputs of Context.pile_call


class KmuError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("%s: %s" % (A.STATUS_NAMES.get(code, str(code)), msg))
        self.code = code


def load():
    """Load libkmu.so; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError("kmerutils_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback." % SO_PATH)
    L = C.CDLL(SO_PATH)
    for name, (argtypes, restype, _) in _ENTRY_POINTS.items():
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype
    _lib = L
    return L


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ptr(x):
    """(pointer, is_device) of a numpy array, a torch tensor, or None"""
    if x is None:
        return None, False
    if _is_torch(x):
        assert x.is_contiguous()
        return C.c_void_p(x.data_ptr()), x.is_cuda
    assert x.flags["C_CONTIGUOUS"]
    return x.ctypes.data_as(C.c_void_p), False


class _StreamOrdered:
    """libkmu's entry points as seen by one Context: every call is first ordered behind torch's current stream.

    The library enqueues on the context's stream.  When that is not torch's current stream (a context that owns its
    stream), nothing orders it behind work torch has queued on its own stream -- the producers of the input tensors, and
    the zero-fill of an output tensor allocated a line earlier, which could otherwise land on top of the kernel's results.
    Doing it here, at the one place every call passes through, covers the buffers of every present and future method."""

    _PLAIN = frozenset(name for name, entry in _ENTRY_POINTS.items() if entry[2])

    def __init__(self, lib, ctx):
        self._lib = lib
        self._ctx = ctx

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name in self._PLAIN:
            return f
        ctx = self._ctx

        def call(*args):
            ctx._order_after_torch()
            return f(*args)
        setattr(self, name, call)
        return call


class Context:
    """kmu_ctx: one HIP device + stream.  Use from one thread at a time."""

    def __init__(self, device_id=0, stream=None, async_device=False):
        lib = load()
        self.h = None
        self.device_id = device_id
        self.L = _StreamOrdered(lib, self)
        cfg = A.DeviceCfg(device_id, 1 if async_device else 0, stream, 0)
        h = C.c_void_p()
        rc = lib.kmu_create(C.byref(cfg), C.byref(h))
        if rc:
            raise KmuError(rc, lib.kmu_last_error(None).decode())
        self.h = h
        self._stream = lib.kmu_stream(h) or 0

    def close(self):
        if getattr(self, "h", None):
            self.L.kmu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise KmuError(rc, self.L.kmu_last_error(self.h).decode())

    def synchronize(self):
        self._check(self.L.kmu_synchronize(self.h))

    @property
    def stream(self):
        return self._stream

    def set_hll_params(self, b=1.001, a=20.0, q=65534):
        """kmu_set_hll_params: SetSketchParams of the following ALGO_HLL sketches on this context"""
        hp = A.HllParams(b, a, q, 0)
        self._check(self.L.kmu_set_hll_params(self.h, C.byref(hp)))

    # ---- communicator (one rank per GPU; kmu.h "multi-GPU") ----
    @staticmethod
    def comm_get_id():
        """kmu_comm_get_id: 128 bytes that rank 0 creates and hands to every other rank"""
        L = load()
        cid = A.CommId()
        rc = L.kmu_comm_get_id(C.byref(cid))
        if rc:
            raise KmuError(rc, L.kmu_last_error(None).decode())
        return bytes(C.string_at(C.byref(cid), A.COMM_ID_BYTES))

    def comm_init(self, comm_id, rank, nranks):
        """kmu_comm_init: RCCL communicator over the ranks' GPUs (collective)"""
        cid = A.CommId()
        C.memmove(C.byref(cid), comm_id, A.COMM_ID_BYTES)
        self._check(self.L.kmu_comm_init(self.h, C.byref(cid), rank, nranks))

    def comm_init_custom(self, rank, nranks, alltoallv, allgather):
        """kmu_comm_init_custom: `alltoallv(send_ptr, send_counts, send_displs, recv_ptr, recv_counts, recv_displs,
        elem_bytes)` (device pointers as ints, counts as lists) and `allgather(bytes) -> bytes of all ranks` supplied by
        the caller; exceptions inside them are reported as KMU_E_RCCL."""
        def a2a(_user, sp, sc, sd, rp, rc_, rd, eb, _stream):
            try:
                alltoallv(sp or 0, [sc[i] for i in range(nranks)], [sd[i] for i in range(nranks)], rp or 0,
                          [rc_[i] for i in range(nranks)], [rd[i] for i in range(nranks)], eb)
                return 0
            except Exception:  # noqa: BLE001 -- must not unwind through C
                import traceback
                traceback.print_exc()
                return 1

        def ag(_user, sp, rp, nbytes):
            try:
                out = allgather(C.string_at(sp, nbytes))
                assert len(out) == nbytes * nranks
                C.memmove(rp, out, len(out))
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        # alltoallv None: the library's COPY transport (device copies into the peers' receive buffers) over the caller's all-gather
        self._comm_cbs = (A.ALLTOALLV_FN(a2a) if alltoallv is not None else C.cast(None, A.ALLTOALLV_FN), A.ALLGATHER_FN(ag))  # keep the trampolines alive
        self._check(self.L.kmu_comm_init_custom(self.h, rank, nranks, self._comm_cbs[0], self._comm_cbs[1], None))

    def comm_set_transport(self, transport):
        """kmu_comm_set_transport: A.TRANSPORT_DEFAULT (RCCL / the host's all-to-all) or A.TRANSPORT_COPY (IPC-mapped device copies)"""
        self._check(self.L.kmu_comm_set_transport(self.h, int(transport)))

    @property
    def comm_transport(self):
        return self.L.kmu_comm_transport(self.h)

    def comm_destroy(self):
        self._check(self.L.kmu_comm_destroy(self.h))

    @property
    def comm_rank(self):
        return self.L.kmu_comm_rank(self.h)

    @property
    def comm_nranks(self):
        return self.L.kmu_comm_nranks(self.h)

    def comm_allgather(self, payload):
        """kmu_comm_allgather: bytes from every rank, in rank order"""
        n = self.comm_nranks
        src = C.create_string_buffer(bytes(payload), len(payload))
        dst = C.create_string_buffer(len(payload) * n)
        self._check(self.L.kmu_comm_allgather(self.h, src, dst, len(payload)))
        return dst.raw

    def comm_stats(self):
        st = A.CommStats()
        self._check(self.L.kmu_comm_get_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in A.CommStats._fields_}

    # ---- profiling ----
    def profile_enable(self, on=True):
        self._check(self.L.kmu_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        self._check(self.L.kmu_profile_reset(self.h))

    def profile_get(self):
        arr = (A.KernelStat * 32)()
        n = self.L.kmu_profile_get(self.h, arr, 32)
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(min(n, 32))}

    def _order_after_torch(self):
        """Wait for what torch has queued on its current stream of this device, unless that IS the context's stream
        (then stream order does it).  Only when torch is loaded and has touched the GPU: host-only callers never pay."""
        import sys
        torch = sys.modules.get("torch")
        if torch is None or self.h is None or not torch.cuda.is_initialized():
            return
        cur = torch.cuda.current_stream(self.device_id)
        if cur.cuda_stream != self._stream:
            cur.synchronize()

    # ---- helpers ----
    @staticmethod
    def _mem(*xs):
        dev = [d for (_, d) in (_ptr(x) for x in xs if x is not None)]
        if any(dev) and not all(dev):
            raise ValueError("all buffers of one call must live on the same side (host or device)")
        return A.MEM_DEVICE if dev and dev[0] else A.MEM_HOST

    def _new_like(self, ref, shape, np_dtype, torch_dtype_name):
        if _is_torch(ref) and ref.is_cuda:
            import torch
            return torch.zeros(shape, dtype=getattr(torch, torch_dtype_name), device=ref.device)
        return np.zeros(shape, np_dtype)

    def _records(self, like, n, dtype):
        """n records of a structured A.*_DTYPE where `like` lives, one at least so that there is an address: a structured array
        on the host, an int32 tensor [n, words of a record] holding the same bits on the device"""
        dtype = np.dtype(dtype)
        if _is_torch(like) and like.is_cuda:
            return self._new_like(like, (max(n, 1), dtype.itemsize // 4), np.int32, "int32")
        return np.zeros(max(n, 1), dtype)

    def _ptrs(self, like):
        """ptr(x) for the inputs of one call: the pointer of x, or where x has no rows (`rows`, where another count decides) that
        of a placeholder of 16 bytes where `like` lives -- an empty array has no address worth passing (an empty device tensor's
        is null), and the library reads no row of it.  The placeholder is made when it is first needed and shared by every ptr
        of one _ptrs call, and lives as long as `ptr` does; a second _ptrs call has a second one."""
        none = []

        def ptr(x, rows=None):
            if int(x.shape[0]) if rows is None else rows:
                return _ptr(x)[0]
            if not none:
                none.append(self._new_like(like, 16, np.uint8, "uint8"))
            return _ptr(none[0])[0]
        return ptr

    def _offsets_like(self, x, ref, mem):
        """the offsets of a batch as uint64 where the arrays of the call live (int64 holding the same bits for torch)"""
        if _is_torch(x):
            if x.is_cuda == (mem == A.MEM_DEVICE):
                return x
            x = x.cpu().numpy()
        x = np.ascontiguousarray(np.asarray(x).astype(np.uint64))
        if mem == A.MEM_DEVICE:
            import torch
            return torch.from_numpy(x.view(np.int64)).to(ref.device)
        return x

    def _offsets_pair(self, offsets_q, offsets_db, ref, mem):
        """_offsets_like of the two batches of a call; one object given for both is converted once"""
        off_q = self._offsets_like(offsets_q, ref, mem)
        return off_q, off_q if offsets_db is offsets_q else self._offsets_like(offsets_db, ref, mem)

    @staticmethod
    def _db_batch(bases_q, offsets_q, bases_db, offsets_db):
        """(bases, offsets) of the second batch of a chain call: the first batch again for the self-join (bases_db None)"""
        if bases_db is None:
            return bases_q, offsets_q
        if offsets_db is None:
            raise ValueError("bases_db without offsets_db")
        return bases_db, offsets_db

    def _runs_of_chains(self, chains, aln, ops, op_offsets, *more):
        """what chain_pileup and chain_pile_ins take from chain_cigar: (chains, aln) contiguous, the side of the call over these
        and `more`, and the number of chains, with one alignment record and one run offset (and one more) each"""
        if not _is_torch(chains):
            chains = np.ascontiguousarray(chains)
        if not _is_torch(aln):
            aln = np.ascontiguousarray(aln)
        mem = self._mem(chains, aln, ops, op_offsets, *more)
        n = int(chains.shape[0])
        if int(aln.shape[0]) != n or int(op_offsets.shape[0]) != n + 1:
            raise ValueError("%d chains need %d alignment records and %d run offsets" % (n, n, n + 1))
        return chains, aln, mem, n

    def _side_tables(self, like, sides, own, into, rows_q, rows_db, cols):
        """(table_q, table_db) of chain_pileup / chain_pile_ins: into=(table_q, table_db), or one table for both, as given;
        otherwise uint32 [rows, cols] tables of zeros where `like` lives, one under both names for the self-join (`own`).  rows_*:
        a number, or a function that gives it and is asked only for a table that is made (where the number has to be read back
        from the device).  The table of a side that `sides` leaves out is None."""
        def rows(r):
            return r() if callable(r) else r
        if into is not None:
            table_q, table_db = into if isinstance(into, (tuple, list)) else (into, into)
            if (sides & A.PILE_Q and table_q is None) or (sides & A.PILE_DB and table_db is None):
                raise ValueError("into lacks the table of a side that is asked for")
            return table_q, table_db
        table_q = self._new_like(like, (rows(rows_q), cols), np.uint32, "int32") if sides & A.PILE_Q else None
        if own and table_q is not None:
            return table_q, (table_q if sides & A.PILE_DB else None)
        return table_q, (self._new_like(like, (rows(rows_db), cols), np.uint32, "int32") if sides & A.PILE_DB else None)

    def _kmer_values(self, canon):
        """(values, how many, mem) of k-mer values to look up: a device tensor as it is, anything on the host as contiguous uint64"""
        mem = self._mem(canon)
        if mem == A.MEM_DEVICE:
            return canon, canon.numel(), mem
        canon = np.ascontiguousarray(canon, np.uint64)
        return canon, canon.size, mem

    def _two_calls(self, fn, args, alloc, n_out=1, cap_at=None, always=False):
        """The count-then-write protocol of the library, fn(*args, *outputs, capacity, &total): once with null outputs and
        capacity 0 for the total, then alloc(total) gives the n_out outputs (a tuple) and the call is made again with exactly that
        capacity -- with a total of 0 only if `always` (the calls whose second pass also writes offsets or summaries).  cap_at: the
        capacity stands behind the first cap_at outputs, not behind all.  Returns (outputs, total)."""
        total = C.c_uint64(0)
        at = n_out if cap_at is None else cap_at

        def call(outs, cap):
            p = [_ptr(x)[0] for x in outs]
            self._check(fn(*args, *p[:at], cap, *p[at:], C.byref(total)))
        call((None,) * n_out, 0)
        n = int(total.value)
        outs = alloc(n)
        if n or always:
            call(outs, n)
        return outs, n

    def count_non_acgt(self, bases, offsets):
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        out = self._new_like(bases, max(n, 1), np.uint64, "int64")
        self._check(self.L.kmu_count_non_acgt(self.h, _ptr(bases)[0], _ptr(offsets)[0], n, mem, _ptr(out)[0]))
        return out[:n]

    def pack2b(self, bases, offsets):
        n = len(offsets) - 1
        L = np.diff(offsets.astype(np.int64))
        poff = np.zeros(n + 1, np.uint64)
        out = np.zeros(int(((L + 3) // 4).sum()) + 16, np.uint8)
        self._check(self.L.kmu_pack2b(self.h, _ptr(bases)[0], _ptr(offsets)[0], n, A.MEM_HOST, _ptr(out)[0],
                                      _ptr(poff)[0]))
        return out[:int(poff[-1])], poff

    def kmer_hashes(self, bases, offsets, kmer_type, k, fhash, input_kind=A.INPUT_ASCII, packed_offsets=None,
                    out=None):
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        hp = A.HashParams(kmer_type, k, fhash, input_kind, mem, 0)
        if out is None:
            if mem == A.MEM_DEVICE:
                import torch
                out = torch.zeros(max(int(offsets[-1].item()), 1), dtype=torch.int64, device=bases.device)
            else:
                out = np.zeros(max(int(offsets[-1]), 1), np.uint64)
        self._check(self.L.kmu_kmer_hashes(self.h, C.byref(hp), _ptr(bases)[0], _ptr(offsets)[0],
                                           _ptr(packed_offsets)[0], n, _ptr(out)[0]))
        return out

    def kmer_hashes_range(self, bases, offsets, kmer_type, k, fhash, range_begin, range_end, input_kind=A.INPUT_ASCII,
                          packed_offsets=None, out=None):
        """kmu_kmer_hashes_range: generate_kmer_pattern_in_range -- fhash of the k-mers inside bases [begin_i, end_i) of
        every sequence, at out[offsets[i] + p]; a bad range raises KMU_E_BAD_ARG (the reference's set_range Err)."""
        n = len(offsets) - 1
        mem = self._mem(bases, offsets, range_begin, range_end)
        hp = A.HashParams(kmer_type, k, fhash, input_kind, mem, 0)
        if out is None:
            if mem == A.MEM_DEVICE:
                import torch
                out = torch.zeros(max(int(offsets[-1].item()), 1), dtype=torch.int64, device=bases.device)
            else:
                out = np.zeros(max(int(offsets[-1]), 1), np.uint64)
        self._check(self.L.kmu_kmer_hashes_range(self.h, C.byref(hp), _ptr(bases)[0], _ptr(offsets)[0], _ptr(packed_offsets)[0],
                                                 n, _ptr(range_begin)[0], _ptr(range_end)[0], _ptr(out)[0]))
        return out

    def kmer_distribution(self, bases, offsets, kmer_type, k, fhash=A.FHASH_IDENTITY_RAW, input_kind=A.INPUT_ASCII,
                          packed_offsets=None):
        """kmu_kmer_distribution: generate_kmer_distribution -- (values, multiplicities, dist_offsets): the distinct fhash
        values of sequence i and their counts are [dist_offsets[i], dist_offsets[i + 1]) of the first two arrays."""
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        hp = A.HashParams(kmer_type, k, fhash, input_kind, mem, 0)
        args = (self.h, C.byref(hp), _ptr(bases)[0], _ptr(offsets)[0], _ptr(packed_offsets)[0], n)
        (kk, cc, do), cnt = self._two_calls(self.L.kmu_kmer_distribution, args, lambda cnt: (
            self._new_like(bases, max(cnt, 1), np.uint64, "int64"), self._new_like(bases, max(cnt, 1), np.uint32, "int32"),
            self._new_like(bases, n + 1, np.uint64, "int64")), n_out=3, cap_at=2, always=True)
        return kk[:cnt], cc[:cnt], do

    def nthash(self, bases, offsets, k, n_hashes=1, mode=A.NTHASH_CANONICAL, table=A.NTHASH_TABLE_2B,
               input_kind=A.INPUT_ASCII, packed_offsets=None, want_strand=True, out=None, strand_out=None):
        """kmu_nthash: (hashes [n_bases, n_hashes] u64, strand [n_bases] u8) -- rows of positions that start no k-mer
        stay untouched (zero in freshly allocated outputs)."""
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        np_ = A.NthashParams(k, table, mode, n_hashes, input_kind, mem)
        if mem == A.MEM_DEVICE:
            import torch
            nb = max(int(offsets[-1].item()), 1)
            if out is None:
                out = torch.zeros((nb, n_hashes), dtype=torch.int64, device=bases.device)
            if want_strand and strand_out is None:
                strand_out = torch.zeros(nb, dtype=torch.uint8, device=bases.device)
        else:
            nb = max(int(offsets[-1]), 1)
            if out is None:
                out = np.zeros((nb, n_hashes), np.uint64)
            if want_strand and strand_out is None:
                strand_out = np.zeros(nb, np.uint8)
        self._check(self.L.kmu_nthash(self.h, C.byref(np_), _ptr(bases)[0], _ptr(offsets)[0], _ptr(packed_offsets)[0], n,
                                      _ptr(out)[0], _ptr(strand_out)[0]))
        return (out, strand_out) if want_strand else out

    def kmer_hashes_compact(self, bases, offsets, kmer_type, k, fhash, input_kind=A.INPUT_ASCII, packed_offsets=None):
        """kmu_kmer_hashes_compact: fhash of every k-mer, sequence after sequence, no gaps (uint64 / int64 tensor)"""
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        hp = A.HashParams(kmer_type, k, fhash, input_kind, mem, 0)
        args = (self.h, C.byref(hp), _ptr(bases)[0], _ptr(offsets)[0], _ptr(packed_offsets)[0], n)
        (out,), cnt = self._two_calls(self.L.kmu_kmer_hashes_compact, args,
                                      lambda cnt: (self._new_like(bases, max(cnt, 1), np.uint64, "int64"),), always=True)
        return out[:cnt]

    def block_layout(self, offsets_host, block_size):
        n = len(offsets_host) - 1
        out = np.zeros(n + 1, np.uint64)
        rc = self.L.kmu_block_layout(_ptr(offsets_host)[0], n, block_size, _ptr(out)[0])
        self._check(rc)
        return out

    def sketch(self, bases, offsets, params, packed_offsets=None, block_row_offsets=None, n_rows=None, out=None,
               counts_out=None, want_counts=False):
        """kmu_sketch.  Host (numpy) or device (torch cuda) buffers.  Returns sig [rows, m] (and counts)."""
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        p = A.SketchParams.from_buffer_copy(params)
        p.mem = mem
        m = p.sketch_size
        if p.block_size > 0:
            if block_row_offsets is None:
                if mem != A.MEM_HOST:
                    raise ValueError("device block sketching needs block_row_offsets (+ n_rows)")
                block_row_offsets = self.block_layout(np.ascontiguousarray(offsets, np.uint64), p.block_size)
            rows = int(n_rows if n_rows is not None else block_row_offsets[-1])
        else:
            rows = 1 if p.mode == A.MODE_ALL_SEQS else n
        if out is None:
            if mem == A.MEM_DEVICE:
                import torch
                tdt = {A.SIG_U32: torch.int32, A.SIG_U64: torch.int64, A.SIG_F32: torch.float32,
                       A.SIG_F64: torch.float64, A.SIG_U16: torch.int16}[p.sig_type]
                out = torch.zeros((max(rows, 1), m), dtype=tdt, device=bases.device)
                if want_counts and counts_out is None:
                    counts_out = torch.zeros((max(rows, 1), m), dtype=torch.int32, device=bases.device)
            else:
                out = np.zeros((max(rows, 1), m), dtype=A.SIG_NP[p.sig_type])
                if want_counts and counts_out is None:
                    counts_out = np.zeros((max(rows, 1), m), np.uint32)
        self._check(self.L.kmu_sketch(self.h, C.byref(p), _ptr(bases)[0], _ptr(offsets)[0], _ptr(packed_offsets)[0],
                                      n, _ptr(block_row_offsets)[0], _ptr(out)[0], _ptr(counts_out)[0]))
        out = out[:rows]
        if want_counts:
            return out, counts_out[:rows]
        return out

    def sketch_groups(self, bases, offsets, group_offsets, params, packed_offsets=None, out=None):
        """kmu_sketch_groups: one signature per group of consecutive sequences, sig [n_groups, m]; row g is the ALL_SEQS row of
        the sequences group_offsets[g] .. group_offsets[g + 1].  Host (numpy) or device (torch cuda) buffers, `group_offsets`
        on the same side as `offsets`."""
        n = len(offsets) - 1
        if not _is_torch(group_offsets):
            group_offsets = np.ascontiguousarray(group_offsets, np.uint64)
        n_groups = len(group_offsets) - 1
        mem = self._mem(bases, offsets, group_offsets)
        p = A.SketchParams.from_buffer_copy(params)
        p.mem = mem
        m = p.sketch_size
        if out is None:
            if mem == A.MEM_DEVICE:
                import torch
                tdt = {A.SIG_U32: torch.int32, A.SIG_U64: torch.int64, A.SIG_F32: torch.float32,
                       A.SIG_F64: torch.float64, A.SIG_U16: torch.int16}[p.sig_type]
                out = torch.zeros((max(n_groups, 1), m), dtype=tdt, device=bases.device)
            else:
                out = np.zeros((max(n_groups, 1), m), dtype=A.SIG_NP[p.sig_type])
        self._check(self.L.kmu_sketch_groups(self.h, C.byref(p), _ptr(bases)[0], _ptr(offsets)[0], _ptr(packed_offsets)[0],
                                             n, _ptr(group_offsets)[0], n_groups, _ptr(out)[0]))
        return out[:n_groups]

    def anchor_layout(self, offsets_host, window, overlap):
        """kmu_anchor_layout: first row of every read, ceil(L / (window - overlap)) rows per read (host arithmetic)"""
        return anchor_layout(offsets_host, window, overlap)

    def read_anchors(self, bases, offsets, params, window, overlap, want_counts=True):
        """kmu_read_anchors: one bottom-k row per overlapping window of every read (ReadAnchors, anchor.rs:228-329).
        Host (numpy) or device (torch cuda) buffers.  Returns (hashes [rows, nbkmer], counts [rows, nbkmer] or None,
        n [rows], row_offsets [n_seq + 1]): numpy arrays for host input; for device input torch tensors holding the same bits
        (int64 / int32), row_offsets as a numpy array (it is computed on the host from a host copy of `offsets`)."""
        nseq = len(offsets) - 1
        mem = self._mem(bases, offsets)
        p = A.SketchParams.from_buffer_copy(params)
        p.mem = mem
        m = p.sketch_size
        h_off = np.ascontiguousarray(offsets.cpu().numpy() if _is_torch(offsets) else offsets).astype(np.uint64)
        row_offsets = anchor_layout(h_off, window, overlap)
        rows = int(row_offsets[-1])
        if mem == A.MEM_DEVICE:
            import torch
            d_rows = torch.from_numpy(row_offsets.astype(np.int64)).to(bases.device)
            hashes = torch.zeros((max(rows, 1), m), dtype=torch.int64, device=bases.device)
            counts = torch.zeros((max(rows, 1), m), dtype=torch.int32, device=bases.device) if want_counts else None
            n = torch.zeros(max(rows, 1), dtype=torch.int32, device=bases.device)
        else:
            d_rows = row_offsets
            hashes = np.zeros((max(rows, 1), m), np.uint64)
            counts = np.zeros((max(rows, 1), m), np.uint32) if want_counts else None
            n = np.zeros(max(rows, 1), np.uint32)
        self._check(self.L.kmu_read_anchors(self.h, C.byref(p), _ptr(bases)[0], _ptr(offsets)[0], nseq, window, overlap,
                                            _ptr(d_rows)[0], _ptr(hashes)[0], _ptr(counts)[0], _ptr(n)[0]))
        return hashes[:rows], (counts[:rows] if want_counts else None), n[:rows], row_offsets

    def read_minimizers(self, bases, offsets, kmer_type, k, fhash, w, want=MINIMIZERS_WANT):
        """kmu_read_minimizers: the (w, k) window minimizers of every read -- per window of w consecutive k-mers the position of
        smallest kmer_hashes value, ties to the smallest position, each chosen position once (include/kmu.h has the rules).
        Returns (hashes, pos, read, strand, mini_offsets): the minimizers of read i are the entries mini_offsets[i] ..
        mini_offsets[i + 1], ascending in position; `want` names the optional outputs to compute ("pos", "read", "strand"), the
        others are None (the ntHash orders have no strand: leave it out).  numpy in gives numpy out (uint64 / uint32 / uint8);
        torch cuda tensors stay on the device (int64 / int32 / uint8 tensors holding the same bits).  Two library calls: one
        that counts, one with exactly that capacity."""
        unknown = [x for x in want if x not in MINIMIZERS_WANT]
        if unknown:
            raise ValueError("want holds %r: the optional outputs are %r" % (unknown, MINIMIZERS_WANT))
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        hp = A.HashParams(kmer_type, k, fhash, A.INPUT_ASCII, mem, 0)
        moff = self._new_like(bases, n + 1, np.uint64, "int64")
        total = C.c_uint64(0)
        ptr = self._ptrs(bases)  # (a batch of empty reads has no bases)
        args = (self.h, C.byref(hp), ptr(bases), _ptr(offsets)[0], n, int(w))
        # (the strand pointer of the count-only call is NULL: an ntHash order is refused only where a strand is asked for)
        self._check(self.L.kmu_read_minimizers(*args, None, None, None, None, 0, _ptr(moff)[0], C.byref(total)))
        m = int(total.value)
        hashes = self._new_like(bases, max(m, 1), np.uint64, "int64")
        pos = self._new_like(bases, max(m, 1), np.uint32, "int32") if "pos" in want else None
        read = self._new_like(bases, max(m, 1), np.uint32, "int32") if "read" in want else None
        strand = self._new_like(bases, max(m, 1), np.uint8, "uint8") if "strand" in want else None
        if m or strand is not None:  # (with no minimizer at all the call still says whether a strand can be had)
            self._check(self.L.kmu_read_minimizers(*args, _ptr(hashes)[0], _ptr(pos)[0], _ptr(read)[0], _ptr(strand)[0], m, None,
                                                   C.byref(total)))
        return hashes[:m], (pos[:m] if pos is not None else None), (read[:m] if read is not None else None), \
            (strand[:m] if strand is not None else None), moff

    def read_syncmers(self, bases, offsets, kmer_type, k, fhash, s, t=0, s_kmer_type=None, s_fhash=None, want=MINIMIZERS_WANT):
        """kmu_read_syncmers: the (k, s, t) syncmers of every read -- the k-mers whose smallest s-mer value sits at offset t or
        k - s - t (t = 0: closed syncmers; 2 t == k - s: open syncmers at the middle offset; include/kmu.h has the rules).  The
        s-mers are ordered by (s_kmer_type, s, s_fhash); the type defaults to the reference's choice for s and the order to
        `fhash`.  Returns (hashes, pos, read, strand, sync_offsets) exactly as read_minimizers does, with the same `want`, the
        same dtypes and the same memory rule: numpy in gives numpy out, torch cuda tensors stay on the device.  Two library
        calls: one that counts, one with exactly that capacity."""
        unknown = [x for x in want if x not in MINIMIZERS_WANT]
        if unknown:
            raise ValueError("want holds %r: the optional outputs are %r" % (unknown, MINIMIZERS_WANT))
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        hp = A.HashParams(kmer_type, k, fhash, A.INPUT_ASCII, mem, 0)
        sp = A.SyncmerParams(A.kmer_type_for_k(s) if s_kmer_type is None else s_kmer_type, int(s), fhash if s_fhash is None else s_fhash, int(t))
        soff = self._new_like(bases, n + 1, np.uint64, "int64")
        total = C.c_uint64(0)
        ptr = self._ptrs(bases)  # (a batch of empty reads has no bases)
        args = (self.h, C.byref(hp), C.byref(sp), ptr(bases), _ptr(offsets)[0], n)
        self._check(self.L.kmu_read_syncmers(*args, None, None, None, None, 0, _ptr(soff)[0], C.byref(total)))
        m = int(total.value)
        hashes = self._new_like(bases, max(m, 1), np.uint64, "int64")
        pos = self._new_like(bases, max(m, 1), np.uint32, "int32") if "pos" in want else None
        read = self._new_like(bases, max(m, 1), np.uint32, "int32") if "read" in want else None
        strand = self._new_like(bases, max(m, 1), np.uint8, "uint8") if "strand" in want else None
        if m or strand is not None:  # (with no syncmer at all the call still says whether a strand can be had)
            self._check(self.L.kmu_read_syncmers(*args, _ptr(hashes)[0], _ptr(pos)[0], _ptr(read)[0], _ptr(strand)[0], m, None,
                                                 C.byref(total)))
        return hashes[:m], (pos[:m] if pos is not None else None), (read[:m] if read is not None else None), \
            (strand[:m] if strand is not None else None), soff

    def sketch_count(self, bases, offsets, params, counter=None, out=None):
        """kmu_sketch_count: the reads once, both results -- signature rows (returned) and, if `counter` is given, the
        k-mer counts of the same reads.  Host buffers (numpy / CPU torch tensors, best pinned): chunked upload overlapped
        with the kernels, rows downloaded under the count build.  Device buffers: both on the resident reads."""
        n = len(offsets) - 1
        mem = self._mem(bases, offsets)
        p = A.SketchParams.from_buffer_copy(params)
        p.mem = mem
        p.mode = A.MODE_PER_SEQ
        if out is None:
            if mem == A.MEM_DEVICE:
                import torch
                tdt = {A.SIG_U32: torch.int32, A.SIG_U64: torch.int64, A.SIG_F32: torch.float32,
                       A.SIG_F64: torch.float64, A.SIG_U16: torch.int16}[p.sig_type]
                out = torch.zeros((max(n, 1), p.sketch_size), dtype=tdt, device=bases.device)
            else:
                out = np.zeros((max(n, 1), p.sketch_size), dtype=A.SIG_NP[p.sig_type])
        self._check(self.L.kmu_sketch_count(self.h, C.byref(p), counter.h if counter is not None else None, _ptr(bases)[0],
                                            _ptr(offsets)[0], n, _ptr(out)[0]))
        return out[:n]

    def sketch_hashed(self, hashed, offsets, params, want_counts=False):
        """kmu_sketch_hashed: the caller evaluated fhash; `hashed` holds Kmer::Val values (uint32 / uint64) of
        sequence i in hashed[offsets[i]:offsets[i+1]]."""
        n = len(offsets) - 1
        mem = self._mem(hashed, offsets)
        p = A.SketchParams.from_buffer_copy(params)
        p.mem = mem
        m = p.sketch_size
        rows = 1 if p.mode == A.MODE_ALL_SEQS else n
        counts = None
        if mem == A.MEM_DEVICE:
            import torch
            tdt = {A.SIG_U32: torch.int32, A.SIG_U64: torch.int64, A.SIG_F32: torch.float32,
                   A.SIG_F64: torch.float64, A.SIG_U16: torch.int16}[p.sig_type]
            out = torch.zeros((max(rows, 1), m), dtype=tdt, device=hashed.device)
            if want_counts:
                counts = torch.zeros((max(rows, 1), m), dtype=torch.int32, device=hashed.device)
        else:
            out = np.zeros((max(rows, 1), m), dtype=A.SIG_NP[p.sig_type])
            if want_counts:
                counts = np.zeros((max(rows, 1), m), np.uint32)
        self._check(self.L.kmu_sketch_hashed(self.h, C.byref(p), _ptr(hashed)[0], _ptr(offsets)[0], n, _ptr(out)[0],
                                             _ptr(counts)[0]))
        return (out[:rows], counts[:rows]) if want_counts else out[:rows]

    # ---- one signature over several GPUs: partial slot minima + merge ----
    def _partial_buf(self, p, like, n_parts=1):
        words = int(self.L.kmu_sketch_partial_words(C.byref(p)))
        if like is not None and _is_torch(like) and like.is_cuda:
            import torch
            return torch.zeros((n_parts, words), dtype=torch.int64, device=like.device)
        return np.zeros((n_parts, words), np.uint64)

    def sketch_partial(self, bases, offsets, params, packed_offsets=None):
        """kmu_sketch_partial: per-slot minima of these sequences (one row of kmu_sketch_partial_words words)"""
        mem = self._mem(bases, offsets)
        p = A.SketchParams.from_buffer_copy(params)
        p.mem = mem
        out = self._partial_buf(p, bases)
        self._check(self.L.kmu_sketch_partial(self.h, C.byref(p), _ptr(bases)[0], _ptr(offsets)[0], _ptr(packed_offsets)[0],
                                              len(offsets) - 1, _ptr(out)[0]))
        return out[0]

    def sketch_hashed_partial(self, hashed, offsets, params):
        """kmu_sketch_hashed_partial: the same for caller-hashed values (disjoint key sets per rank for ProbMinHash)"""
        mem = self._mem(hashed, offsets)
        p = A.SketchParams.from_buffer_copy(params)
        p.mem = mem
        out = self._partial_buf(p, hashed)
        self._check(self.L.kmu_sketch_hashed_partial(self.h, C.byref(p), _ptr(hashed)[0], _ptr(offsets)[0], len(offsets) - 1,
                                                     _ptr(out)[0]))
        return out[0]

    def sketch_merge_partials(self, partials, params):
        """kmu_sketch_merge_partials: [n_parts, words] partial rows -> one signature row"""
        mem = self._mem(partials)
        p = A.SketchParams.from_buffer_copy(params)
        p.mem = mem
        m = p.sketch_size
        if mem == A.MEM_DEVICE:
            import torch
            tdt = {A.SIG_U32: torch.int32, A.SIG_U64: torch.int64, A.SIG_F32: torch.float32, A.SIG_F64: torch.float64,
                   A.SIG_U16: torch.int16}[p.sig_type]
            out = torch.zeros(m, dtype=tdt, device=partials.device)
        else:
            out = np.zeros(m, dtype=A.SIG_NP[p.sig_type])
        self._check(self.L.kmu_sketch_merge_partials(self.h, C.byref(p), _ptr(partials)[0], int(partials.shape[0]), _ptr(out)[0]))
        return out

    # ---- ingest (kmu_ingest.hip) ----
    def ingest_fasta(self, text, want_index=False):
        """kmu_ingest_fasta: like ingest_fastq for a FASTA text (multi-line records)"""
        return self.ingest_fastq(text, want_index, fn="kmu_ingest_fasta")

    def ingest_fastx(self, text, want_index=False):
        """kmu_ingest_fastx: FASTA or FASTQ by the first byte (needletail::parse_fastx_file)"""
        return self.ingest_fastq(text, want_index, fn="kmu_ingest_fastx")

    def ingest_fastq_qual(self, text, want_index=False):
        """kmu_ingest_fastq_qual: ingest_fastq that keeps the quality line -> (bases, quals, offsets, info[, record_index]);
        quals[offsets[i] + p] is the raw quality byte of base p of kept read i"""
        return self.ingest_fastq(text, want_index, fn="kmu_ingest_fastq_qual")

    def ingest_fastq(self, text, want_index=False, fn="kmu_ingest_fastq"):
        """kmu_ingest_fastq: FASTQ text (bytes / numpy uint8 on the host, torch uint8 tensor on the device) -> (bases,
        offsets, info[, record_index]) of the reads made of ACGTacgt only, in file order."""
        quals = fn == "kmu_ingest_fastq_qual"
        entry = getattr(self.L, fn)

        def call(text_p, bases, offs, idx, qual, info):
            """one call of the entry point; kmu_ingest_fastq_qual has quals_out and quals_cap behind bases_cap"""
            cap = 0 if bases is None else bases.shape[0]
            more = (_ptr(qual)[0], cap) if quals else ()
            return entry(self.h, text_p, n, mem, _ptr(bases)[0], cap, *more, _ptr(offs)[0], 0 if offs is None else offs.shape[0], _ptr(idx)[0],
                         C.byref(info))
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(bytes(text), np.uint8)
        dev = _is_torch(text) and text.is_cuda
        mem = A.MEM_DEVICE if dev else A.MEM_HOST
        n = int(text.shape[0])
        info = A.IngestInfo()
        self._check(call(_ptr(text)[0] if n else None, None, None, None, None, info))
        qual = self._new_like(text, max(int(info.kept_bases), 1), np.uint8, "uint8") if quals else None
        if dev:
            import torch
            bases = torch.zeros(max(int(info.kept_bases), 1), dtype=torch.uint8, device=text.device)
            offs = torch.zeros(int(info.n_kept) + 1, dtype=torch.int64, device=text.device)
            idx = torch.zeros(max(int(info.n_kept), 1), dtype=torch.int32, device=text.device) if want_index else None
        else:
            bases = np.zeros(max(int(info.kept_bases), 1), np.uint8)
            offs = np.zeros(int(info.n_kept) + 1, np.uint64)
            idx = np.zeros(max(int(info.n_kept), 1), np.uint32) if want_index else None
        info2 = A.IngestInfo()
        self._check(call(_ptr(text)[0] if n else None, bases, offs, idx, qual, info2))
        res = (bases[:int(info.kept_bases)],) + ((qual[:int(info.kept_bases)],) if quals else ()) + (offs, info2)
        return res + (idx[:int(info.n_kept)],) if want_index else res

    # ---- read statistics (kmu_read_stats.hip) ----
    def read_stats(self, bases, offsets, max_len=1000000, sig_digits=3, want=READ_STATS_WANT, into=None):
        """kmu_read_stats: the base composition of every read, the 101 x 4 table of base percentages, the length histogram in
        HdrHistogram's layout of (max_len, sig_digits) and the totals.  Returns (comp, pct_hist, len_hist, info); an output that
        `want` leaves out is None.  comp: A.READ_COMP_DTYPE records on the host, an int32 tensor [n, 12] holding the same bits
        on the device; pct_hist [101, 4] and len_hist [n_buckets]: uint64 (int64 tensors); info: a dict of A.READ_STATS_INFO.
        into=(comp, pct_hist, len_hist): arrays to fill instead of new ones (the call zeroes them itself)."""
        unknown = [w for w in want if w not in READ_STATS_WANT]
        if unknown:
            raise ValueError("want holds %r: the optional outputs are %r" % (unknown, READ_STATS_WANT))
        n_buckets, _ = len_hist_layout(max_len, sig_digits)
        mem = self._mem(bases)
        off = self._offsets_like(offsets, bases, mem)
        n = int(off.shape[0]) - 1
        if into is not None:
            comp, pct, hist = into
        else:
            comp = self._records(bases, n, A.READ_COMP_DTYPE) if "comp" in want else None
            pct = self._new_like(bases, (A.RS_PCT_ROWS, 4), np.uint64, "int64") if "pct" in want else None
            hist = self._new_like(bases, n_buckets, np.uint64, "int64") if "len" in want else None
        p, info = A.ReadStatsParams(sig_digits, 0, max_len), A.ReadStatsInfo()
        ptr = self._ptrs(bases)
        self._check(self.L.kmu_read_stats(self.h, C.byref(p), ptr(bases), _ptr(off)[0], n, mem, _ptr(comp)[0], _ptr(pct)[0], _ptr(hist)[0],
                                          C.byref(info)))
        info = {k: [int(x) for x in info.n_base] if k == "n_base" else int(getattr(info, k)) for k in A.READ_STATS_INFO}
        return (comp[:n] if comp is not None else None), pct, hist, info

    def quality_remap(self, quals, out=None):
        """kmu_quality_remap: the class (remap_quality8: 0 .. 7) of every quality byte; out=quals remaps in place"""
        mem = self._mem(quals)
        n = int(quals.shape[0])
        if out is None:
            out = self._new_like(quals, max(n, 1), np.uint8, "uint8")
        ptr = self._ptrs(quals)
        self._check(self.L.kmu_quality_remap(self.h, ptr(quals), n, mem, ptr(out, n)))
        return out[:n]

    def read_qual_stats(self, quals, offsets, want=READ_QUAL_WANT):
        """kmu_read_qual_stats: (records, class_hist) -- one A.READ_QUAL_DTYPE record per read (an int32 tensor [n, 20] holding
        the same bits on the device) and the bases of the batch per quality class, uint64 [8]; one not in `want` is None"""
        unknown = [w for w in want if w not in READ_QUAL_WANT]
        if unknown:
            raise ValueError("want holds %r: the optional outputs are %r" % (unknown, READ_QUAL_WANT))
        mem = self._mem(quals)
        off = self._offsets_like(offsets, quals, mem)
        n = int(off.shape[0]) - 1
        recs = self._records(quals, n, A.READ_QUAL_DTYPE) if "reads" in want else None
        hist = self._new_like(quals, A.RS_QUAL_CLASSES, np.uint64, "int64") if "hist" in want else None
        ptr = self._ptrs(quals)
        self._check(self.L.kmu_read_qual_stats(self.h, ptr(quals), _ptr(off)[0], n, mem, _ptr(recs)[0], _ptr(hist)[0]))
        return (recs[:n] if recs is not None else None), hist

    # ---- signature comparison (kmu_compare.hip) ----
    @staticmethod
    def _sig_type_of(sig):
        name = str(sig.dtype).replace("torch.", "")
        return {"uint32": A.SIG_U32, "int32": A.SIG_U32, "uint64": A.SIG_U64, "int64": A.SIG_U64, "float32": A.SIG_F32,
                "float64": A.SIG_F64}[name]

    def sig_equal_pairs(self, sig_a, sig_b, ia, ib):
        """kmu_sig_equal_pairs: number of equal slots of rows sig_a[ia[p]] and sig_b[ib[p]]."""
        mem = self._mem(sig_a, sig_b, ia, ib)
        n = int(ia.shape[0])
        out = self._new_like(sig_a, max(n, 1), np.uint32, "int32")
        self._check(self.L.kmu_sig_equal_pairs(self.h, _ptr(sig_a)[0], sig_a.shape[0], _ptr(sig_b)[0], sig_b.shape[0],
                                               sig_a.shape[1], self._sig_type_of(sig_a), _ptr(ia)[0], _ptr(ib)[0], n, mem,
                                               _ptr(out)[0]))
        return out[:n]

    def sig_equal_matrix(self, sig_a, sig_b):
        """kmu_sig_equal_matrix: equal-slot counts of every row of sig_a against every row of sig_b."""
        mem = self._mem(sig_a, sig_b)
        out = self._new_like(sig_a, (max(sig_a.shape[0], 1), max(sig_b.shape[0], 1)), np.uint16, "int16")
        # (the output stands in for a side without rows: it is there already, and the library reads no row through it)
        pa = _ptr(sig_a)[0] if sig_a.shape[0] else _ptr(out)[0]
        pb = _ptr(sig_b)[0] if sig_b.shape[0] else _ptr(out)[0]
        self._check(self.L.kmu_sig_equal_matrix(self.h, pa, sig_a.shape[0], pb, sig_b.shape[0],
                                                sig_a.shape[1], self._sig_type_of(sig_a), mem, _ptr(out)[0]))
        return out[:sig_a.shape[0], :sig_b.shape[0]]

    def sig_knn(self, sig_q, sig_db, k, group_q=None, group_db=None):
        """kmu_sig_knn: for every row of sig_q the k rows of sig_db with the most equal slots (ties: lower row first),
        rows of the query's own group left out.  Returns (idx uint32 [nq, k], eq uint16 [nq, k]); entries that do not
        exist are idx = KNN_NONE, eq = 0.  Device tensors in give device tensors out (int32 / int16 holding the same
        bits, like the other comparison calls)."""
        mem = self._mem(sig_q, sig_db, group_q, group_db)
        nq, ndb, k = int(sig_q.shape[0]), int(sig_db.shape[0]), int(k)
        if self._sig_type_of(sig_q) != self._sig_type_of(sig_db) or sig_q.shape[1] != sig_db.shape[1]:
            raise ValueError("query and database signatures differ in type or sketch size")
        idx = self._new_like(sig_q, (max(nq, 1), max(k, 1)), np.uint32, "int32")
        eq = self._new_like(sig_q, (max(nq, 1), max(k, 1)), np.uint16, "int16")
        # (as in sig_equal_matrix, an output stands in for a side without rows)
        pq = _ptr(sig_q)[0] if nq else _ptr(idx)[0]
        pdb = _ptr(sig_db)[0] if ndb else _ptr(idx)[0]
        self._check(self.L.kmu_sig_knn(self.h, pq, nq, pdb, ndb, sig_q.shape[1], self._sig_type_of(sig_q), k,
                                       _ptr(group_q)[0], _ptr(group_db)[0], mem, _ptr(idx)[0], _ptr(eq)[0]))
        return idx[:nq, :k], eq[:nq, :k]

    def minhash_distance_pairs(self, hashes_a, hashes_b, ia, ib):
        """kmu_minhash_distance_pairs on bottom-k rows: (common, total, i) per pair."""
        mem = self._mem(hashes_a, hashes_b, ia, ib)
        n = int(ia.shape[0])
        out = self._new_like(hashes_a, (max(n, 1), 3), np.uint32, "int32")
        self._check(self.L.kmu_minhash_distance_pairs(self.h, _ptr(hashes_a)[0], hashes_a.shape[0], _ptr(hashes_b)[0],
                                                      hashes_b.shape[0], hashes_a.shape[1], _ptr(ia)[0], _ptr(ib)[0], n,
                                                      mem, _ptr(out)[0]))
        return out[:n]

    def anchor_match(self, hashes_q, hashes_db, n_keys=1, min_common=1, group_q=None, group_db=None):
        """kmu_anchor_match: the pairs (row of hashes_q, row of hashes_db) of bottom-k rows that share one of their n_keys
        smallest hashes (rows of one group left out), with (common, total, i) of kmu_minhash_distance_pairs for each, kept when
        common >= min_common; ordered by query row, shared hash, database row.  Returns (pairs uint32 [n, 2], dist uint32
        [n, 3]); device tensors in give device tensors out (int32 holding the same bits).  Two library calls: one that counts,
        one with exactly that capacity."""
        mem = self._mem(hashes_q, hashes_db, group_q, group_db)
        nq, ndb = int(hashes_q.shape[0]), int(hashes_db.shape[0])
        if hashes_q.shape[1] != hashes_db.shape[1]:
            raise ValueError("query and database rows differ in length")
        m = int(hashes_q.shape[1])
        ptr = self._ptrs(hashes_q)
        args = (self.h, ptr(hashes_q), nq, ptr(hashes_db), ndb, m, int(n_keys), int(min_common), _ptr(group_q)[0], _ptr(group_db)[0], mem)
        return self._count_then_write(self.L.kmu_anchor_match, args, hashes_q)

    def _count_then_write(self, fn, args, like):
        """the call pair of anchor_match and AnchorIndex.match, fn(*args, pairs_out, dist_out, cap, n_out): (pairs [n, 2], dist
        [n, 3]) allocated where `like` lives"""
        (pairs, dist), n = self._two_calls(fn, args, lambda n: (self._new_like(like, (max(n, 1), 2), np.uint32, "int32"),
                                                                 self._new_like(like, (max(n, 1), 3), np.uint32, "int32")), n_out=2)
        return pairs[:n], dist[:n]

    def anchor_overlaps(self, pairs, dist, row_offsets_q, row_offsets_db=None, strands=2, band=1, min_score=1, upper=False):
        """kmu_anchor_overlaps: the read pairs behind the window pairs of anchor_match (pairs [n, 2], dist [n, 3] or None: every
        pair weighs 1), one record each -- the strand and first diagonal of the band of `band` + 1 diagonals with the largest
        weight, its score, votes and extent in slices of read a (include/kmu.h has the rules).  row_offsets_*: the layout arrays
        of the two sides (db defaults to q: a self-join); upper: only read_a < read_b.  numpy arrays give a structured array
        (A.OVERLAP_DTYPE); torch cuda tensors stay on the device and give an int32 tensor [n, 8] holding the same bits (offsets
        that are numpy arrays are copied up).  Two library calls: one that counts, one with exactly that capacity."""
        mem = self._mem(pairs, dist)
        n_pairs = int(pairs.shape[0])
        off_q, off_db = self._offsets_pair(row_offsets_q, row_offsets_q if row_offsets_db is None else row_offsets_db, pairs, mem)
        ptr = self._ptrs(pairs)
        args = (self.h, ptr(pairs), _ptr(dist)[0], n_pairs, _ptr(off_q)[0], int(off_q.shape[0]) - 1,
                _ptr(off_db)[0], int(off_db.shape[0]) - 1, int(strands), int(band), int(min_score), A.OVL_UPPER if upper else 0, mem)
        (out,), n = self._two_calls(self.L.kmu_anchor_overlaps, args, lambda n: (self._records(pairs, n, A.OVERLAP_DTYPE),))
        return out[:n]

    def seed_chains(self, pairs, q, db, span, max_gap, band, min_seeds=1, min_score=0, max_pos=0, upper=False):
        """kmu_seed_chains: one colinear chain of seeds per read pair behind the entry pairs of minimizer.seed_pairs (pairs [n, 2]:
        an entry of q, an entry of db, in any order) -- its strand, score, seed count and its start and end on both reads in
        bases (include/kmu.h has the rules).  q, db: Minimizers records (pos, read, strand or None, offsets with one entry per
        read and one more); db=None is the self-join.  span: the k of the minimizers; max_pos: 0, or a promise that no position is
        above it; upper: only read_a < read_b.  numpy arrays give a structured array (A.CHAIN_DTYPE); torch cuda tensors stay on
        the device and give an int32 tensor [n, 10] holding the same bits.  Two library calls: one that counts, one with exactly
        that capacity."""
        return self._seed_chains(self.L.kmu_seed_chains, pairs, q, db, span, max_gap, band, min_seeds, min_score, max_pos, upper)

    def seed_chains_all(self, pairs, q, db, span, max_gap, band, min_seeds=1, min_score=0, max_pos=0, upper=False):
        """kmu_seed_chains_all: EVERY chain of every (read pair, strand) behind the same entry pairs -- the repeat copies, the parts
        of a chimeric read, both sides of a structural difference -- ordered by read_a, read_b, strand and end anchor
        (include/kmu.h has the rules).  Arguments, records and the two library calls are those of seed_chains."""
        return self._seed_chains(self.L.kmu_seed_chains_all, pairs, q, db, span, max_gap, band, min_seeds, min_score, max_pos, upper)

    def _seed_chains(self, entry, pairs, q, db, span, max_gap, band, min_seeds, min_score, max_pos, upper):
        """the one marshalling of both chaining entries"""
        if db is None:
            db = q
        mem = self._mem(pairs, q.pos, q.read, q.strand, db.pos, db.read, db.strand)
        n_pairs = int(pairs.shape[0])
        p = A.ChainParams(int(span), int(max_gap), int(band), int(min_seeds), int(min_score), int(max_pos), A.CHAIN_UPPER if upper else 0)
        ptr = self._ptrs(pairs)

        def side(m):
            n = int(m.pos.shape[0])  # the entries of a side: pos, read and strand have as many
            return ptr(m.pos), ptr(m.read), _ptr(m.strand)[0] if n else None, n, len(m.offsets) - 1
        args = (self.h, ptr(pairs), n_pairs, *side(q), *side(db), C.byref(p), mem)
        (out,), n = self._two_calls(entry, args, lambda n: (self._records(pairs, n, A.CHAIN_DTYPE),))
        return out[:n]

    def chain_rank(self, chains, n_reads_q, mask_permille=500):
        """kmu_chain_rank: for every chain its rank inside its query read (score descending), the chain it is secondary to
        (parent; itself for a primary) and, for a primary, the best score and the number of its secondaries (include/kmu.h has the
        rules).  chains: the records of seed_chains / seed_chains_all, the chains of one read_a together and read_a ascending;
        n_reads_q: the reads of the q batch; mask_permille: the share of the shorter query interval that has to be covered.
        numpy in (A.CHAIN_DTYPE) gives a structured A.CHAIN_RANK_DTYPE array; torch cuda tensors (the int32 [n, 10] records)
        stay on the device and give an int32 tensor [n, 4] holding the same bits."""
        if not _is_torch(chains):
            chains = np.ascontiguousarray(chains)
        mem = self._mem(chains)
        n = int(chains.shape[0])
        p = A.RankParams(int(mask_permille), 0)
        out = self._records(chains, n, A.CHAIN_RANK_DTYPE)
        ptr = self._ptrs(chains)
        self._check(self.L.kmu_chain_rank(self.h, ptr(chains), n, int(n_reads_q), C.byref(p), mem, _ptr(out)[0]))
        return out[:n]

    def chain_align(self, chains, bases_q, offsets_q, bases_db=None, offsets_db=None, band=64):
        """kmu_chain_align: for every chain record the banded global alignment of the two segments it names -- edit distance,
        matching columns, the diagonals of its band and the flags A.ALN_DONE / A.ALN_EXACT (include/kmu.h has the rules).  chains:
        the records of seed_chains; bases_* / offsets_*: the ASCII batches the chains' reads are numbered in (db=None: the
        self-join on one batch).  numpy in (a structured A.CHAIN_DTYPE array) gives a structured A.CHAIN_ALN_DTYPE array; torch
        cuda tensors (the int32 [n, 10] records) stay on the device and give an int32 tensor [n, 4] holding the same bits
        (offsets that are numpy arrays are copied up)."""
        bases_db, offsets_db = self._db_batch(bases_q, offsets_q, bases_db, offsets_db)
        if not _is_torch(chains):
            chains = np.ascontiguousarray(chains)
        mem = self._mem(chains, bases_q, bases_db)
        n = int(chains.shape[0])
        off_q, off_db = self._offsets_pair(offsets_q, offsets_db, chains, mem)
        p = A.AlignParams(int(band), 0)
        out = self._records(chains, n, A.CHAIN_ALN_DTYPE)
        ptr = self._ptrs(chains)
        self._check(self.L.kmu_chain_align(self.h, ptr(chains), n, ptr(bases_q), _ptr(off_q)[0], int(off_q.shape[0]) - 1, ptr(bases_db),
                                           _ptr(off_db)[0], int(off_db.shape[0]) - 1, C.byref(p), mem, _ptr(out)[0]))
        return out[:n]

    def chain_cigar(self, chains, bases_q, offsets_q, bases_db=None, offsets_db=None, band=64, max_trace_bytes=0, aln=None):
        """kmu_chain_cigar: the records of chain_align and, for every chain, the path of its alignment as CIGAR runs (include/kmu.h
        has the rules).  Returns (aln, ops, op_offsets): aln as chain_align returns it, with A.ALN_PATH set where the chain's runs
        were written; ops: uint32 runs, len << 4 | code (A.CIGAR_I / D / EQ / X), the runs of chain c being
        ops[op_offsets[c]:op_offsets[c + 1]], in path order along A; op_offsets: uint64 [n + 1].  numpy in gives numpy out; torch
        cuda tensors stay on the device (ops int32 and op_offsets int64 holding the same bits).  max_trace_bytes: the workspace the
        direction bits of one batch of chains may take (0: A.CIGAR_TRACE_DEFAULT); a chain whose own bits need more gets its record
        without A.ALN_PATH and no runs.  aln: the records chain_align gave for the same chains at the same band -- ops is then sized
        by 2 edit + 1 runs per chain and the library is called once; without it twice: one call that counts, one that writes."""
        bases_db, offsets_db = self._db_batch(bases_q, offsets_q, bases_db, offsets_db)
        if not _is_torch(chains):
            chains = np.ascontiguousarray(chains)
        mem = self._mem(chains, bases_q, bases_db)
        n = int(chains.shape[0])
        off_q, off_db = self._offsets_pair(offsets_q, offsets_db, chains, mem)
        p = A.CigarParams(int(band), 0, int(max_trace_bytes))
        out = self._records(chains, n, A.CHAIN_ALN_DTYPE)
        op_off = self._new_like(chains, n + 1, np.uint64, "int64")
        ptr = self._ptrs(chains)
        args = (self.h, ptr(chains), n, ptr(bases_q), _ptr(off_q)[0], int(off_q.shape[0]) - 1, ptr(bases_db), _ptr(off_db)[0],
                int(off_db.shape[0]) - 1, C.byref(p), mem, _ptr(out)[0], _ptr(op_off)[0])

        def runs(cap):
            return (self._new_like(chains, max(cap, 1), np.uint32, "int32"),)
        if aln is None:
            (ops,), total = self._two_calls(self.L.kmu_chain_cigar, args, runs)
        else:  # one call: at most 2 edit + 1 runs for a chain that was aligned, none for the others
            rec = aln.cpu().numpy().view(np.uint32).reshape(-1, 4) if _is_torch(aln) else np.asarray(aln).view(np.uint32).reshape(-1, 4)
            if rec.shape[0] != n:
                raise ValueError("aln holds %d records for %d chains" % (rec.shape[0], n))
            done = (rec[:, 3] & A.ALN_DONE) != 0
            cap, written = int((2 * rec[done, 0].astype(np.int64) + 1).sum()), C.c_uint64(0)
            ops, = runs(cap)
            self._check(self.L.kmu_chain_cigar(*args, _ptr(ops)[0], cap, C.byref(written)))
            total = int(written.value)
        return out[:n], ops[:total], op_off

    def chain_pileup(self, chains, aln, ops, op_offsets, bases_q, offsets_q, bases_db=None, offsets_db=None, sides=A.PILE_Q | A.PILE_DB,
                     into=None):
        """kmu_chain_pileup: the votes of every chain's runs onto the bases of both reads (include/kmu.h has the rules).  chains, aln,
        ops, op_offsets: the records given to chain_cigar and what it returned; bases_* / offsets_*: the same batches (db=None: the
        self-join).  Returns (pile_q, pile_db): uint32 [n_bases, A.PILE_COLS] tables, one row per base, columns A.PILE_A ..
        A.PILE_ENDS; numpy in gives numpy out, torch cuda tensors stay on the device (int32 holding the same bits).  In the
        self-join both names are the same array, so every read collects the votes of all its partners; the table of a side that
        `sides` (A.PILE_Q, A.PILE_DB) leaves out is None.  into=(pile_q, pile_db), or one table for the self-join: tables to
        accumulate into; otherwise they are allocated here, zeroed."""
        own = bases_db is None
        bases_db, offsets_db = self._db_batch(bases_q, offsets_q, bases_db, offsets_db)
        chains, aln, mem, n = self._runs_of_chains(chains, aln, ops, op_offsets, bases_q, bases_db)
        off_q, off_db = self._offsets_pair(offsets_q, offsets_db, chains, mem)
        sides = int(sides)
        pile_q, pile_db = self._side_tables(chains, sides, own, into, lambda: int(off_q[-1]), lambda: int(off_db[-1]), A.PILE_COLS)
        p = A.PileupParams(sides)
        ptr = self._ptrs(chains)
        self._check(self.L.kmu_chain_pileup(self.h, ptr(chains), n, ptr(aln), _ptr(op_offsets)[0], ptr(ops), int(ops.shape[0]), ptr(bases_q),
                                            _ptr(off_q)[0], int(off_q.shape[0]) - 1, ptr(bases_db), _ptr(off_db)[0], int(off_db.shape[0]) - 1,
                                            C.byref(p), mem, ptr(pile_q) if sides & A.PILE_Q else None,
                                            ptr(pile_db) if sides & A.PILE_DB else None))
        return pile_q, pile_db

    def pile_call(self, pile, bases, offsets, min_depth=3, want=PILE_CALL_WANT):
        """kmu_pile_call: from a table of chain_pileup and the batch it belongs to, the call of every base -- uint8 [n_bases]: the code
        A.PILE_A .. A.PILE_DEL with the largest count (A.CALL_NONE below min_depth) and the bits A.CALL_INS and A.CALL_DIFF -- and the
        summary of every read (A.READ_PILE_DTYPE records; for torch an int32 tensor [n_reads, 8] holding the same bits).  Returns
        (call, reads); `want` names the outputs to compute ("call", "reads"), the other is None."""
        unknown = [w for w in want if w not in PILE_CALL_WANT]
        if unknown or not want:
            raise ValueError("want holds %r: the outputs are %r, at least one" % (list(want), PILE_CALL_WANT))
        mem = self._mem(pile, bases)
        off = self._offsets_like(offsets, pile, mem)
        n_reads = int(off.shape[0]) - 1
        n_bases = int(off[-1])
        if int(pile.shape[0]) != n_bases or int(bases.shape[0]) != n_bases:
            raise ValueError("the batch has %d bases: the table and the bases must have as many rows" % n_bases)
        call = self._new_like(pile, max(n_bases, 1), np.uint8, "uint8") if "call" in want else None
        reads = self._records(pile, n_reads, A.READ_PILE_DTYPE) if "reads" in want else None
        p = A.PileCallParams(int(min_depth), 0)
        ptr = self._ptrs(pile)
        self._check(self.L.kmu_pile_call(self.h, ptr(pile), ptr(bases), _ptr(off)[0], n_reads, C.byref(p), mem, _ptr(call)[0], _ptr(reads)[0]))
        return (call[:n_bases] if call is not None else None), (reads[:n_reads] if reads is not None else None)

    def pile_ins_plan(self, pile, call, max_ins=16):
        """kmu_pile_ins_plan: how many insertion slots every base of a batch gets, from its table (chain_pileup) and its calls
        (pile_call): 0 without A.CALL_INS, otherwise min(max_ins, (2 INS_BASES - 1) // depth).  Returns (ins_len, n_slots): uint8
        [n_bases] where the table lives, and the sum as an int.  Slot s of row g has the index S(g) + s, S being the exclusive
        prefix sum of ins_len."""
        mem = self._mem(pile, call)
        n_bases = int(pile.shape[0])
        if int(call.shape[0]) != n_bases:
            raise ValueError("the table has %d rows: call must have as many bytes" % n_bases)
        ins_len = self._new_like(pile, max(n_bases, 1), np.uint8, "uint8")
        p = A.InsPlanParams(int(max_ins), 0)
        ptr, total = self._ptrs(pile), C.c_uint64(0)
        self._check(self.L.kmu_pile_ins_plan(self.h, ptr(pile), ptr(call), n_bases, C.byref(p), mem, _ptr(ins_len)[0], C.byref(total)))
        return ins_len[:n_bases], int(total.value)

    def chain_pile_ins(self, chains, aln, ops, op_offsets, bases_q, offsets_q, ins_len_q, n_slots_q, bases_db=None, offsets_db=None,
                       ins_len_db=None, n_slots_db=None, sides=A.PILE_Q | A.PILE_DB, into=None):
        """kmu_chain_pile_ins: the letters of every chain's gap runs, voted into the insertion slots of both reads (include/kmu.h has
        the rules).  chains .. offsets_*: as chain_pileup takes them; ins_len_* / n_slots_*: what pile_ins_plan gave for each batch
        (db=None: the self-join, one plan).  Returns (ins_q, ins_db): uint32 [n_slots, A.INS_COLS] tables, one count per letter of
        every slot (int32 holding the same bits for torch); in the self-join both names are the same array; the table of a side
        that `sides` leaves out is None.  into=(ins_q, ins_db), or one table for the self-join: tables to accumulate into;
        otherwise they are allocated here, zeroed."""
        own = bases_db is None
        bases_db, offsets_db = self._db_batch(bases_q, offsets_q, bases_db, offsets_db)
        if own:
            ins_len_db, n_slots_db = ins_len_q, n_slots_q
        sides = int(sides)
        if (sides & A.PILE_Q and ins_len_q is None) or (sides & A.PILE_DB and ins_len_db is None):
            raise ValueError("a side that is asked for needs its ins_len and n_slots")
        chains, aln, mem, n = self._runs_of_chains(chains, aln, ops, op_offsets, bases_q, bases_db, ins_len_q, ins_len_db)
        off_q, off_db = self._offsets_pair(offsets_q, offsets_db, chains, mem)
        n_slots_q, n_slots_db = int(n_slots_q or 0), int(n_slots_db or 0)
        ins_q, ins_db = self._side_tables(chains, sides, own, into, n_slots_q, n_slots_db, A.INS_COLS)
        p = A.PileupParams(sides)
        ptr, spare = self._ptrs(chains), self._ptrs(chains)  # two empty tables are still two tables: a placeholder each
        q, db = bool(sides & A.PILE_Q), bool(sides & A.PILE_DB)

        def table(x):
            return (ptr if x is ins_q else spare)(x)
        self._check(self.L.kmu_chain_pile_ins(self.h, ptr(chains), n, ptr(aln), _ptr(op_offsets)[0], ptr(ops), int(ops.shape[0]), ptr(bases_q),
                                              _ptr(off_q)[0], int(off_q.shape[0]) - 1, ptr(bases_db), _ptr(off_db)[0], int(off_db.shape[0]) - 1,
                                              C.byref(p), mem, ptr(ins_len_q) if q else None, n_slots_q, table(ins_q) if q else None,
                                              ptr(ins_len_db) if db else None, n_slots_db, table(ins_db) if db else None))
        return ins_q, ins_db

    def _consensus_inputs(self, pile, call, ins_len, n_slots, ins, bases, offsets, *more):
        """the checks pile_consensus and pile_consensus_pos share, `more` being further arrays of the call: (the offsets where the
        arrays live, n_reads, n_bases, n_slots, mem)"""
        mem = self._mem(pile, call, ins_len, ins, bases, *more)
        off = self._offsets_like(offsets, pile, mem)
        n_bases = int(off[-1])
        if any(int(x.shape[0]) != n_bases for x in (pile, call, ins_len, bases)):
            raise ValueError("the batch has %d bases: the table, call, ins_len and the bases must have as many rows" % n_bases)
        n_slots = int(n_slots)
        if int(ins.shape[0]) != n_slots:
            raise ValueError("ins has %d slots, not n_slots = %d" % (int(ins.shape[0]), n_slots))
        return off, int(off.shape[0]) - 1, n_bases, n_slots, mem

    def pile_consensus(self, pile, call, ins_len, n_slots, ins, bases, offsets):
        """kmu_pile_consensus: the corrected reads of a batch -- per base the called letter (the read's own byte where there is no
        call, nothing for a DEL call) and then the emitted insertion slots.  pile, call: of chain_pileup and pile_call; ins_len,
        n_slots: of pile_ins_plan; ins: of chain_pile_ins.  Returns (cons_bases, cons_offsets): a new ASCII batch, uint8 and uint64
        [n_reads + 1] (int64 holding the same bits for torch), where the arrays live.  A row gives at most one byte and its slots, so
        the output is sized by n_bases + n_slots and the library is called once."""
        off, n_reads, n_bases, n_slots, mem = self._consensus_inputs(pile, call, ins_len, n_slots, ins, bases, offsets)
        cons_off = self._new_like(pile, n_reads + 1, np.uint64, "int64")
        cap = n_bases + n_slots
        cons = self._new_like(pile, max(cap, 1), np.uint8, "uint8")
        p, ptr, total = A.ConsensusParams(0), self._ptrs(pile), C.c_uint64(0)
        self._check(self.L.kmu_pile_consensus(self.h, ptr(pile), ptr(call), ptr(ins_len), n_slots, ptr(ins), ptr(bases), _ptr(off)[0], n_reads,
                                              C.byref(p), mem, _ptr(cons_off)[0], _ptr(cons)[0], cap, C.byref(total)))
        return cons[:int(total.value)], cons_off

    def pile_segments(self, pile, offsets, min_depth=3, min_span=None, min_len=1, longest=False):
        """kmu_pile_segments: the supported segments of every read of a batch from its table (chain_pileup) -- maximal runs of rows
        with depth >= min_depth in which consecutive rows are linked (max(depth - ENDS) of the two >= min_span; None: min_depth; 0:
        depth only), kept from min_len rows on -- and a summary with a class A.TRIM_* per read.  Returns (segs, seg_offsets, reads):
        A.PILE_SEG_DTYPE records in (read, start) order, uint64 [n_reads + 1], and A.READ_TRIM_DTYPE records; for torch int32
        tensors [n, 4] and [n_reads, 8] and int64 offsets holding the same bits.  longest=True lists only the longest kept segment
        of every read.  Kept segments are disjoint and at least min_len long, so the output is sized by n_bases // min_len and the
        library is called once."""
        mem = self._mem(pile)
        off = self._offsets_like(offsets, pile, mem)
        n_reads = int(off.shape[0]) - 1
        n_bases = int(off[-1])
        if int(pile.shape[0]) != n_bases:
            raise ValueError("the batch has %d bases: the table must have as many rows" % n_bases)
        min_span = int(min_depth if min_span is None else min_span)
        cap = min(n_bases // max(int(min_len), 1), n_reads if longest else n_bases)
        seg_off = self._new_like(pile, n_reads + 1, np.uint64, "int64")
        segs, reads = self._records(pile, cap, A.PILE_SEG_DTYPE), self._records(pile, n_reads, A.READ_TRIM_DTYPE)
        p = A.PileSegParams(int(min_depth), min_span, int(min_len), A.SEG_LONGEST if longest else 0)
        ptr, total = self._ptrs(pile), C.c_uint64(0)
        self._check(self.L.kmu_pile_segments(self.h, ptr(pile), _ptr(off)[0], n_reads, C.byref(p), mem,
                                             _ptr(seg_off)[0], _ptr(segs)[0], cap, C.byref(total), _ptr(reads)[0]))
        return segs[:int(total.value)], seg_off, reads[:n_reads]

    def extract_ranges(self, bases, begin, end):
        """kmu_extract_ranges: a new batch whose read i is bases[begin[i]:end[i]], verbatim.  Ranges may be empty, overlap, repeat
        and come in any order; a range with begin > end or end > len(bases) is refused (KmuError, A.E_UNSUPPORTED).  Returns
        (out_bases, out_offsets): uint8 and uint64 [n_ranges + 1] (int64 holding the same bits for torch), where the arrays
        live.  The library is called twice: for the total, then for the bytes."""
        mem = self._mem(bases, begin, end)
        n = int(begin.shape[0])
        if int(end.shape[0]) != n:
            raise ValueError("%d begins need as many ends" % n)
        if not _is_torch(begin):
            begin, end = (np.ascontiguousarray(np.asarray(x).astype(np.uint64)) for x in (begin, end))
        n_bases = int(bases.shape[0])
        out_off = self._new_like(bases, n + 1, np.uint64, "int64")
        ptr = self._ptrs(bases)
        args = (self.h, ptr(bases), n_bases, ptr(begin), ptr(end), n, mem, _ptr(out_off)[0])
        (out,), cap = self._two_calls(self.L.kmu_extract_ranges, args, lambda cap: (self._new_like(bases, max(cap, 1), np.uint8, "uint8"),))
        return out[:cap], out_off

    def pile_consensus_pos(self, pile, call, ins_len, n_slots, ins, bases, offsets, rows):
        """kmu_pile_consensus_pos: where raw rows land in the corrected batch -- pos[i] is the number of consensus bytes that the
        rows before row rows[i] of the batch produce (rows[i] == n_bases: the total), from the inputs of pile_consensus.  rows =
        offsets gives the cons_offsets of pile_consensus.  Returns pos: uint64 like rows (int64 for torch), where the arrays live."""
        off, n_reads, n_bases, n_slots, mem = self._consensus_inputs(pile, call, ins_len, n_slots, ins, bases, offsets, rows)
        if not _is_torch(rows):
            rows = np.ascontiguousarray(np.asarray(rows).astype(np.uint64))
        n = int(rows.shape[0])
        pos = self._new_like(pile, max(n, 1), np.uint64, "int64")
        p, ptr = A.ConsensusParams(0), self._ptrs(pile)
        self._check(self.L.kmu_pile_consensus_pos(self.h, ptr(pile), ptr(call), ptr(ins_len), n_slots, ptr(ins), ptr(bases), _ptr(off)[0], n_reads,
                                                  C.byref(p), mem, ptr(rows), n, _ptr(pos)[0]))
        return pos[:n]

    def _sg_inputs(self, chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz):
        """what sg_classify and sg_graph hand to the library: (the arguments up to `mem`, the arrays behind them -- the chains first,
        which the outputs are allocated like; they must outlive the call -- mem, n, n_reads)"""
        if not _is_torch(chains):
            chains = np.ascontiguousarray(chains)
        if aln is not None and not _is_torch(aln):
            aln = np.ascontiguousarray(aln)
        mem = self._mem(chains, aln)
        n = int(chains.shape[0])
        if aln is not None and int(aln.shape[0]) != n:
            raise ValueError("%d chains need as many alignment records" % n)
        off = self._offsets_like(offsets, chains, mem)
        n_reads = int(off.shape[0]) - 1
        p = A.SgParams(int(min_overlap), int(max_hang), int(int_permille), int(min_identity_permille), int(fuzz), 0)
        ptr = self._ptrs(chains)
        args = (self.h, ptr(chains), _ptr(aln if n else None)[0], n, _ptr(off)[0], n_reads, C.byref(p), mem)
        return args, (chains, aln, off, p, ptr), mem, n, n_reads

    def sg_classify(self, chains, aln, offsets, min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=0, fuzz=10):
        """kmu_sg_classify: the class of every chain record of a self-join (A.SG_SKIP .. A.SG_DOVETAIL; include/kmu.h has the rules)
        and a summary per read -- A.SG_READ_CONTAINED and the number of its records that are not SKIP.  chains: the records of
        seed_chains; aln: the records of chain_align for them, or None (no identity test); offsets: the batch's, of which only the
        lengths count.  Returns (classes, reads): uint8 [n] and A.SG_READ_DTYPE records; for torch cuda tensors a uint8 tensor and
        an int32 tensor [n_reads, 4] holding the same bits, on the device."""
        args, keep, mem, n, n_reads = self._sg_inputs(chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz)
        like = keep[0]
        classes = self._new_like(like, max(n, 1), np.uint8, "uint8")
        reads = self._records(like, n_reads, A.SG_READ_DTYPE)
        self._check(self.L.kmu_sg_classify(*args, _ptr(classes)[0], _ptr(reads)[0]))
        return classes[:n], reads[:n_reads]

    def sg_graph(self, chains, aln, offsets, min_overlap=500, max_hang=1000, int_permille=250, min_identity_permille=0, fuzz=10):
        """kmu_sg_graph: the string graph of a self-join -- two arcs per dovetail record between reads that are not contained, in
        (from, to, rec) order, transitively reduced: A.SG_ARC_REDUCED in an arc's flags, and unique = 1 where an arc and its mate
        are the only surviving arcs of their vertices (include/kmu.h has the rules).  Arguments as sg_classify.  Returns (arcs,
        arc_offsets, classes, reads): A.SG_ARC_DTYPE records, uint64 [2 n_reads + 1] (vertex 2r is read r forward, 2r + 1 its
        reverse complement), and what sg_classify returns with the surviving out-degrees filled in; for torch cuda tensors int32
        [n, 8], int64, uint8 and int32 [n_reads, 4] tensors holding the same bits, on the device.  Two library calls: one that
        counts, one with exactly that capacity."""
        args, keep, mem, n, n_reads = self._sg_inputs(chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz)
        like = keep[0]
        (classes, reads, arcs, arc_off), cap = self._two_calls(self.L.kmu_sg_graph, args, lambda cap: (
            self._new_like(like, max(n, 1), np.uint8, "uint8"), self._records(like, n_reads, A.SG_READ_DTYPE),
            self._records(like, cap, A.SG_ARC_DTYPE), self._new_like(like, 2 * n_reads + 1, np.uint64, "int64")), n_out=4, cap_at=3, always=True)
        return arcs[:cap], arc_off, classes[:n], reads[:n_reads]

    def sg_unitigs(self, arcs, reads, offsets):
        """kmu_sg_unitigs: the unitigs of a string graph as ordered paths of reads -- the arcs whose `unique` is 1 are the links,
        every read that is not contained lies on exactly one unitig, a circular one starts at its smallest read (include/kmu.h has
        the rules).  arcs: the records of sg_graph, in any order; reads: its summaries, or None (no read is contained); offsets: the
        batch's, of which only the lengths count.  Returns (unitigs, path, place): A.SG_UNITIG_DTYPE records numbered by their
        smallest read, A.SG_STEP_DTYPE records (unitig u's are path[first : first + n_reads]) and A.SG_PLACE_DTYPE records, one per
        read; for torch cuda tensors int32 [n, 8], [n_steps, 4] and [n_reads, 4] tensors holding the same bits, on the device.  One
        library call: both counts are at most n_reads."""
        if not _is_torch(arcs):
            arcs = np.ascontiguousarray(arcs)
        if reads is not None and not _is_torch(reads):
            reads = np.ascontiguousarray(reads)
        mem = self._mem(arcs, reads)
        n = int(arcs.shape[0])
        off = self._offsets_like(offsets, arcs, mem)
        n_reads = int(off.shape[0]) - 1
        if reads is not None and int(reads.shape[0]) != n_reads:
            raise ValueError("%d reads need as many summaries" % n_reads)
        unitigs, path, place = (self._records(arcs, n_reads, dt) for dt in (A.SG_UNITIG_DTYPE, A.SG_STEP_DTYPE, A.SG_PLACE_DTYPE))
        ptr, n_steps, total = self._ptrs(arcs), C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.kmu_sg_unitigs(self.h, ptr(arcs), n, _ptr(reads if n_reads else None)[0], _ptr(off)[0], n_reads, mem,
                                          _ptr(unitigs)[0], _ptr(path)[0], _ptr(place)[0], C.byref(n_steps), C.byref(total)))
        return unitigs[:int(total.value)], path[:int(n_steps.value)], place[:n_reads]

    def sg_clean(self, arcs, reads, n_reads, max_tip_reads=4, max_bubble_reads=8):
        """kmu_sg_clean: one round of graph cleaning on the arcs of sg_graph (or of an earlier sg_clean) -- dead ends of at most
        max_tip_reads reads are removed, simple bubbles whose branches hold at most max_bubble_reads reads are popped (0 turns a
        phase off), `unique` and the degrees are recomputed (include/kmu.h has the rules).  arcs: the records, sorted by `from`;
        reads: the summaries, or None.  Returns (arcs, reads, stats): new arrays with A.SG_ARC_TIP / A.SG_ARC_BUBBLE in the flags of
        the removed arcs and A.SG_READ_TIP / A.SG_READ_BUBBLE in those of the removed reads, and a dict of the A.SG_CLEAN_STATS
        counts; for torch cuda tensors int32 [n, 8] and [n_reads, 4] tensors holding the same bits, on the device."""
        if not _is_torch(arcs):
            arcs = np.ascontiguousarray(arcs)
        if reads is not None and not _is_torch(reads):
            reads = np.ascontiguousarray(reads)
        mem = self._mem(arcs, reads)
        n, n_reads = int(arcs.shape[0]), int(n_reads)
        if reads is not None and int(reads.shape[0]) != n_reads:
            raise ValueError("%d reads need as many summaries" % n_reads)
        arcs_out, reads_out = self._records(arcs, n, A.SG_ARC_DTYPE), self._records(arcs, n_reads, A.SG_READ_DTYPE)
        p, stats, ptr = A.SgCleanParams(int(max_tip_reads), int(max_bubble_reads), 0, 0), A.SgCleanStats(), self._ptrs(arcs)
        self._check(self.L.kmu_sg_clean(self.h, ptr(arcs), n, _ptr(reads if n_reads else None)[0], n_reads, C.byref(p), mem,
                                        _ptr(arcs_out)[0], _ptr(reads_out)[0], C.byref(stats)))
        return arcs_out[:n], reads_out[:n_reads], {name: int(getattr(stats, name)) for name in A.SG_CLEAN_STATS}

    def sg_unitig_chains(self, unitigs, path, place, chains, classes, offsets):
        """kmu_sg_unitig_chains: one chain record per read saying where the read lies on which unitig -- from the layout for a read
        on a path, from its longest containment record projected through the container's place for a contained read whose
        container is on a path (include/kmu.h has the rules).  unitigs, path, place: the records of sg_unitigs; chains, classes:
        the self-join and the classes of sg_graph / sg_classify for it, or both None (then no contained read is placed); offsets:
        the batch's, of which only the lengths count.  Returns (records, stats): A.CHAIN_DTYPE records in ascending read id with
        read_a = the unitig (a read of the batch of sg_unitig_seqs) and read_b = the read, and a dict of the A.UM_STATS counts; for
        torch cuda tensors an int32 tensor [n, 10] holding the same bits, on the device."""
        if not _is_torch(unitigs):
            unitigs, path, place = np.ascontiguousarray(unitigs), np.ascontiguousarray(path), np.ascontiguousarray(place)
        if (chains is None) != (classes is None):
            raise ValueError("chains and classes come together")
        if chains is not None and not _is_torch(chains):
            chains, classes = np.ascontiguousarray(chains), np.ascontiguousarray(classes)
        mem = self._mem(unitigs, path, place, chains, classes)
        n, n_steps = int(unitigs.shape[0]), int(path.shape[0])
        n_chains = 0 if chains is None else int(chains.shape[0])
        if n_chains and int(classes.shape[0]) != n_chains:
            raise ValueError("%d chains need as many classes" % n_chains)
        off = self._offsets_like(offsets, place, mem)
        n_reads = int(off.shape[0]) - 1
        if int(place.shape[0]) != n_reads:
            raise ValueError("%d reads need as many places" % n_reads)
        out, ptr = self._records(place, n_reads, A.CHAIN_DTYPE), self._ptrs(place)
        p, stats, total = A.UmParams(0, 0), A.UmStats(), C.c_uint64(0)
        self._check(self.L.kmu_sg_unitig_chains(self.h, ptr(unitigs), n, ptr(path), n_steps, ptr(place), ptr(chains) if n_chains else None,
                                                ptr(classes) if n_chains else None, n_chains, _ptr(off)[0], n_reads, C.byref(p), mem,
                                                _ptr(out)[0], C.byref(stats), C.byref(total)))
        return out[:int(total.value)], {name: int(getattr(stats, name)) for name in A.UM_STATS}

    def sg_unitig_seqs(self, unitigs, path, bases, offsets):
        """kmu_sg_unitig_seqs: the bases of every unitig -- over its steps, the last end - previous end bytes of the read in the
        step's orientation; strand 1 is the reverse complement, which turns every byte that is not one of ACGTacgt into N.  unitigs,
        path: the records of sg_unitigs; bases, offsets: the batch.  Returns (seq, seq_offsets): uint8 and uint64 [n_unitigs + 1]
        (int64 holding the same bits for torch), where the arrays live.  The library is called twice: for the total, then for the
        bytes."""
        if not _is_torch(unitigs):
            unitigs, path = np.ascontiguousarray(unitigs), np.ascontiguousarray(path)
        mem = self._mem(unitigs, path, bases)
        n, n_steps = int(unitigs.shape[0]), int(path.shape[0])
        off = self._offsets_like(offsets, bases, mem)
        n_reads = int(off.shape[0]) - 1
        ptr = self._ptrs(bases)
        args = (self.h, ptr(unitigs), n, ptr(path), n_steps, ptr(bases), _ptr(off)[0], n_reads, mem)
        (seq_off, seq), cap = self._two_calls(self.L.kmu_sg_unitig_seqs, args, lambda cap: (
            self._new_like(bases, n + 1, np.uint64, "int64"), self._new_like(bases, max(cap, 1), np.uint8, "uint8")), n_out=2, always=True)
        return seq[:cap], seq_off

    def _components(self, call, like, n_nodes, want, count):
        """the outputs of kmu_components / kmu_components_knn allocated where `like` lives, call(*output pointers) run on them,
        and the named tuple"""
        unknown = [w for w in want if w not in COMPONENTS_WANT]
        if unknown:
            raise ValueError("want holds %r: the optional outputs are %r" % (unknown, COMPONENTS_WANT))
        n = int(n_nodes)
        label = self._new_like(like, max(n, 1), np.uint32, "int32")
        cluster, size, members = (self._new_like(like, max(n, 1), np.uint32, "int32") if w in want else None for w in COMPONENTS_WANT)
        total = C.c_uint32(0)
        self._check(call(_ptr(label)[0], _ptr(cluster)[0], _ptr(size)[0], _ptr(members)[0], C.byref(total) if count else None))
        n_comp = int(total.value) if count else None
        return Components(label[:n], cluster[:n] if cluster is not None else None,
                          size[:n_comp if count else n] if size is not None else None, members[:n] if members is not None else None, n_comp)

    def components(self, edges, n_nodes, weight_at=0, min_weight=0, want=COMPONENTS_WANT, count=True):
        """kmu_components: connected components of the undirected graph over nodes 0 .. n_nodes - 1 whose edges are the rows of
        `edges` -- a [n, stride] uint32 / int32 array (words 0 and 1 are the ends), or a structured A.OVERLAP_DTYPE array (stride
        8).  weight_at = 0: every edge counts; otherwise an edge counts iff its word weight_at is >= min_weight (4: the score of
        an overlap record, 5: its votes).  Self loops, edges that do not count and edges with an end >= n_nodes are skipped.
        Returns Components(label, cluster, size[:n_components], members, n_components); `want` names the optional outputs to
        compute ("cluster", "size", "members"), the others are None.  count=False leaves n_components None and `size` whole
        (n_nodes entries, 0 behind the last cluster): nothing crosses to the host, and an async_device context does not wait.
        numpy in gives numpy (uint32) out; torch cuda tensors stay on the device (int32 tensors holding the same bits)."""
        if not _is_torch(edges):
            edges = np.ascontiguousarray(edges)
            if edges.dtype.names is not None:
                if edges.dtype != np.dtype(A.OVERLAP_DTYPE):
                    raise ValueError("a structured edge array must be of A.OVERLAP_DTYPE")
                edges = edges.reshape(-1).view(np.uint32).reshape(-1, 8)
        if edges.ndim != 2 or edges.dtype.itemsize != 4 or str(edges.dtype).replace("torch.", "") not in ("uint32", "int32"):
            raise ValueError("edges must be a [n, stride] array of uint32 / int32 words")
        n_edges, stride = int(edges.shape[0]), int(edges.shape[1])
        mem = self._mem(edges)
        ptr = self._ptrs(edges)
        pe = ptr(edges)

        def call(*outs):
            return self.L.kmu_components(self.h, int(n_nodes), pe, n_edges, stride, int(weight_at), int(min_weight), mem, *outs)
        return self._components(call, edges, n_nodes, want, count)

    def components_knn(self, idx, eq, min_eq=0, want=COMPONENTS_WANT, count=True):
        """kmu_components_knn: the components of the neighbour lists of a sig_knn self-join (idx [n, k], eq [n, k] or None): node i
        is joined to idx[i, j] iff eq[i, j] >= min_eq; KNN_NONE entries join nothing.  Returns what `components` returns."""
        n, k = int(idx.shape[0]), int(idx.shape[1])
        mem = self._mem(idx, eq)
        if eq is not None and tuple(eq.shape) != (n, k):
            raise ValueError("idx and eq differ in shape")
        ptr = self._ptrs(idx)
        pi = ptr(idx, n * k)

        def call(*outs):
            return self.L.kmu_components_knn(self.h, n, pi, _ptr(eq)[0], k, int(min_eq), mem, *outs)
        return self._components(call, idx, n, want, count)

    def anchor_index(self, hashes_db, n_keys=1, group_db=None):
        """kmu_anchor_index_create: the database side of anchor_match as an object that stays on the device (AnchorIndex)"""
        return AnchorIndex(self, hashes_db, n_keys, group_db)

    def counter(self, kmer_type, k, counter_bits=8, capacity_hint=1 << 20, distributed=False, owner_hash=False, hint_occurrences=False):
        return Counter(self, kmer_type, k, counter_bits, capacity_hint, distributed, owner_hash, hint_occurrences)

    def kfilter(self, kmer_type, k, n_cells, n_hashes=4):
        """kmu_kfilter_create: the count prefilter (KFilter) of n_cells 16-byte cells; kfilter_cells_for sizes it"""
        return KFilter(self, kmer_type, k, n_cells, n_hashes)


class _Handle:
    """An object of the library that lives on a context: `ctx`, its entry points `L`, the handle `h` and `_destroy`, the name of the
    call that frees it.  Close it (or leave its `with` block) before its context; closing it afterwards, or twice, is silent."""
    _destroy = None

    def __init__(self, ctx):
        self.ctx, self.L, self.h = ctx, ctx.L, None

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            getattr(self.L, self._destroy)(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class AnchorIndex(_Handle):
    """kmu_anchor_index: ndb bottom-k rows (numpy, or a torch cuda tensor), their n_keys smallest hashes sorted into buckets, and
    optionally the group of every row, kept on the device: built once, matched against by any number of query batches, and the
    owner of the bucket sizes behind the repeat mask `max_occ` (include/kmu.h has the rules).  The index copies what it is given;
    close it before its context."""

    _destroy = "kmu_anchor_index_destroy"

    def __init__(self, ctx, hashes_db, n_keys=1, group_db=None):
        super().__init__(ctx)
        mem = ctx._mem(hashes_db, group_db)
        ndb, self.m = int(hashes_db.shape[0]), int(hashes_db.shape[1])
        ptr, h = ctx._ptrs(hashes_db), C.c_void_p()
        ctx._check(self.L.kmu_anchor_index_create(ctx.h, ptr(hashes_db), ndb, self.m, int(n_keys), _ptr(group_db)[0], mem, C.byref(h)))
        self.h = h

    def info(self):
        """kmu_anchor_index_info as a dict: ndb, m, n_keys, has_groups, n_entries, n_distinct, max_occupancy, device_bytes"""
        t = A.AnchorIndexInfo()
        self.ctx._check(self.L.kmu_anchor_index_info(self.h, C.byref(t)))
        return {k: int(getattr(t, k)) for k, _ in A.AnchorIndexInfo._fields_ if k != "pad"}

    def occupancy(self, n_bins):
        """kmu_anchor_index_occupancy: hist[c] = the distinct keys that c database rows carry, the last bin collecting every
        c >= n_bins - 1 (a numpy uint64 array: it feeds anchor.max_occ_for_fraction on the host)"""
        hist = np.zeros(int(n_bins), np.uint64)
        self.ctx._check(self.L.kmu_anchor_index_occupancy(self.h, _ptr(hist)[0], int(n_bins), A.MEM_HOST))
        return hist

    def match(self, hashes_q, group_q=None, min_common=1, max_occ=0):
        """kmu_anchor_index_match: anchor_match of hashes_q against the index's rows, seeded only by keys that at most max_occ
        database rows carry (0: no mask, the result of anchor_match).  Returns (pairs uint32 [n, 2], dist uint32 [n, 3]); device
        tensors in give device tensors out (int32 holding the same bits).  Two library calls, one that counts and one with exactly
        that capacity, on the one index."""
        ctx = self.ctx
        mem = ctx._mem(hashes_q, group_q)
        nq = int(hashes_q.shape[0])
        if int(hashes_q.shape[1]) != self.m:
            raise ValueError("query rows and the index's rows differ in length")
        ptr = ctx._ptrs(hashes_q)
        args = (self.h, ptr(hashes_q), nq, _ptr(group_q)[0], int(min_common), int(max_occ), mem)
        return ctx._count_then_write(self.L.kmu_anchor_index_match, args, hashes_q)


class Counter(_Handle):
    """kmu_counter: exact canonical k-mer multiplicities on the device (KmerCountT contract)."""
    _destroy = "kmu_count_destroy"

    def __init__(self, ctx, kmer_type, k, counter_bits=8, capacity_hint=1 << 20, distributed=False, owner_hash=False,
                 hint_occurrences=False):
        """hint_occurrences: capacity_hint counts k-mer occurrences; the first add sizes the table from the duplication it measures"""
        super().__init__(ctx)
        flags = ((A.COUNT_DISTRIBUTED if distributed else 0) | (A.COUNT_OWNER_HASH if owner_hash else 0)
                 | (A.COUNT_HINT_OCCURRENCES if hint_occurrences else 0))
        self.p = A.CountParams(kmer_type, k, counter_bits, flags, capacity_hint)
        h = C.c_void_p()
        ctx._check(self.L.kmu_count_create(ctx.h, C.byref(self.p), C.byref(h)))
        self.h = h

    def reset(self):
        self.ctx._check(self.L.kmu_count_reset(self.h))

    def finalize(self):
        """kmu_count_finalize (collective): afterwards this rank's counter holds the k-mers it owns, counted over all ranks"""
        self.ctx._check(self.L.kmu_count_finalize(self.h))

    def add_reads(self, bases, offsets, input_kind=A.INPUT_ASCII, packed_offsets=None):
        mem = Context._mem(bases, offsets)
        self.ctx._check(self.L.kmu_count_add_reads(self.h, _ptr(bases)[0], _ptr(offsets)[0], _ptr(packed_offsets)[0],
                                                   len(offsets) - 1, input_kind, mem))

    def add_kmers(self, canon):
        mem = Context._mem(canon)
        n = canon.numel() if _is_torch(canon) else canon.size
        self.ctx._check(self.L.kmu_count_add_kmers(self.h, _ptr(canon)[0], n, mem))

    def add_reads_filtered(self, kfilter, bases, offsets):
        """kmu_count_add_reads_filtered: the occurrences of the reads whose k-mer the prefilter puts in class 2 (may occur twice
        or more) go into the table; returns their number.  A failed call raises with `n_passed` on the exception."""
        mem = Context._mem(bases, offsets)
        n = C.c_uint64(0)
        try:
            self.ctx._check(self.L.kmu_count_add_reads_filtered(self.h, kfilter.h, _ptr(bases)[0], _ptr(offsets)[0], len(offsets) - 1, mem,
                                                                C.byref(n)))
        except KmuError as e:
            e.n_passed = n.value
            raise
        return n.value

    def query(self, canon):
        canon, n, mem = self.ctx._kmer_values(canon)
        out = self.ctx._new_like(canon, max(n, 1), np.uint32, "int32")
        self.ctx._check(self.L.kmu_count_query(self.h, _ptr(canon)[0], n, mem, _ptr(out)[0]))
        return out[:n]

    def nb_distinct(self):
        v = C.c_uint64(0)
        self.ctx._check(self.L.kmu_count_nb_distinct(self.h, C.byref(v)))
        return v.value

    def nb_unique(self):
        v = C.c_uint64(0)
        self.ctx._check(self.L.kmu_count_nb_unique(self.h, C.byref(v)))
        return v.value

    def table_info(self):
        """kmu_count_table_info: {nslots, table_bytes, bytes_per_slot, count_field_bits}"""
        ti = A.CountTableInfo()
        self.ctx._check(self.L.kmu_count_table_info(self.h, C.byref(ti)))
        return {"nslots": ti.nslots, "table_bytes": ti.table_bytes, "bytes_per_slot": ti.bytes_per_slot,
                "count_field_bits": ti.count_field_bits, "count_ceiling": ti.count_ceiling}

    def table_bytes(self):
        return self.table_info()["table_bytes"]

    def nb_saturated(self):
        """kmu_count_nb_saturated: k-mers whose in-table count reached the table's ceiling (nb_occurrences is then a lower bound)"""
        n = C.c_uint64(0)
        self.ctx._check(self.L.kmu_count_nb_saturated(self.h, C.byref(n)))
        return n.value

    def nb_occurrences(self):
        """kmu_count_nb_occurrences: sum of the multiplicities held (= k-mer occurrences inserted)"""
        v = C.c_uint64(0)
        self.ctx._check(self.L.kmu_count_nb_occurrences(self.h, C.byref(v)))
        return v.value

    def dump(self, min_count=2):
        (k, c), n = self.ctx._two_calls(self.L.kmu_count_dump, (self.h, min_count),
                                        lambda n: (np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)), n_out=2, always=True)
        return k[:n], c[:n]

    def eliminate_once(self):
        """kmu_count_eliminate_once: drop the k-mers seen once"""
        self.ctx._check(self.L.kmu_count_eliminate_once(self.h))

    def once_positions(self, bases, offsets):
        """kmu_count_once_positions: (canonical k-mers, numseq, numkmer) of the occurrences whose k-mer has count 1, in
        (sequence, position) order; numpy arrays for host input, torch cuda tensors for device input"""
        mem = Context._mem(bases, offsets)
        new, args = self.ctx._new_like, (self.h, _ptr(bases)[0], _ptr(offsets)[0], len(offsets) - 1, mem)
        (k, s, p), n = self.ctx._two_calls(self.L.kmu_count_once_positions, args, lambda n: (
            new(bases, max(n, 1), np.uint64, "int64"), new(bases, max(n, 1), np.uint32, "int32"), new(bases, max(n, 1), np.uint32, "int32")),
            n_out=3, always=True)
        return k[:n], s[:n], p[:n]

    def histogram(self, n_bins=None, device=None):
        """kmu_count_histogram: hist[v] = distinct k-mers whose reported count is v, the last bin collecting every count
        >= n_bins - 1 (default 2^counter_bits bins); a numpy uint64 array, or a torch int64 cuda tensor when device is given"""
        if n_bins is None:
            n_bins = 1 << self.p.counter_bits
        if device is not None:
            import torch
            h = torch.zeros(max(n_bins, 1), dtype=torch.int64, device=device)
            mem = A.MEM_DEVICE
        else:
            h = np.zeros(max(n_bins, 1), np.uint64)
            mem = A.MEM_HOST
        self.ctx._check(self.L.kmu_count_histogram(self.h, _ptr(h)[0], n_bins, mem))
        return h[:n_bins]

    def read_profile(self, bases, offsets, solid_min=2, want_counts=True, want_stats=True, counts_out=None):
        """kmu_count_read_profile: the reported count of the canonical k-mer at every k-mer start of every read, and one
        kmu_read_abundance record per read.  Returns (counts, stats), or the one asked for.
        counts: counts[offsets[i] + p] (the layout of kmer_hashes) -- a numpy uint16 array for host input, a torch int16 cuda
        tensor (the same bits) for device input; `counts_out` gives the array to fill instead of a new one of zeros.
        stats: a numpy array of A.READ_ABUNDANCE_DTYPE records for host input; for device input a torch uint8 cuda tensor
        [n_seq, 32] holding the same records (`.cpu().numpy().view(A.READ_ABUNDANCE_DTYPE).reshape(-1)`)."""
        mem = Context._mem(bases, offsets)
        nseq = len(offsets) - 1
        counts = stats = None
        if mem == A.MEM_DEVICE:
            import torch
            if want_counts:
                counts = counts_out if counts_out is not None else torch.zeros(max(int(offsets[-1].item()), 1), dtype=torch.int16,
                                                                               device=bases.device)
            if want_stats:
                stats = torch.zeros((max(nseq, 1), 32), dtype=torch.uint8, device=bases.device)
        else:
            if want_counts:
                counts = counts_out if counts_out is not None else np.zeros(max(int(offsets[-1]), 1), np.uint16)
            if want_stats:
                stats = np.zeros(max(nseq, 1), np.dtype(A.READ_ABUNDANCE_DTYPE))
        self.ctx._check(self.L.kmu_count_read_profile(self.h, _ptr(bases)[0], _ptr(offsets)[0], nseq, mem, solid_min,
                                                      _ptr(counts)[0], _ptr(stats)[0]))
        if stats is not None:
            stats = stats[:nseq]
        if want_counts and want_stats:
            return counts, stats
        return counts if want_counts else stats

    def export_part(self, part, n_parts, device=None):
        """entries owned by `part`: (kmers, counts) as numpy arrays, or torch cuda tensors when device is given"""
        n = C.c_uint64(0)
        self.ctx._check(self.L.kmu_count_export_part(self.h, part, n_parts, None, None, 0, A.MEM_HOST, C.byref(n)))
        if device is not None:
            import torch
            k = torch.zeros(max(n.value, 1), dtype=torch.int64, device=device)
            c = torch.zeros(max(n.value, 1), dtype=torch.int32, device=device)
            mem = A.MEM_DEVICE
        else:
            k = np.zeros(max(n.value, 1), np.uint64)
            c = np.zeros(max(n.value, 1), np.uint32)
            mem = A.MEM_HOST
        self.ctx._check(self.L.kmu_count_export_part(self.h, part, n_parts, _ptr(k)[0], _ptr(c)[0], n.value, mem,
                                                     C.byref(n)))
        return k[:n.value], c[:n.value]

    def extract_by_owner(self, bases, offsets, n_parts):
        """canonical k-mers of the reads grouped by owner rank.  Returns (kmers, bounds): `kmers` is a zero-copy view
        (torch int64 cuda tensor via __cuda_array_interface__) of a buffer owned by the context, valid until the next
        counter call; bounds[n_parts + 1] (numpy) delimits the groups."""
        import torch
        mem = Context._mem(bases, offsets)
        ptr = C.c_void_p()
        bounds = np.zeros(n_parts + 1, np.uint64)
        self.ctx._check(self.L.kmu_count_extract_by_owner(self.h, _ptr(bases)[0], _ptr(offsets)[0], len(offsets) - 1, mem,
                                                          n_parts, C.byref(ptr), _ptr(bounds)[0]))
        n = int(bounds[-1])

        class _Dev:  # CUDA array interface v2 over the library-owned buffer
            __cuda_array_interface__ = {"shape": (max(n, 1),), "typestr": "<i8", "data": (ptr.value, False), "version": 2}

        dev = bases.device if _is_torch(bases) else torch.device("cuda", self.ctx.device_id)
        t = torch.as_tensor(_Dev(), device=dev)
        return t[:n], bounds

    @property
    def owner_kind(self):
        """kmu_count_owner_kind: A.OWNER_MINIMIZER / A.OWNER_HASH"""
        return int(self.L.kmu_count_owner_kind(self.h))

    def extract_superkmers(self, bases, offsets, n_parts):
        """the k-mers of the reads as super-k-mer records grouped by minimizer owner.  Returns (records, bounds, kmers):
        `records` a zero-copy [n, 3] int32 view (torch cuda tensor) of a buffer owned by the context, valid until the next
        counter call; bounds[n_parts + 1] (numpy, in records); kmers[n_parts] the k-mers every group holds."""
        import torch
        mem = Context._mem(bases, offsets)
        ptr = C.c_void_p()
        bounds = np.zeros(n_parts + 1, np.uint64)
        kmers = np.zeros(n_parts, np.uint64)
        self.ctx._check(self.L.kmu_count_extract_superkmers(self.h, _ptr(bases)[0], _ptr(offsets)[0], len(offsets) - 1, mem, n_parts,
                                                            C.byref(ptr), _ptr(bounds)[0], _ptr(kmers)[0]))
        n = int(bounds[-1])

        class _Dev:  # CUDA array interface v2 over the library-owned buffer
            __cuda_array_interface__ = {"shape": (max(n, 1), 3), "typestr": "<i4", "data": (ptr.value, False), "version": 2}

        dev = bases.device if _is_torch(bases) else torch.device("cuda", self.ctx.device_id)
        t = torch.as_tensor(_Dev(), device=dev)
        return t[:n], bounds, kmers

    def add_superkmers(self, records):
        """kmu_count_add_superkmers: records as an [n, 3] int32 / uint32 array (numpy or torch cuda tensor)"""
        mem = Context._mem(records)
        n = (records.numel() if _is_torch(records) else records.size) // 3
        self.ctx._check(self.L.kmu_count_add_superkmers(self.h, _ptr(records)[0], n, mem))

    def merge_entries(self, kmers, counts):
        mem = Context._mem(kmers, counts)
        n = kmers.numel() if _is_torch(kmers) else kmers.size
        self.ctx._check(self.L.kmu_count_merge_entries(self.h, _ptr(kmers)[0], _ptr(counts)[0], n, mem))

    def retain_part(self, part, n_parts):
        self.ctx._check(self.L.kmu_count_retain_part(self.h, part, n_parts))


def len_hist_layout(max_len, sig_digits):
    """kmu_len_hist_layout (plain host code): (n_buckets, limit) of the length histogram of kmu_read_stats"""
    n, limit = C.c_uint32(), C.c_uint64()
    rc = load().kmu_len_hist_layout(int(max_len), int(sig_digits), C.byref(n), C.byref(limit))
    if rc != A.OK:
        raise KmuError(rc, "max_len must be positive and sig_digits in [1, 5]")
    return int(n.value), int(limit.value)


def len_bucket_range(sig_digits, bucket):
    """kmu_len_bucket_range (plain host code): the (lowest, highest) length of a bucket"""
    lo, hi = C.c_uint64(), C.c_uint64()
    rc = load().kmu_len_bucket_range(int(sig_digits), int(bucket), C.byref(lo), C.byref(hi))
    if rc != A.OK:
        raise KmuError(rc, "sig_digits must be in [1, 5]")
    return int(lo.value), int(hi.value)


def kfilter_cells_for(expected_distinct, bits_per_kmer=16):
    """kmu_kfilter_cells_for (plain host code): max(1, ceil(expected_distinct * bits_per_kmer / 64)) cells; 0 when that is more
    than a filter can have (2^32 - 1)"""
    return int(load().kmu_kfilter_cells_for(int(expected_distinct), int(bits_per_kmer)))


class KFilter(_Handle):
    """kmu_kfilter: the count prefilter -- n_cells cells {A, B} that tell the canonical k-mers added once (class 1) from those that
    may have been added twice or more (class 2); include/kmu.h has the structure.  Close it before its context."""
    _destroy = "kmu_kfilter_destroy"

    def __init__(self, ctx, kmer_type, k, n_cells, n_hashes=4):
        super().__init__(ctx)
        self.p = A.KFilterParams(kmer_type, k, n_hashes, 0, n_cells)
        h = C.c_void_p()
        ctx._check(self.L.kmu_kfilter_create(ctx.h, C.byref(self.p), C.byref(h)))
        self.h = h

    def reset(self):
        self.ctx._check(self.L.kmu_kfilter_reset(self.h))

    def add_reads(self, bases, offsets):
        """kmu_kfilter_add_reads: one occurrence of every canonical k-mer of every read (ASCII bases)"""
        mem = Context._mem(bases, offsets)
        self.ctx._check(self.L.kmu_kfilter_add_reads(self.h, _ptr(bases)[0], _ptr(offsets)[0], len(offsets) - 1, mem))

    def add_kmers(self, canon):
        mem = Context._mem(canon)
        n = canon.numel() if _is_torch(canon) else canon.size
        self.ctx._check(self.L.kmu_kfilter_add_kmers(self.h, _ptr(canon)[0], n, mem))

    def query(self, canon):
        """kmu_kfilter_query: the class (0 never added, 1 added once, 2 maybe more often) of every value; uint8"""
        canon, n, mem = self.ctx._kmer_values(canon)
        out = self.ctx._new_like(canon, max(n, 1), np.uint8, "uint8")
        self.ctx._check(self.L.kmu_kfilter_query(self.h, _ptr(canon)[0], n, mem, _ptr(out)[0]))
        return out[:n]

    def info(self):
        """kmu_kfilter_info as a dict: n_cells, bytes, n_hashes, kmer_size, n_added, bits_a, bits_b, est_distinct"""
        t = A.KFilterInfo()
        self.ctx._check(self.L.kmu_kfilter_info(self.h, C.byref(t)))
        return {k: (float(t.est_distinct) if k == "est_distinct" else int(getattr(t, k))) for k, _ in A.KFilterInfo._fields_}

    def export(self, device=None):
        """kmu_kfilter_export: the 2 * n_cells words A0 B0 A1 B1 ...; a numpy uint64 array, or a torch int64 cuda tensor when
        device is given"""
        n = 2 * int(self.p.n_cells)
        if device is not None:
            import torch
            out = torch.zeros(n, dtype=torch.int64, device=device)
            self.ctx._check(self.L.kmu_kfilter_export(self.h, _ptr(out)[0], A.MEM_DEVICE))
            return out
        out = np.zeros(n, np.uint64)
        self.ctx._check(self.L.kmu_kfilter_export(self.h, _ptr(out)[0], A.MEM_HOST))
        return out

    def merge(self, other):
        """kmu_kfilter_merge: this filter becomes the filter of both inputs (same context and parameters)"""
        self.ctx._check(self.L.kmu_kfilter_merge(self.h, other.h))

    def select_reads(self, bases, offsets):
        """kmu_kfilter_select_reads: the canonical k-mer of every class-2 occurrence of the reads, in (sequence, position) order;
        a numpy array for host input, a torch cuda tensor for device input.  Two library calls: the size, then the k-mers."""
        n = self.n_passing(bases, offsets)
        mem = Context._mem(bases, offsets)
        k = self.ctx._new_like(bases, max(n, 1), np.uint64, "int64")
        got = C.c_uint64(0)
        self.ctx._check(self.L.kmu_kfilter_select_reads(self.h, _ptr(bases)[0], _ptr(offsets)[0], len(offsets) - 1, mem, _ptr(k)[0], n,
                                                        C.byref(got)))
        return k[:got.value]

    def n_passing(self, bases, offsets):
        """the size query of kmu_kfilter_select_reads: how many k-mer occurrences of the reads are class 2"""
        mem = Context._mem(bases, offsets)
        n = C.c_uint64(0)
        self.ctx._check(self.L.kmu_kfilter_select_reads(self.h, _ptr(bases)[0], _ptr(offsets)[0], len(offsets) - 1, mem, None, 0, C.byref(n)))
        return n.value


def anchor_layout(offsets_host, window, overlap):
    """kmu_anchor_layout: row_offsets[n_seq + 1] of the anchors of reads given by host offsets (no device needed)"""
    L = load()
    off = np.ascontiguousarray(offsets_host, np.uint64)
    out = np.zeros(off.size, np.uint64)
    rc = L.kmu_anchor_layout(_ptr(off)[0], off.size - 1, window, overlap, _ptr(out)[0])
    if rc:
        raise KmuError(rc, "kmu_anchor_layout: window %d, overlap %d" % (window, overlap))
    return out


def minimizer_layout(offsets_host, k, w):
    """kmu_minimizer_layout: win_offsets[n_seq + 1], the windows of w k-mers of reads given by host offsets -- an upper bound of
    their minimizers, and a sufficient `cap` of kmu_read_minimizers (no device needed)"""
    L = load()
    off = np.ascontiguousarray(offsets_host, dtype=np.uint64)
    out = np.zeros(off.size, np.uint64)
    rc = L.kmu_minimizer_layout(_ptr(off)[0], off.size - 1, k, w, _ptr(out)[0])
    if rc:
        raise KmuError(rc, "kmu_minimizer_layout: k %d, w %d" % (k, w))
    return out


def kmer_owner(kmer_type, canon_kmers, n_parts):
    """kmu_kmer_owner: DispatchableT::dispatch of canonical k-mer values (host arithmetic)"""
    L = load()
    k = np.ascontiguousarray(canon_kmers, np.uint64)
    out = np.zeros(max(k.size, 1), np.uint32)
    rc = L.kmu_kmer_owner(kmer_type, _ptr(k)[0], k.size, n_parts, _ptr(out)[0])
    if rc:
        raise KmuError(rc, "kmu_kmer_owner")
    return out[:k.size]


def kmer_owner_minimizer(k, canon_kmers, n_parts):
    """kmu_kmer_owner_minimizer: the minimizer owner of Kmer64bit values of k bases (host arithmetic)"""
    L = load()
    v = np.ascontiguousarray(canon_kmers, np.uint64)
    out = np.zeros(max(v.size, 1), np.uint32)
    rc = L.kmu_kmer_owner_minimizer(k, _ptr(v)[0], v.size, n_parts, _ptr(out)[0])
    if rc:
        raise KmuError(rc, "kmu_kmer_owner_minimizer")
    return out[:v.size]
