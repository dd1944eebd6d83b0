"""-m gpu: the timed kernel names and launch counts of three calls, pinned to what the library reported before every launch went
through the one `launch` step of kmu_ctx.hpp (scripts/profile_launches.py prints the same for every family of entry points).
The three are where that step can go wrong:
  components with member lists   four k_cc_* launches and the sort passes that radix_id_passes(n_nodes) selects;
  an exact partitioned add_reads `k_part_scan1` and `k_arr_scan` are ONE timed launch for two kernels each (a KernelTimer scope);
  a per-read sketch with a genome the helpers of that route (k_max_len, k_nk_scan) were never timed: a launch that passes no name
                                 stays out of the profile (profile_get reads at most 32 names).
With profiling off the same calls leave the profile empty.  The expected dictionaries are what the library of the commit before
reported for these calls on an MI355X (and what this one reports)."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, synth

pytestmark = pytest.mark.gpu

N_NODES, N_EDGES = 1000, 2000  # n_nodes - 1 = 999 has two bytes: two radix passes over the (cluster, node) entries

COMPONENTS = {"k_cc_init": 1, "k_cc_hook": 1, "k_cc_flatten": 1, "k_cc_number": 1, "k_sort_hist": 2, "k_sort_scatter": 2,
              "k_ing_scan": 3}  # (the scans: the root flags, and one per sort pass)
COUNT_EXACT = {"k_part_hist1": 1, "k_part_scan1": 1, "k_part_scatter1": 1, "k_arr_hist": 1, "k_arr_scan": 1, "k_arr_scatter": 1,
               "k_part_build_q": 1}
SKETCH_LONG = {"k_sketch_pmh3a": 2, "k_seq_hashes_compact": 1, "k_arr_hist": 1, "k_arr_scan": 1, "k_arr_scatter": 1, "k_pmh_reduce": 1}
UNTIMED = ("k_max_len", "k_nk_scan", "k_widen_u32", "k_pts_long_list", "k_fill_linear", "k_spill_header", "k_seg_tails")


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def launches(ctx, call, profiling=True):
    """{timed name: launches} of call() on a clean profile"""
    ctx.profile_reset()
    ctx.profile_enable(profiling)
    try:
        call()
        ctx.synchronize()
        prof = {name: n for name, (n, _) in ctx.profile_get().items()}
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    print(call.__name__, dict(sorted(prof.items())))
    return prof


def test_components_launches(ctx):
    rng = np.random.default_rng(0xCC1)
    edges = rng.integers(0, N_NODES, size=(N_EDGES, 2)).astype(np.uint32)

    def components():
        got = ctx.components(edges, N_NODES)
        assert got.members.shape == (N_NODES,) and 1 <= got.n_components < N_NODES

    assert launches(ctx, components) == COMPONENTS
    assert launches(ctx, components, profiling=False) == {}


def test_exact_partition_launches(ctx, monkeypatch):
    monkeypatch.setenv("KMU_COUNT_PATH", "partitioned")
    monkeypatch.setenv("KMU_COUNT_SEG", "0")  # the exact levels: the route with the two-kernel scans
    bases, off = synth.genome_reads(24, np.full(24, 3030, np.int64), 4_000_000, 0xCC2)  # 72 000 31-mers: a little above 2^16

    def add_reads():
        c = ctx.counter(A.KMER64BIT, 31, 8, 12_000_000)  # 2^25 slots: two partition levels
        try:
            c.add_reads(bases, off)
        finally:
            c.close()

    assert int(off[-1]) - 30 * (len(off) - 1) > 1 << 16
    assert launches(ctx, add_reads) == COUNT_EXACT
    assert launches(ctx, add_reads, profiling=False) == {}


def test_untimed_helpers_stay_untimed(ctx):
    """a per-read ProbMinHash3a sketch of a few reads and one sequence of more than 2^18 k-mers: the longest length is looked for on
    the device (k_max_len), the long sequence goes through the all-sequences route (k_nk_scan), none of them under a name"""
    bases, off = synth.genome_reads(6, np.array([3000, 500, (1 << 18) + 4000, 150, 9000, 2000], np.int64), 2_000_000, 0xCC3)
    p = A.SketchParams(A.ALGO_PROB3A, A.KMER64BIT, 31, 64, A.SIG_U64, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)

    def sketch():
        sig = ctx.sketch(bases, off, p)
        assert sig.shape == (6, 64)

    prof = launches(ctx, sketch)
    assert not [name for name in UNTIMED if name in prof]
    assert "k_seq_hashes_compact" in prof and "k_pmh_reduce" in prof  # the long sequence did take the all-sequences route
    assert prof == SKETCH_LONG
    assert launches(ctx, sketch, profiling=False) == {}
