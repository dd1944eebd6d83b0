"""-m gpu: the timed kernel names and launch counts of three calls, pinned to what the library reported before every launch went
through the one `launch` step of kmu_ctx.hpp (scripts/profile_launches.py prints the same for every family of entry points).
The three are where that step can go wrong:
  components with member lists   four k_cc_* launches and the sort passes that radix_id_passes(n_nodes) selects;
  an exact partitioned add_reads `k_part_scan1` and `k_arr_scan` are ONE timed launch for two kernels each (a KernelTimer scope);
  a per-read sketch with a genome the helpers of that route (k_max_len, k_nk_scan) were never timed: a launch that passes no name
                                 stays out of the profile (profile_get reads at most 32 names).
With profiling off the same calls leave the profile empty.  The expected dictionaries are what the library of the commit before
reported for these calls on an MI355X (and what this one reports).

Two more, pinned to what the library reported before kmu_anchor_overlaps and kmu_seed_chains took their grouping (keys, two sorts
with a gather between them, heads, scans, starts) from the one pipeline of kmu_runs.h; a lost or doubled sort pass shows here:
  anchor_overlaps, two strands   five passes over the diagonal keys, two over the read pairs (9 reads: one byte per side);
  seed_chains with max_pos       five passes over (strand, x, y + max_pos) at max_pos = 2999, two over the read pairs.
Both with upper=True, so the COUNT form of the keys kernel runs, and both through lib.Context, whose one call is two calls of
the library: one that counts, one that writes."""
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chains_abi import side  # noqa: E402
from test_gpu_anchor_overlaps import random_case  # noqa: E402

pytestmark = pytest.mark.gpu

N_NODES, N_EDGES = 1000, 2000  # n_nodes - 1 = 999 has two bytes: two radix passes over the (cluster, node) entries

COMPONENTS = {"k_cc_init": 1, "k_cc_hook": 1, "k_cc_flatten": 1, "k_cc_number": 1, "k_sort_hist": 2, "k_sort_scatter": 2,
              "k_ing_scan": 3}  # (the scans: the root flags, and one per sort pass)
COUNT_EXACT = {"k_part_hist1": 1, "k_part_scan1": 1, "k_part_scatter1": 1, "k_arr_hist": 1, "k_arr_scan": 1, "k_arr_scatter": 1,
               "k_part_build_q": 1}
SKETCH_LONG = {"k_sketch_pmh3a": 2, "k_seq_hashes_compact": 1, "k_arr_hist": 1, "k_arr_scan": 1, "k_arr_scatter": 1, "k_pmh_reduce": 1}
OVERLAPS = {"k_ovl_keys_count": 2, "k_ovl_keys_write": 2, "k_sort_hist": 14, "k_sort_scatter": 14, "k_ovl_gather": 2,
            "k_ovl_heads": 2, "k_ovl_starts": 2, "k_ovl_runs": 2, "k_ovl_best_count": 2, "k_ovl_best_write": 1,
            "k_ing_scan": 22}  # (the scans of a library call: the tile counts, one per sort pass, two flag arrays, keep)
CHAINS = {"k_chain_keys_count": 2, "k_chain_keys_write": 2, "k_sort_hist": 14, "k_sort_scatter": 14, "k_chain_gather": 2,
          "k_chain_heads": 2, "k_chain_starts": 2, "k_chain_dp": 2, "k_chain_best_count": 2, "k_chain_best_write": 1,
          "k_ing_scan": 22}
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


def test_anchor_overlaps_launches(ctx):
    off, pairs, dist = random_case(np.random.default_rng(0xCC4), 500, n_reads=9)

    def anchor_overlaps():
        assert ctx.anchor_overlaps(pairs, dist, off, strands=2, band=1, upper=True).shape[0] > 0

    assert launches(ctx, anchor_overlaps) == OVERLAPS
    assert launches(ctx, anchor_overlaps, profiling=False) == {}


def test_seed_chains_launches(ctx):
    rng = np.random.default_rng(0xCC5)
    nq, ndb = 60, 50  # entries of 4 and of 3 reads, strands on both sides
    q = side(rng.integers(0, 3000, nq), rng.integers(0, 4, nq), rng.integers(0, 2, nq), 4)
    db = side(rng.integers(0, 3000, ndb), rng.integers(0, 3, ndb), rng.integers(0, 2, ndb), 3)
    pairs = np.stack([rng.integers(0, nq, 1500), rng.integers(0, ndb, 1500)], axis=1).astype(np.uint32)

    def seed_chains():
        assert ctx.seed_chains(pairs, q, db, 15, 500, 100, max_pos=2999, upper=True).shape[0] > 0

    assert launches(ctx, seed_chains) == CHAINS
    assert launches(ctx, seed_chains, profiling=False) == {}
