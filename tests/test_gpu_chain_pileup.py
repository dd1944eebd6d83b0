"""-m gpu: kmu_chain_pileup against `reference_pileup` and kmu_pile_call against `reference_call` (tests/test_pileup_abi.py: the
contracts of include/kmu.h in plain numpy).  Whole tables are compared byte for byte.  The pileup depends on the run structure and
the letters only, so the edge cases synthesise run lists (synth_chains) and need no aligner; the planted truth and the cross-check
go through Context.chain_cigar on hand-made whole-read chain records."""
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import ALN, batch, chain_recs, revcomp  # noqa: E402
from test_gpu_chain_align import ACGT, mutate  # noqa: E402
from test_pileup_abi import LETTER_CODE, READ_PILE, depth_of, random_runs, reference_call, reference_pileup, synth_chains  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def same_table(got, want, what=""):
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s row %d of %d rows that differ: got %s, want %s" % (what, bad[0], bad.size, got[bad[0]], want[bad[0]])


def check(ctx, case, separate=False):
    """the device's tables equal to the reference's in every byte; case: what synth_chains returns.  separate: two tables of the
    one batch instead of the shared table of the self-join"""
    chains, aln, ops, off, bases, offsets = case
    if separate:
        want = reference_pileup(chains, aln, ops, off, bases, offsets, bases, offsets)
        got = ctx.chain_pileup(chains, aln, ops, off, bases, offsets, bases, offsets.copy())
        same_table(got[0], want[0], "q")
        same_table(got[1], want[1], "db")
    else:
        want = reference_pileup(chains, aln, ops, off, bases, offsets)
        got = ctx.chain_pileup(chains, aln, ops, off, bases, offsets)
        assert got[0] is got[1]
        same_table(got[0], want[0])
    return got


def to_device(case):
    """the arrays of a case as torch tensors on the device, holding the same bits"""
    import torch
    chains, aln, ops, off, bases, offsets = case

    def dev(x, dtype):
        return torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).cuda()
    return (dev(chains, np.int32).reshape(-1, 10), dev(aln, np.int32).reshape(-1, 4), dev(ops, np.int32), dev(off, np.int64), dev(bases, np.uint8),
            dev(offsets, np.int64))


def host_table(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the edges of the tiles and of the run lengths --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_runs", [0, 1, 63, 64, 65, 127, 128, 129, 1000])
def test_tile_edges(ctx, n_runs):
    """one chain with this many runs on either strand, and a few small ones around it"""
    rng = np.random.default_rng(n_runs)
    lists = [random_runs(rng, 3), random_runs(rng, n_runs), random_runs(rng, n_runs), random_runs(rng, 5)]
    case = synth_chains(rng, lists, [0, 0, 1, 1])
    check(ctx, case)
    check(ctx, case, separate=True)


@pytest.mark.parametrize("length", [1, 63, 64, 65, 5000])
def test_run_length_edges(ctx, length):
    """one run of this length for each of the four ops alone and inside a chain; one long I run then one long D run; a chain that starts
    with D, one that ends with D, and one that starts with I on strand 1 (the j = n rule where it also ends with one)"""
    rng = np.random.default_rng(length)
    lists, strands = [], []
    for s in (0, 1):
        for x in "=XID":
            lists += [[(length, x)], random_runs(rng, 4) + [(length, x)] + random_runs(rng, 70)]
        lists += [[(length, "I"), (length, "D")], [(length, "D"), (3, "="), (2, "I")], [(4, "X"), (length, "D")], [(length, "I"), (5, "="), (length, "I")],
                  [(2, "I"), (length, "I"), (1, "D"), (length, "D")]]  # (cut runs)
        strands += [s] * (len(lists) - len(strands))
    check(ctx, synth_chains(rng, lists, strands, pad=2))


def test_lower_case_letters_and_both_strands(ctx):
    rng = np.random.default_rng(7)
    lists = [random_runs(rng, int(rng.integers(1, 90))) for _ in range(24)]
    case = synth_chains(rng, lists, [c & 1 for c in range(24)], lower=True)
    upper = (case[0], case[1], case[2], case[3], case[4] & 0xDF, case[5])
    got = check(ctx, case)[0]
    same_table(got, check(ctx, upper)[0])


def test_contention_300_chains_on_the_same_100_bases(ctx):
    rng = np.random.default_rng(8)
    lists = [[(100, "=")] if c % 3 else [(40, "="), (2, "D"), (60, "X")] for c in range(300)]
    case = synth_chains(rng, lists, [c & 1 for c in range(300)], shared_a=(0, 17))
    pile = check(ctx, case)[0]
    assert (depth_of(pile)[17:117] == 300).all() and pile[17, A.PILE_ENDS] == pile[116, A.PILE_ENDS] == 300
    assert pile[17 + 39, A.PILE_INS] == 100 and pile[17 + 39, A.PILE_INS_BASES] == 200


# ---- sides, tables, skipped chains --------------------------------------------------------------------------------------------------
def mixed_case(seed=9, n=40):
    rng = np.random.default_rng(seed)
    return synth_chains(rng, [random_runs(rng, int(rng.integers(1, 150))) for _ in range(n)], [int(rng.integers(0, 2)) for _ in range(n)])


def test_one_side_only_leaves_the_other_table_alone(ctx):
    chains, aln, ops, off, bases, offsets = case = mixed_case()
    for side in (A.PILE_Q, A.PILE_DB):
        want = reference_pileup(*case, bases, offsets, sides=side)
        got = ctx.chain_pileup(*case, bases, offsets.copy(), sides=side)
        mine, other = (0, 1) if side == A.PILE_Q else (1, 0)
        assert got[other] is None and not want[other].any()
        same_table(got[mine], want[mine])
        # a table that is there all the same is not touched
        pattern = np.full(want[0].shape, 0xABCD0123, np.uint32)
        tables = [np.zeros_like(pattern), np.zeros_like(pattern)]
        tables[other] = pattern.copy()
        ctx.chain_pileup(*case, bases, offsets.copy(), sides=side, into=tuple(tables))
        same_table(tables[mine], want[mine])
        assert (tables[other] == pattern).all()
    # the self-join into one table is the sum of the two sides
    q, db = reference_pileup(*case, bases, offsets)
    shared = ctx.chain_pileup(*case)[0]
    same_table(shared, q + db)
    same_table(ctx.chain_pileup(*case, sides=A.PILE_Q)[0], q)


def test_separate_q_and_db_batches(ctx):
    """the A segments in one batch, the B segments in another"""
    rng = np.random.default_rng(10)
    chains, aln, ops, off, bases, offsets = synth_chains(rng, [random_runs(rng, int(rng.integers(1, 100))) for _ in range(16)], [c & 1 for c in range(16)])
    reads = [bases[int(offsets[r]):int(offsets[r + 1])].tobytes().decode() for r in range(32)]
    bq, oq = batch(reads[0::2])
    bdb, odb = batch(reads[1::2] + ["ACGT"])
    chains["read_a"], chains["read_b"] = chains["read_a"] // 2, chains["read_b"] // 2
    want = reference_pileup(chains, aln, ops, off, bq, oq, bdb, odb)
    got = ctx.chain_pileup(chains, aln, ops, off, bq, oq, bdb, odb)
    assert got[0] is not got[1] and got[1].shape[0] == bdb.size
    same_table(got[0], want[0], "q")
    same_table(got[1], want[1], "db")


def test_chains_without_path_or_done_vote_nothing(ctx):
    chains, aln, ops, off, bases, offsets = mixed_case(11, 30)
    keep = np.ones(30, bool)
    keep[[0, 4, 5, 17, 29]] = False
    parts = [ops[int(off[c]):int(off[c + 1])] if keep[c] else ops[:0] for c in range(30)]
    off2 = np.zeros(31, np.uint64)
    off2[1:] = np.cumsum([p.size for p in parts])
    aln2 = aln.copy()
    aln2["flags"][[0, 4, 29]] = A.ALN_DONE | A.ALN_EXACT              # aligned, no path
    aln2[[5, 17]] = np.array([(0xFFFFFFFF, 0, 1300, 0)] * 2, ALN)     # not aligned
    case = (chains, aln2, np.concatenate(parts), off2, bases, offsets)
    got = check(ctx, case)[0]
    same_table(got, reference_pileup(chains[keep], aln[keep], case[2], off2[np.r_[keep, True]], bases, offsets)[0])


def test_accumulation_and_order(ctx):
    chains, aln, ops, off, bases, offsets = case = mixed_case(12, 50)
    whole = check(ctx, case)[0]
    cut = 23
    first = (chains[:cut], aln[:cut], ops[:int(off[cut])], off[:cut + 1], bases, offsets)
    second = (chains[cut:], aln[cut:], ops[int(off[cut]):], off[cut:] - off[cut], bases, offsets)
    table = ctx.chain_pileup(*first)[0]
    assert ctx.chain_pileup(*second, into=table)[0] is table
    same_table(table, whole)
    perm = np.random.default_rng(3).permutation(50)
    parts = [ops[int(off[c]):int(off[c + 1])] for c in perm]
    poff = np.zeros(51, np.uint64)
    poff[1:] = np.cumsum([p.size for p in parts])
    same_table(ctx.chain_pileup(chains[perm], aln[perm], np.concatenate(parts), poff, bases, offsets)[0], whole)


def test_device_mode_equals_host_mode(ctx):
    import torch
    case = mixed_case(13, 60)
    want = check(ctx, case)[0]
    dev = to_device(case)
    got = ctx.chain_pileup(*dev)
    assert got[0] is got[1] and got[0].is_cuda and got[0].dtype == torch.int32
    same_table(host_table(got[0]), want)
    again = ctx.chain_pileup(*dev, into=got[0])[0]  # accumulates on the device too
    same_table(host_table(again), 2 * want)
    q, db = ctx.chain_pileup(*dev, dev[4], dev[5].clone())
    same_table(host_table(q) + host_table(db), want)
    assert ctx.chain_pileup(dev[0][:0], dev[1][:0], dev[2][:0], dev[3][:1], dev[4], dev[5])[0].sum().item() == 0
    empty = ctx.chain_pileup(case[0][:0], case[1][:0], case[2][:0], case[3][:1], case[4], case[5])[0]
    assert empty.shape == want.shape and not empty.any()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _spoil(case, what):
    chains, aln, ops, off, bases, offsets = (x.copy() for x in case)
    c = 3
    lo = int(off[c])
    if what == "read_a":
        chains["read_a"][c] = len(offsets) - 1
    elif what == "read_b":
        chains["read_b"][c] = 0xFFFFFFFF
    elif what == "strand":
        chains["strand"][c] = 2
    elif what == "start_above_end":
        chains["a_start"][c] = chains["a_end"][c] + 1
    elif what == "end_above_read":
        chains["b_end"][c] = int(offsets[chains["read_b"][c] + 1] - offsets[chains["read_b"][c]]) + 1
    elif what == "offsets_decrease":
        off[c + 1] = off[c] - 1
    elif what == "offsets_above_n_ops":
        ops = ops[:-1]
    elif what == "offsets_far_above_n_ops":
        off[-1] = 1 << 40
    elif what == "runs_without_path":
        aln["flags"][c] = A.ALN_DONE
    elif what == "unknown_op":
        ops[lo + 2] = ops[lo + 2] & ~np.uint32(15) | np.uint32(0)   # BAM's M
    elif what == "unknown_op_3":
        ops[lo] = 5 << 4 | 3
    elif what == "length_0":
        ops[lo + 1] = ops[lo + 1] & np.uint32(15)
    elif what == "a_short":
        chains["a_end"][c] += 1
    elif what == "a_long":
        chains["a_start"][c] += 1
    elif what == "b_short":
        chains["b_start"][c] -= 1
    elif what == "b_long":
        chains["b_end"][c] -= 1
    elif what == "huge_run":
        ops[lo + 1] = np.uint32(A.CIGAR_MAX_RUN << 4 | 7)
    return chains, aln, ops, off, bases, offsets


SPOILED = ["read_a", "read_b", "strand", "start_above_end", "end_above_read", "offsets_decrease", "offsets_above_n_ops", "offsets_far_above_n_ops",
           "runs_without_path", "unknown_op", "unknown_op_3", "length_0", "a_short", "a_long", "b_short", "b_long", "huge_run"]


@pytest.fixture(scope="module")
def refusal_case():
    rng = np.random.default_rng(14)
    lists = [[(3, "="), (2, "I"), (4, "X"), (1, "D"), (6, "=")] + random_runs(rng, int(rng.integers(0, 100))) for _ in range(8)]
    return synth_chains(rng, lists, [c & 1 for c in range(8)], pad=5)


@pytest.mark.parametrize("what", SPOILED)
def test_unsupported_is_found_before_any_vote(ctx, refusal_case, what):
    """on the device's own tables (device mode), filled with a pattern that must come back unchanged; and on host arrays"""
    import torch
    bad = _spoil(refusal_case, what)
    dev = to_device(bad)
    table = torch.full((int(bad[5][-1]), A.PILE_COLS), 0x5A5A5A5, dtype=torch.int32, device="cuda")
    with pytest.raises(lib.KmuError) as e:
        ctx.chain_pileup(*dev, into=table)
    assert e.value.code == A.E_UNSUPPORTED
    assert (table == 0x5A5A5A5).all().item()
    host = np.full((int(bad[5][-1]), A.PILE_COLS), 77, np.uint32)
    with pytest.raises(lib.KmuError) as e:
        ctx.chain_pileup(*bad, into=host)
    assert e.value.code == A.E_UNSUPPORTED and (host == 77).all()
    check(ctx, refusal_case)  # the context goes on working


def test_bad_arguments_and_non_acgt(ctx, refusal_case):
    chains, aln, ops, off, bases, offsets = refusal_case
    for sides in (0, 4, 7):
        with pytest.raises(lib.KmuError) as e:
            ctx.chain_pileup(*refusal_case, sides=sides, into=np.zeros((bases.size, 8), np.uint32))
        assert e.value.code == A.E_BAD_ARG
    with pytest.raises(lib.KmuError) as e:  # one table for two different batches
        ctx.chain_pileup(*refusal_case, bases, offsets.copy(), into=np.zeros((bases.size, 8), np.uint32))
    assert e.value.code == A.E_BAD_ARG
    with pytest.raises(lib.KmuError) as e:
        ctx.pile_call(np.zeros((bases.size, 8), np.uint32), bases, offsets, min_depth=0)
    assert e.value.code == A.E_BAD_ARG
    # an N under a voted column; under a column of the side that is not voted it is not looked at
    rec = chains[2]
    spoiled = bases.copy()
    spoiled[int(offsets[rec["read_b"]]) + int(rec["b_start"]) + (0 if not rec["strand"] else int(rec["b_end"] - rec["b_start"]) - 1)] = ord("N")
    with pytest.raises(lib.KmuError) as e:
        ctx.chain_pileup(chains, aln, ops, off, spoiled, offsets)
    assert e.value.code == A.E_NON_ACGT
    with pytest.raises(lib.KmuError) as e:
        ctx.chain_pileup(chains, aln, ops, off, spoiled, offsets, sides=A.PILE_Q)
    assert e.value.code == A.E_NON_ACGT
    got = ctx.chain_pileup(chains, aln, ops, off, spoiled, offsets, sides=A.PILE_DB)[1]  # B's own letters are not voted onto B
    same_table(got, reference_pileup(chains, aln, ops, off, bases, offsets, sides=A.PILE_DB)[1])


# ---- pile_call ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call_case():
    """reads of 1, 63, 64, 65 and 10 000 bases and an empty one, with a table of small random counts (many ties) and a few large ones"""
    rng = np.random.default_rng(15)
    lengths = [1, 63, 0, 64, 65, 10000, 7]
    bases, offsets = batch(["".join(rng.choice(list("ACGTacgtN"), n)) for n in lengths])
    pile = rng.integers(0, 3, (bases.size, 8)).astype(np.uint32)
    pile[rng.integers(0, bases.size, 200), rng.integers(0, 8, 200)] = 0xFFFFFFFF
    pile[100:140] = 0
    return pile, bases, offsets


@pytest.mark.parametrize("min_depth", [1, 3])
def test_pile_call(ctx, call_case, min_depth):
    import torch
    pile, bases, offsets = call_case
    want_call, want_reads = reference_call(pile, bases, offsets, min_depth)
    call, reads = ctx.pile_call(pile, bases, offsets, min_depth=min_depth)
    assert call.dtype == np.uint8 and reads.dtype == READ_PILE
    assert (call == want_call).all() and reads.tobytes() == want_reads.tobytes()
    only_call, none = ctx.pile_call(pile, bases, offsets, min_depth=min_depth, want=("call",))
    assert none is None and (only_call == want_call).all()
    none, only_reads = ctx.pile_call(pile, bases, offsets, min_depth=min_depth, want=("reads",))
    assert none is None and only_reads.tobytes() == want_reads.tobytes()
    with pytest.raises(ValueError):
        ctx.pile_call(pile, bases, offsets, want=())
    d_call, d_reads = ctx.pile_call(torch.from_numpy(pile.view(np.int32)).cuda(), torch.from_numpy(bases).cuda(), offsets, min_depth=min_depth)
    assert d_call.is_cuda and (d_call.cpu().numpy() == want_call).all()
    assert d_reads.cpu().numpy().tobytes() == want_reads.tobytes()


def test_pile_call_on_the_tables_of_the_pileup(ctx):
    chains, aln, ops, off, bases, offsets = case = mixed_case(16, 80)
    pile = ctx.chain_pileup(*case)[0]
    for min_depth in (1, 3):
        call, reads = ctx.pile_call(pile, bases, offsets, min_depth=min_depth)
        want = reference_call(pile, bases, offsets, min_depth)
        assert (call == want[0]).all() and reads.tobytes() == want[1].tobytes()
    assert reads["depth_sum"].sum() == depth_of(pile).sum() > 0


# ---- through the aligner ------------------------------------------------------------------------------------------------------------
def test_planted_truth(ctx):
    """read 0 is T with six substitutions, reads 1 .. 5 are T (even ones reverse-complemented): the five partners outvote read 0 at
    exactly the six positions; the hand-made whole-read chains do not depend on seed finding"""
    rng = np.random.default_rng(17)
    truth = "".join(rng.choice(list("ACGT"), 600))
    planted = [60, 130, 222, 311, 455, 540]
    read0 = list(truth)
    for p in planted:
        read0[p] = "ACGT"[("ACGT".index(read0[p]) + 1 + p % 3) % 4]
    reads = ["".join(read0)] + [truth if r & 1 else revcomp(truth) for r in range(1, 6)]
    bases, offsets = batch(reads)
    chains = chain_recs([(0, r, 0 if r & 1 else 1, 0, 600, 0, 600) for r in range(1, 6)])
    aln, ops, op_off = ctx.chain_cigar(chains, bases, offsets, band=64)
    assert (aln["flags"] & A.ALN_PATH).all() and aln["edit"].tolist() == [6] * 5
    pile, same = ctx.chain_pileup(chains, aln, ops, op_off, bases, offsets)
    assert pile is same
    call, summary = ctx.pile_call(pile, bases, offsets, min_depth=3)
    diff = np.nonzero(call[:600] & A.CALL_DIFF)[0]
    assert diff.tolist() == planted
    assert (call[:600][planted] & 7).tolist() == [int(LETTER_CODE[ord(truth[p])]) for p in planted]
    assert all(pile[p, LETTER_CODE[ord(truth[p])]] == 5 for p in planted)
    assert summary[0].tolist() == (600, 600, 6, 0, 0, 5, 3000)
    assert (call[600:] == A.CALL_NONE).all() and summary["covered"][1:].tolist() == [0] * 5  # depth 1 is below 3
    call1, summary1 = ctx.pile_call(pile, bases, offsets, min_depth=1)
    for r in range(1, 6):
        mine = call1[600 * r:600 * (r + 1)]
        where = sorted(p if r & 1 else 599 - p for p in planted)
        assert np.nonzero(mine & A.CALL_DIFF)[0].tolist() == where
        assert [int(mine[q] & 7) for q in where] == [int(LETTER_CODE[ord(reads[0][q])]) if r & 1 else 3 - int(LETTER_CODE[ord(reads[0][599 - q])]) for q in where]
        assert summary1[r].tolist() == (600, 600, 6, 0, 0, 1, 600)


def test_cross_check_on_the_device_s_own_cigars(ctx):
    """40 related reads of 2 kb, every second one reverse-complemented; chains (r, r + 1) and (r, r + 7) take the reads whole"""
    rng = np.random.default_rng(18)
    root = rng.choice(ACGT, 2000).astype(np.uint8)
    reads = []
    for r in range(40):
        s = bytes(mutate(rng, root, 0.04)[0]).decode()
        reads.append(revcomp(s) if r & 1 else s)
    bases, offsets = batch(reads)
    rows = [(r, q, (r ^ q) & 1, 0, len(reads[r]), 0, len(reads[q])) for r in range(40) for q in (r + 1, r + 7) if q < 40]
    chains = chain_recs(rows)
    aln, ops, op_off = ctx.chain_cigar(chains, bases, offsets, band=64)
    assert (aln["flags"] & A.ALN_PATH).all() and ops.size > 5000
    pile = ctx.chain_pileup(chains, aln, ops, op_off, bases, offsets)[0]
    same_table(pile, reference_pileup(chains, aln, ops, op_off, bases, offsets)[0])
    call, summary = ctx.pile_call(pile, bases, offsets)
    want = reference_call(pile, bases, offsets)
    assert (call == want[0]).all() and summary.tobytes() == want[1].tobytes()
    assert int(summary["max_depth"].max()) == 4 and int(pile[:, A.PILE_ENDS].sum()) == 4 * len(rows)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_read_pileups_from_reads_to_calls(ctx):
    """12 reads of one 3 kb sequence with 3 % edits, every second one reverse-complemented: read_pileups finds the chains itself;
    its table equals reference_pileup on the chains and runs it returns beside it, its calls reference_call; on resident arrays
    everything stays on the device and holds the same bytes"""
    import torch
    from kmerutils_amd import minimizer
    rng = np.random.default_rng(19)
    root = rng.choice(ACGT, 3000).astype(np.uint8)
    reads = []
    for r in range(12):
        s = bytes(mutate(rng, root, 0.03)[0]).decode()
        reads.append(revcomp(s) if r & 1 else s)
    bases, offsets = batch(reads)
    chains, aln, pile, call, summary = minimizer.read_pileups(ctx, bases, offsets, 15, 10, min_depth=2)
    assert chains.shape[0] >= 30 and (aln["flags"] & A.ALN_PATH).all()
    _, ops, op_off = ctx.chain_cigar(chains, bases, offsets, band=64)
    same_table(pile, reference_pileup(chains, aln, ops, op_off, bases, offsets)[0])
    want = reference_call(pile, bases, offsets, 2)
    assert (call == want[0]).all() and summary.tobytes() == want[1].tobytes()
    assert (summary["covered"] > 2000).all() and (summary["n_diff"] > 20).all() and int(summary["max_depth"].max()) <= 11
    d = minimizer.read_pileups(ctx, torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), 15, 10, min_depth=2)
    assert all(x.is_cuda for x in d)
    assert [x.cpu().numpy().tobytes() for x in d] == [chains.tobytes(), aln.tobytes(), pile.tobytes(), call.tobytes(), summary.tobytes()]


def test_the_kernels_that_ran(ctx):
    case = mixed_case(20, 10)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        pile = ctx.chain_pileup(*case)[0]
        ctx.pile_call(pile, case[4], case[5])
        assert {"k_pile_count", "k_pile_starts", "k_pile_vote", "k_pile_call", "k_pile_reads"} <= set(ctx.profile_get())
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
