"""-m "not gpu": the host side of read correction -- `reference_ins_plan`, `reference_ins_votes` and `reference_consensus`: the
contracts of kmu_pile_ins_plan, kmu_chain_pile_ins and kmu_pile_consensus (include/kmu.h) as plain numpy, which
tests/test_gpu_pile_consensus.py compares the device against; hand cases worked out on paper; the symbols and their bindings, the
constants and struct sizes, refusals that need no device, and the minimizer wrappers on a stub context."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import ALN, batch, chain_recs  # noqa: E402
from test_pileup_abi import LETTER_CODE, PATH, NonACGT, random_runs, reference_call, reference_pileup, run_word, synth_chains  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the references ---------------------------------------------------------------------------------------------------------------
def depth_of(pile):
    return (np.asarray(pile).astype(np.int64)[:, :5] & 0xFFFFFFFF).sum(axis=1)


def reference_ins_plan(pile, call, max_ins=16):
    """(ins_len uint8 [n_bases], n_slots) of kmu_pile_ins_plan by the text of include/kmu.h"""
    depth = depth_of(pile)
    ins_bases = np.asarray(pile).astype(np.int64)[:, A.PILE_INS_BASES] & 0xFFFFFFFF
    has = ((np.asarray(call) & A.CALL_INS) != 0) & (depth > 0) & (ins_bases > 0)
    n = np.where(has, np.minimum(max_ins, (2 * ins_bases - 1) // np.maximum(depth, 1)), 0)
    return n.astype(np.uint8), int(n.sum())


def slot_base(ins_len):
    """S: the exclusive prefix sum of ins_len (one more entry: the total)"""
    return np.concatenate([[0], np.cumsum(np.asarray(ins_len).astype(np.int64))])


def reference_ins_votes(chains, aln, ops, op_offsets, bases_q, offsets_q, ins_len_q, bases_db=None, offsets_db=None, ins_len_db=None,
                        sides=A.PILE_Q | A.PILE_DB, into=None):
    """(ins_q, ins_db) of kmu_chain_pile_ins by the text of include/kmu.h (valid input only): uint32 [n_slots, 4]; one shared table in
    the self-join; into=(ins_q, ins_db) accumulates; NonACGT for a voted letter outside ACGTacgt"""
    own = bases_db is None
    if own:
        bases_db, offsets_db, ins_len_db = bases_q, offsets_q, ins_len_q
    s_q = slot_base(ins_len_q) if ins_len_q is not None else None
    s_db = s_q if own else (slot_base(ins_len_db) if ins_len_db is not None else None)
    if into is not None:
        ins_q, ins_db = into
    else:
        ins_q = np.zeros((int(s_q[-1]) if s_q is not None else 0, A.INS_COLS), np.uint32)
        ins_db = ins_q if own else np.zeros((int(s_db[-1]) if s_db is not None else 0, A.INS_COLS), np.uint32)
    ops, off = np.asarray(ops).astype(np.int64) & 0xFFFFFFFF, np.asarray(op_offsets).astype(np.int64)
    vote_q, vote_db = bool(sides & A.PILE_Q), bool(sides & A.PILE_DB)

    def code_of(byte, s):
        code = int(LETTER_CODE[byte])
        if code == 5:
            raise NonACGT()
        return 3 - code if s else code
    for c, rec in enumerate(chains):
        if not int(aln[c]["flags"]) & A.ALN_PATH:
            continue
        a0, a1, b0, b1, s = (int(rec[f]) for f in ("a_start", "a_end", "b_start", "b_end", "strand"))
        n = b1 - b0
        row_a = int(offsets_q[rec["read_a"]]) + a0
        beg_b = int(offsets_db[rec["read_b"]])

        def pos_b(j):  # base j of B' as a row of the db batch
            return beg_b + (b1 - 1 - j if s else b0 + j)
        i = j = 0
        for v in ops[off[c]:off[c + 1]].tolist():
            length, op = v >> 4, v & 15
            if op in (7, 8):
                i, j = i + length, j + length
            elif op == 2:  # D: bases of B' only, inserted behind A's base i - 1
                if vote_q and i > 0:
                    g = row_a + i - 1
                    for k in range(min(length, int(ins_len_q[g]))):
                        ins_q[s_q[g] + k, code_of(bases_db[pos_b(j + k)], s)] += 1
                j += length
            else:  # I: bases of A only, inserted behind the base before the gap in read b's forward direction
                at = (j if j < n else None) if s else (j - 1 if j > 0 else None)
                if vote_db and at is not None:
                    g = pos_b(at)
                    for k in range(min(length, int(ins_len_db[g]))):
                        ins_db[s_db[g] + k, code_of(bases_q[row_a + (i + length - 1 - k if s else i + k)], s)] += 1
                i += length
    return ins_q, ins_db


def reference_consensus(pile, call, ins_len, ins, bases, offsets):
    """(cons_bases uint8, cons_offsets uint64 [n_reads + 1]) of kmu_pile_consensus by the text of include/kmu.h"""
    depth, s = depth_of(pile), slot_base(ins_len)
    ins = np.asarray(ins).astype(np.int64) & 0xFFFFFFFF
    out, row_end = bytearray(), np.zeros(len(bases) + 1, np.int64)
    for g in range(len(bases)):
        code = int(call[g]) & 7
        if code < 4:
            out.append(ord("ACGT"[code]))
        elif code != A.PILE_DEL:
            out.append(int(bases[g]))
        for k in range(int(ins_len[g])):
            slot = ins[s[g] + k]
            if not 2 * int(slot.sum()) > int(depth[g]):
                break
            out.append(ord("ACGT"[int(slot.argmax())]))
        row_end[g + 1] = len(out)
    return np.frombuffer(bytes(out), np.uint8), row_end[np.asarray(offsets).astype(np.int64)].astype(np.uint64)


def reference_correct(chains, aln, ops, op_offsets, bases, offsets, min_depth=3, max_ins=16):
    """the whole route of the self-join on the references: (cons_bases, cons_offsets, pile, call, ins_len, ins)"""
    pile, _ = reference_pileup(chains, aln, ops, op_offsets, bases, offsets)
    call, _ = reference_call(pile, bases, offsets, min_depth)
    ins_len, _ = reference_ins_plan(pile, call, max_ins)
    ins, _ = reference_ins_votes(chains, aln, ops, op_offsets, bases, offsets, ins_len)
    return reference_consensus(pile, call, ins_len, ins, bases, offsets) + (pile, call, ins_len, ins)


# ---- hand cases -----------------------------------------------------------------------------------------------------------------
def one_chain(a, b, runs, strand):
    bases, off = batch([a, b])
    chains = chain_recs([(0, 1, strand, 0, len(a), 0, len(b))])
    aln = np.zeros(1, ALN)
    aln["flags"] = PATH
    ops = np.array([run_word(k, x) for k, x in runs], np.uint32)
    return chains, aln, ops, np.array([0, len(ops)], np.uint64), bases, off


def hand_votes(votes, a, b, runs, strand, ins_len):
    """the slot table of one whole-read chain, both sides into the shared table, as lists"""
    return np.asarray(votes(*one_chain(a, b, runs, strand), np.array(ins_len, np.uint8))).tolist()


def insertion_cases(votes):
    """the hand cases of the votes, worked out on paper; votes(chains, aln, ops, op_offsets, bases, offsets, ins_len) -> the self-join's
    slot table: reference_ins_votes here, the device in tests/test_gpu_pile_consensus.py"""
    def votes_by_hand(a, b, runs, strand, ins_len):
        return hand_votes(votes, a, b, runs, strand, ins_len)
    #                                                                A  C  G  T
    # A side, strand 0: A = AC, B = AGTC, 1=2D1=: GT sits behind A's base 0
    assert votes_by_hand("AC", "AGTC", [(1, "="), (2, "D"), (1, "=")], 0, [2, 0, 0, 0, 0, 0]) == [[0, 0, 1, 0], [0, 0, 0, 1]]
    # ... with one slot only, the T is dropped
    assert votes_by_hand("AC", "AGTC", [(1, "="), (2, "D"), (1, "=")], 0, [1, 0, 0, 0, 0, 0]) == [[0, 0, 1, 0]]
    # A side, strand 1: read b = GACT, B' = AGTC as above: the same letters, complemented from b's forward ones
    assert votes_by_hand("AC", "GACT", [(1, "="), (2, "D"), (1, "=")], 1, [2, 0, 0, 0, 0, 0]) == [[0, 0, 1, 0], [0, 0, 0, 1]]
    # B side, strand 0: A = AGTC, B = AC, 1=2I1=: GT sits behind B's base 0 (row 4)
    assert votes_by_hand("AGTC", "AC", [(1, "="), (2, "I"), (1, "=")], 0, [0, 0, 0, 0, 2, 0]) == [[0, 0, 1, 0], [0, 0, 0, 1]]
    # B side, strand 1: read b = GT (B' = AC).  The I run begins at j0 = 1, which is b's forward base 0 (row 4); in b's forward direction
    # the insertion reads revcomp(GT) = AC: slot 0 takes the complement of A's letter at i0 + L - 1 (T -> A), slot 1 that at i0 (G -> C)
    assert votes_by_hand("AGTC", "GT", [(1, "="), (2, "I"), (1, "=")], 1, [0, 0, 0, 0, 2, 0]) == [[1, 0, 0, 0], [0, 1, 0, 0]]
    # ... the slots of the other row (b's base 1) stay empty, and with one slot the vote is the first letter in b's direction
    assert votes_by_hand("AGTC", "GT", [(1, "="), (2, "I"), (1, "=")], 1, [0, 0, 0, 0, 1, 3]) == [[1, 0, 0, 0]] + [[0, 0, 0, 0]] * 3
    # an I run at j = 0 on strand 0 and at j = n on strand 1 has no row; a D run at i = 0 neither
    assert votes_by_hand("GA", "A", [(1, "I"), (1, "=")], 0, [1, 1, 1]) == [[0, 0, 0, 0]] * 3
    assert votes_by_hand("AG", "T", [(1, "="), (1, "I")], 1, [1, 1, 1]) == [[0, 0, 0, 0]] * 3
    assert votes_by_hand("A", "GA", [(1, "D"), (1, "=")], 0, [1, 1, 1]) == [[0, 0, 0, 0]] * 3
    # a letter beyond the row's slots is not looked at
    assert votes_by_hand("AC", "AGNC", [(1, "="), (2, "D"), (1, "=")], 0, [1, 0, 0, 0, 0, 0]) == [[0, 0, 1, 0]]


def adjacent_runs_case(votes):
    # A = AC, B = AGTC with the gap as 1D1D: G and T both vote into slot 0 of A's base 0; slot 1 stays empty
    assert hand_votes(votes, "AC", "AGTC", [(1, "="), (1, "D"), (1, "D"), (1, "=")], 0, [2, 0, 0, 0, 0, 0]) == [[0, 0, 1, 1], [0, 0, 0, 0]]


def test_insertions_on_each_side_and_strand():
    insertion_cases(lambda *case: reference_ins_votes(*case)[0])
    with pytest.raises(NonACGT):
        reference_ins_votes(*one_chain("AC", "ANTC", [(1, "="), (2, "D"), (1, "=")], 0), np.array([2, 0, 0, 0, 0, 0], np.uint8))


def test_two_adjacent_d_runs_both_start_at_slot_0():
    adjacent_runs_case(lambda *case: reference_ins_votes(*case)[0])


def hand_rows(rows, own, min_depth=1):
    pile = np.array(rows, np.uint32)
    bases, off = batch([own])
    call, _ = reference_call(pile, bases, off, min_depth)
    return pile, call, bases, off


def slot_count_cases(plan):
    """plan(pile, call, max_ins) -> (ins_len, n_slots): reference_ins_plan here, the device in tests/test_gpu_pile_consensus.py.
    2 INS_BASES - 1 = 5 against depth 5 (equal: one slot), depth 4 (one above: one slot) and depth 6 (one below: none -- a table
    kmu_chain_pileup cannot make, since INS_BASES >= INS, but a defined result); then larger counts and the cap"""
    #        A  C  G  T DEL INS INSB
    rows = [[5, 0, 0, 0, 0, 3, 3, 0], [4, 0, 0, 0, 0, 3, 3, 0], [6, 0, 0, 0, 0, 4, 3, 0],
            [5, 0, 0, 0, 0, 3, 5, 0],      # 9 // 5 = 1
            [5, 0, 0, 0, 0, 3, 8, 0],      # 15 // 5 = 3
            [5, 0, 0, 0, 0, 3, 1000, 0],   # 1999 // 5 = 399: the cap
            [5, 0, 0, 0, 0, 2, 9, 0],      # 2 INS = 4 < 5: no KMU_CALL_INS, no slots
            [3, 0, 0, 0, 2, 3, 3, 0]]      # DEL counts in the depth
    pile, call, bases, off = hand_rows(rows, "AAAAAAAA")
    assert (call & A.CALL_INS).tolist() == [8, 8, 8, 8, 8, 8, 0, 8]
    for max_ins, want in ((16, [1, 1, 0, 1, 3, 16, 0, 1]), (2, [1, 1, 0, 1, 2, 2, 0, 1]), (255, [1, 1, 0, 1, 3, 255, 0, 1]), (1, [1, 1, 0, 1, 1, 1, 0, 1])):
        ins_len, n_slots = plan(pile, call, max_ins)
        assert ins_len.dtype == np.uint8 and ins_len.tolist() == want and n_slots == sum(want)
    # an uncalled row has none; counts near 2^32 do not wrap
    pile3, call3, _, _ = hand_rows([[1, 0, 0, 0, 0, 1, 5, 0]], "A", min_depth=3)
    assert call3.tolist() == [A.CALL_NONE] and plan(pile3, call3, 16)[1] == 0
    big = 0xFFFFFFFF
    pile4, call4, _, _ = hand_rows([[big, big, 0, 0, 0, big, big, 0]], "A")
    assert call4[0] & A.CALL_INS == 0
    pile4[0, 1] = 0
    call4 = reference_call(pile4, np.frombuffer(b"A", np.uint8), np.array([0, 1], np.uint64), 1)[0]
    assert call4[0] & A.CALL_INS and plan(pile4, call4, 16)[0].tolist() == [1]   # (2^33 - 3) // (2^32 - 1) = 1


def test_slot_count_formula_around_the_half():
    slot_count_cases(reference_ins_plan)


def hand_consensus(consensus, rows, own, ins_len, ins, reads=None, min_depth=1):
    pile = np.array(rows, np.uint32)
    bases, off = batch(reads if reads is not None else [own])
    call, _ = reference_call(pile, bases, off, min_depth)
    cons, coff = consensus(pile, call, np.array(ins_len, np.uint8), np.array(ins, np.uint32).reshape(-1, 4), bases, off)
    return np.asarray(cons).tobytes().decode(), np.asarray(coff).tolist()


def row_rule_cases(consensus):
    """the hand cases of the row rule; consensus(pile, call, ins_len, ins, bases, offsets) -> (cons_bases, cons_offsets):
    reference_consensus here, the device in tests/test_gpu_pile_consensus.py"""
    def consensus_by_hand(*args, **kw):
        return hand_consensus(consensus, *args, **kw)
    #         A  C  G  T DEL INS INSB
    rows = [[3, 0, 0, 0, 0, 0, 0, 0],   # own a: called A, upper case
            [0, 0, 0, 0, 3, 2, 2, 0],   # called DEL, with an insertion behind it: the base goes, the inserted letter stays
            [0, 3, 0, 0, 0, 0, 0, 0],   # own G, called C
            [0, 0, 0, 0, 0, 0, 0, 0],   # no call: own n verbatim
            [0, 0, 0, 3, 0, 2, 4, 0]]   # the last base of the read, two slots
    ins = [[0, 0, 2, 0], [0, 1, 0, 1], [2, 0, 0, 0]]  # G; then a tie C / T -> C; then A
    assert consensus_by_hand(rows, "aAGnT", [0, 1, 0, 0, 2], ins) == ("AG" "C" "n" "TCA", [0, 7])
    # the same rows as three reads, one of them empty: the offsets follow the rows
    assert consensus_by_hand(rows, None, [0, 1, 0, 0, 2], ins, reads=["aA", "", "GnT"])[1] == [0, 2, 2, 7]
    # every row of a read called DEL: the read comes out empty
    assert consensus_by_hand([[0, 0, 0, 0, 2, 0, 0, 0]] * 2 + [[2, 0, 0, 0, 0, 0, 0, 0]], None, [0, 0, 0], [], reads=["CC", "A"]) == ("A", [0, 0, 1])
    # below min_depth nothing is corrected, N and lower case pass through
    assert consensus_by_hand([[0, 2, 0, 0, 0, 0, 0, 0]] * 3, "Nax", [0, 0, 0], [], min_depth=3) == ("Nax", [0, 3])


def emission_cases(consensus):
    def consensus_by_hand(*args, **kw):
        return hand_consensus(consensus, *args, **kw)
    # depth 4: a slot needs 3 votes.  Slots with 3, 2, 4 votes: only the first is emitted although the third has the votes
    rows = [[4, 0, 0, 0, 0, 3, 9, 0]]
    assert consensus_by_hand(rows, "A", [3], [[0, 3, 0, 0], [1, 1, 0, 0], [0, 0, 0, 4]]) == ("AC", [0, 2])
    assert consensus_by_hand(rows, "A", [3], [[0, 2, 0, 0], [3, 0, 0, 0], [0, 0, 0, 4]]) == ("A", [0, 1])
    assert consensus_by_hand(rows, "A", [3], [[0, 3, 0, 0], [1, 1, 1, 0], [0, 0, 0, 4]]) == ("ACAT", [0, 4])  # 1 1 1 0: the smallest code
    # exactly half is not enough
    assert consensus_by_hand(rows, "A", [1], [[0, 2, 0, 0]]) == ("A", [0, 1])


def test_consensus_row_rules():
    row_rule_cases(reference_consensus)


def test_emission_stops_at_the_first_slot_that_fails():
    emission_cases(reference_consensus)


def test_references_on_random_chains():
    """the whole route on the references: an insertion every partner has comes out, and the votes respect the slots"""
    rng = np.random.default_rng(50)
    # read 0 lacks GT behind its base 9; five partners have it (as D runs seen from read 0)
    truth = "".join(rng.choice(list("ACGT"), 30))
    short = truth[:10] + truth[12:]
    bases, off = batch([short] + [truth] * 5)
    chains = chain_recs([(0, r, 0, 0, 28, 0, 30) for r in range(1, 6)])
    aln = np.zeros(5, ALN)
    aln["flags"] = PATH
    runs = [run_word(10, "="), run_word(2, "D"), run_word(18, "=")]
    ops, op_off = np.array(runs * 5, np.uint32), np.arange(6, dtype=np.uint64) * 3
    cons, coff, pile, call, ins_len, ins = reference_correct(chains, aln, ops, op_off, bases, off, min_depth=3)
    assert ins_len[9] == 3 and ins_len.sum() == 3   # (2 * 10 - 1) // 5 = 3 slots; the partners fill two
    assert ins[:3].tolist() == [[5 if x == "ACGT".index(truth[10 + k]) else 0 for x in range(4)] for k in range(2)] + [[0, 0, 0, 0]]
    assert cons[int(coff[0]):int(coff[1])].tobytes().decode() == truth and coff.tolist()[1:] == [30 * r for r in range(1, 7)]
    # random run lists: every vote falls inside the slots of its row, and their number is what the runs give
    for seed in range(5):
        case = synth_chains(rng, [random_runs(rng, int(rng.integers(1, 60))) for _ in range(12)], [c & 1 for c in range(12)], shared_a=(0, 2))
        ins_len = rng.integers(0, 4, case[4].size).astype(np.uint8)
        ins, _ = reference_ins_votes(*case, ins_len)
        assert ins.shape == (int(ins_len.sum()), 4)
        q, db = reference_ins_votes(*case, ins_len, case[4], case[5], ins_len)
        assert (q + db == ins).all() and q.any() and db.any()


# ---- the symbols and their surroundings -------------------------------------------------------------------------------------------
def test_symbols_and_bindings():
    """fails without the feature: the symbols are missing"""
    L = lib.load()
    for name in ("kmu_pile_ins_plan", "kmu_chain_pile_ins", "kmu_pile_consensus"):
        assert name in lib.SYMBOLS and hasattr(L, name)
    assert len(L.kmu_pile_ins_plan.argtypes) == 8 and len(L.kmu_chain_pile_ins.argtypes) == 21 and len(L.kmu_pile_consensus.argtypes) == 15
    assert callable(lib.Context.pile_ins_plan) and callable(lib.Context.chain_pile_ins) and callable(lib.Context.pile_consensus)
    assert callable(minimizer.insertions_chains) and callable(minimizer.consensus_reads) and callable(minimizer.correct_reads)


def test_constants_and_struct_sizes_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()

    def define(name):
        return int(re.search(r"#define %s\s+(\d+)u?\s" % name, txt).group(1))
    assert define("KMU_INS_COLS") == A.INS_COLS == 4 and define("KMU_INS_MAX") == A.INS_MAX == 255
    assert C.sizeof(A.InsPlanParams) == 8 and C.sizeof(A.ConsensusParams) == 4
    assert [n for n, _ in A.InsPlanParams._fields_] == re.findall(r"uint32_t (\w+);", re.search(r"typedef struct kmu_ins_plan_params \{(.*?)\}", txt, re.S).group(1))
    assert [n for n, _ in A.ConsensusParams._fields_] == re.findall(r"uint32_t (\w+);", re.search(r"typedef struct kmu_consensus_params \{(.*?)\}", txt, re.S).group(1))
    tail = txt[txt.index("} kmu_read_pile;"):]
    assert tail.index("int kmu_pile_call(") < tail.index("int kmu_pile_ins_plan(") < tail.index("int kmu_chain_pile_ins(") < tail.index("int kmu_pile_consensus(")
    assert "does not collect the inserted letters" not in txt
    core = open(os.path.join(ROOT, "kmerutils_amd", "csrc", "kmu_cons_core.h")).read()
    assert int(re.search(r"constexpr uint32_t CONS_BLOCK = (\d+);", core).group(1)) == 64
    assert int(re.search(r"constexpr uint32_t CONS_MAX_INS = (\d+);", core).group(1)) == A.INS_MAX
    # the check and tile step of the pileup exists once
    csrc = os.path.join(ROOT, "kmerutils_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if "k_pile_starts," in open(os.path.join(csrc, f)).read()]
    assert users == ["kmu_chain_pileup.hip"]


def test_refusals_that_need_no_device():
    L = lib.load()
    arr = np.zeros(64, np.uint8)
    a = arr.ctypes.data
    n = C.c_uint64(99)
    plan, sides, cons = A.InsPlanParams(16, 0), A.PileupParams(3), A.ConsensusParams(0)
    assert L.kmu_pile_ins_plan(None, a, a, 1, C.byref(plan), A.MEM_HOST, a, C.byref(n)) == A.E_BAD_ARG
    assert L.kmu_pile_ins_plan(None, None, None, 0, None, 7, None, None) == A.E_BAD_ARG
    assert L.kmu_chain_pile_ins(None, a, 1, a, a, a, 1, a, a, 1, a, a, 1, C.byref(sides), A.MEM_HOST, a, 0, a, a, 0, a) == A.E_BAD_ARG
    assert L.kmu_chain_pile_ins(None, None, 1, None, None, None, 0, None, None, 1, None, None, 1, None, A.MEM_HOST, None, 0, None, None, 0, None) == A.E_BAD_ARG
    assert L.kmu_pile_consensus(None, a, a, a, 0, a, a, a, 1, C.byref(cons), A.MEM_HOST, a, a, 64, C.byref(n)) == A.E_BAD_ARG
    assert L.kmu_pile_consensus(None, None, None, None, 0, None, None, None, 0, None, 7, None, None, 0, None) == A.E_BAD_ARG
    assert not arr.any() and n.value == 99


# ---- the wrappers on a stub context -----------------------------------------------------------------------------------------------
class _StubContext:
    def chain_pileup(self, *args, **kw):
        self.piled = args + (kw,)
        return "pile", "pile"

    def pile_call(self, pile, bases, offsets, min_depth=3):
        self.called = (pile, bases, offsets, min_depth)
        return "call", "reads"

    def pile_ins_plan(self, pile, call, max_ins=16):
        self.planned = (pile, call, max_ins)
        return "len", 11

    def chain_pile_ins(self, chains, aln, ops, op_offsets, bases_q, offsets_q, ins_len_q, n_slots_q, bases_db=None, offsets_db=None,
                       ins_len_db=None, n_slots_db=None, sides=3, into=None):
        self.voted = (chains, aln, ops, op_offsets, bases_q, offsets_q, ins_len_q, n_slots_q, bases_db, offsets_db, ins_len_db, n_slots_db, sides, into)
        return "ins", "ins"

    def pile_consensus(self, pile, call, ins_len, n_slots, ins, bases, offsets):
        self.written = (pile, call, ins_len, n_slots, ins, bases, offsets)
        return "cons", "coff"


def test_wrappers_pass_everything_on(monkeypatch):
    stub = _StubContext()
    assert minimizer.insertions_chains(stub, "ch", "aln", "ops", "off", "bq", "oq", "lq", 5) == ("ins", "ins")
    assert stub.voted == ("ch", "aln", "ops", "off", "bq", "oq", "lq", 5, None, None, None, None, A.PILE_Q | A.PILE_DB, None)
    minimizer.insertions_chains(stub, "ch", "aln", "ops", "off", "bq", "oq", "lq", 5, "bdb", "odb", "ldb", 6, sides=A.PILE_DB, into="t")
    assert stub.voted == ("ch", "aln", "ops", "off", "bq", "oq", "lq", 5, "bdb", "odb", "ldb", 6, A.PILE_DB, "t")
    assert minimizer.consensus_reads(stub, "pile", "call", "len", 11, "ins", "b", "o") == ("cons", "coff")
    assert stub.written == ("pile", "call", "len", 11, "ins", "b", "o")
    seen = {}

    def read_cigars(ctx, bases, offsets, k, w, *rest):
        seen["args"] = (ctx, bases, offsets, k, w) + rest
        return "ch", "aln", "ops", "off"
    monkeypatch.setattr(minimizer, "read_cigars", read_cigars)
    assert minimizer.correct_reads(stub, "b", "o", 15, 10, band=32, min_depth=2, max_ins=7) == ("cons", "coff", "reads")
    assert seen["args"] == (stub, "b", "o", 15, 10, A.FHASH_CANON_INVHASH, 0, 5000, 500, 3, 0, 32, 0)
    assert stub.piled[:6] == ("ch", "aln", "ops", "off", "b", "o")
    assert stub.called == ("pile", "b", "o", 2) and stub.planned == ("pile", "call", 7)
    assert stub.voted == ("ch", "aln", "ops", "off", "b", "o", "len", 11, None, None, None, None, A.PILE_Q | A.PILE_DB, None)
    assert stub.written == ("pile", "call", "len", 11, "ins", "b", "o")
