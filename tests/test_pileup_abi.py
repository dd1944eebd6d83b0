"""-m "not gpu": the host side of the read pileup -- `reference_pileup` and `reference_call`: the contracts of kmu_chain_pileup and
kmu_pile_call (include/kmu.h) as plain numpy, one replay loop per chain, which tests/test_gpu_chain_pileup.py compares the device
against; `synth_chains`, which makes chains, records and reads from run lists without an aligner; the symbols and their bindings,
the constants and struct sizes, refusals that need no device, and the minimizer wrappers on a stub context.  The references are
checked here by the single-chain depth identity, by column sums on chains made by reference_cigar, and on hand-made cases."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import ALN, batch, chain_recs, revcomp  # noqa: E402
from test_chain_cigar_abi import CODE, reference_cigar, sums  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_PILE = np.dtype(A.READ_PILE_DTYPE)
PATH = A.ALN_DONE | A.ALN_EXACT | A.ALN_PATH
LETTER_CODE = np.full(256, 5, np.int64)  # 5: outside ACGTacgt
for _k, _c in enumerate("ACGT"):
    LETTER_CODE[ord(_c)] = LETTER_CODE[ord(_c.lower())] = _k


class NonACGT(Exception):
    pass


# ---- the references ---------------------------------------------------------------------------------------------------------------
def reference_pileup(chains, aln, ops, op_offsets, bases_q, offsets_q, bases_db=None, offsets_db=None, sides=A.PILE_Q | A.PILE_DB, into=None):
    """(pile_q, pile_db) of kmu_chain_pileup by the text of include/kmu.h (valid input only): uint32 [n_bases, 8]; one shared table
    in the self-join; into=(pile_q, pile_db) accumulates; NonACGT for a voted letter outside ACGTacgt"""
    own = bases_db is None
    if own:
        bases_db, offsets_db = bases_q, offsets_q
    if into is not None:
        pile_q, pile_db = into
    else:
        pile_q = np.zeros((int(offsets_q[-1]), A.PILE_COLS), np.uint32)
        pile_db = pile_q if own else np.zeros((int(offsets_db[-1]), A.PILE_COLS), np.uint32)
    ops, off = np.asarray(ops).astype(np.int64) & 0xFFFFFFFF, np.asarray(op_offsets).astype(np.int64)
    vote_q, vote_db = bool(sides & A.PILE_Q), bool(sides & A.PILE_DB)
    for c, rec in enumerate(chains):
        runs = ops[off[c]:off[c + 1]]
        if not int(aln[c]["flags"]) & A.ALN_PATH:
            assert runs.size == 0
            continue
        a0, a1, b0, b1, s = (int(rec[f]) for f in ("a_start", "a_end", "b_start", "b_end", "strand"))
        m, n = a1 - a0, b1 - b0
        row_a = int(offsets_q[rec["read_a"]]) + a0          # the row of A's base 0
        beg_b = int(offsets_db[rec["read_b"]])

        def rows_b(j, length):  # the rows of B' bases j .. j + length - 1
            k = np.arange(j, j + length, dtype=np.int64)
            return beg_b + (b1 - 1 - k if s else b0 + k)
        i = j = 0
        for v in runs.tolist():
            length, op = v >> 4, v & 15
            assert length > 0 and op in (1, 2, 7, 8)
            if op in (7, 8):
                ra, rb = row_a + np.arange(i, i + length, dtype=np.int64), rows_b(j, length)
                if vote_q:
                    code = LETTER_CODE[bases_db[rb]]
                    if (code == 5).any():
                        raise NonACGT()
                    np.add.at(pile_q, (ra, 3 - code if s else code), 1)
                if vote_db:
                    code = LETTER_CODE[bases_q[ra]]
                    if (code == 5).any():
                        raise NonACGT()
                    np.add.at(pile_db, (rb, 3 - code if s else code), 1)
                i, j = i + length, j + length
            elif op == 1:  # I: bases of A only
                if vote_q:
                    pile_q[row_a + i:row_a + i + length, A.PILE_DEL] += 1
                if vote_db:
                    at = (j if j < n else None) if s else (j - 1 if j > 0 else None)  # the base before the gap, forwards on read b
                    if at is not None:
                        pile_db[rows_b(at, 1)[0], A.PILE_INS] += 1
                        pile_db[rows_b(at, 1)[0], A.PILE_INS_BASES] += length
                i += length
            else:  # D: bases of B' only
                if vote_db:
                    np.add.at(pile_db, (rows_b(j, length), A.PILE_DEL), 1)
                if vote_q and i > 0:
                    pile_q[row_a + i - 1, A.PILE_INS] += 1
                    pile_q[row_a + i - 1, A.PILE_INS_BASES] += length
                j += length
        assert (i, j) == (m, n)
        if vote_q and m:
            pile_q[row_a, A.PILE_ENDS] += 1
            pile_q[row_a + m - 1, A.PILE_ENDS] += 1
        if vote_db and n:
            pile_db[beg_b + b0, A.PILE_ENDS] += 1
            pile_db[beg_b + b1 - 1, A.PILE_ENDS] += 1
    return pile_q, pile_db


def reference_call(pile, bases, offsets, min_depth=3):
    """(call uint8 [n_bases], reads READ_PILE [n_reads]) of kmu_pile_call by the text of include/kmu.h"""
    cnt = np.asarray(pile).astype(np.int64)[:, :5] & 0xFFFFFFFF
    ins = np.asarray(pile).astype(np.int64)[:, A.PILE_INS] & 0xFFFFFFFF
    g = np.arange(cnt.shape[0])
    depth = cnt.sum(axis=1)
    best = cnt.argmax(axis=1) if cnt.shape[0] else np.zeros(0, np.int64)  # the first of the largest: the smallest code
    own = LETTER_CODE[np.asarray(bases)]
    tied = (own < 5) & (cnt[g, np.minimum(own, 4)] == cnt[g, best])
    best = np.where(tied, own, best)
    called = depth >= min_depth
    call = np.where(called, best | np.where(2 * ins > depth, A.CALL_INS, 0) | np.where(best != own, A.CALL_DIFF, 0), A.CALL_NONE).astype(np.uint8)
    reads = np.zeros(len(offsets) - 1, READ_PILE)
    for r in range(len(offsets) - 1):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        cl, ok = call[lo:hi], called[lo:hi]
        reads[r] = (hi - lo, ok.sum(), (ok & ((cl & A.CALL_DIFF) != 0)).sum(), (ok & ((cl & 7) == A.PILE_DEL)).sum(),
                    (ok & ((cl & A.CALL_INS) != 0)).sum(), min(int(depth[lo:hi].max()), 0xFFFFFFFF) if hi > lo else 0, depth[lo:hi].sum())
    return call, reads


# ---- chains from run lists, without an aligner -------------------------------------------------------------------------------------
def run_word(length, letter):
    return length << 4 | CODE[letter]


def runs_mn(runs):
    """(m, n) of a list of (length, letter) runs"""
    return (sum(k for k, x in runs if x in "=XI"), sum(k for k, x in runs if x in "=XD"))


def synth_chains(rng, run_lists, strands, pad=3, lower=False, shared_a=None):
    """one chain per run list ((length, letter) pairs): read 2 c holds its A segment and read 2 c + 1 its B segment, each with `pad`
    bases before and behind, random letters (no bases are compared).  shared_a=(read, start): every A segment starts there on one
    read instead.  Returns (chains, aln, ops, op_offsets, bases, offsets); aln has DONE | EXACT | PATH"""
    reads, rows, ops, off = [], [], [], [0]
    letters = list("acgt" if lower else "ACGT")
    if shared_a is not None:
        longest = max(runs_mn(r)[0] for r in run_lists)
        reads.append("".join(rng.choice(letters, shared_a[1] + longest + pad)))
    for runs, s in zip(run_lists, strands):
        m, n = runs_mn(runs)
        if shared_a is None:
            reads.append("".join(rng.choice(letters, m + 2 * pad)))
            ra, a0 = len(reads) - 1, pad
        else:
            ra, a0 = 0, shared_a[1]
        reads.append("".join(rng.choice(letters, n + 2 * pad)))
        rows.append((ra, len(reads) - 1, s, a0, a0 + m, pad, pad + n))
        ops += [run_word(k, x) for k, x in runs]
        off.append(len(ops))
    bases, offsets = batch(reads)
    chains = chain_recs(rows)
    aln = np.zeros(len(rows), ALN)
    aln["flags"], aln["n_diags"] = PATH, 129
    return chains, aln, np.array(ops, np.uint32), np.array(off, np.uint64), bases, offsets


def random_runs(rng, n_runs, max_len=12):
    """n_runs runs with random ops (adjacent runs may share an op: a cut run) and lengths 1 .. max_len"""
    return [(int(rng.integers(1, max_len + 1)), "=XID"[int(rng.integers(0, 4))]) for _ in range(n_runs)]


def depth_of(pile):
    return pile[:, :5].astype(np.int64).sum(axis=1)


# ---- the references against themselves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strand", [0, 1])
def test_single_chain_depth_is_one_on_the_segment(strand):
    rng = np.random.default_rng(40 + strand)
    for n_runs in (1, 2, 7, 40):
        chains, aln, ops, off, bases, offsets = synth_chains(rng, [random_runs(rng, n_runs)], [strand], pad=4)
        pq, pdb = reference_pileup(chains, aln, ops, off, bases, offsets, bases, offsets)  # two tables of one batch
        rec = chains[0]
        for pile, read, lo, hi in ((pq, rec["read_a"], rec["a_start"], rec["a_end"]), (pdb, rec["read_b"], rec["b_start"], rec["b_end"])):
            want = np.zeros(pile.shape[0], np.int64)
            want[int(offsets[read]) + int(lo):int(offsets[read]) + int(hi)] = 1
            assert (depth_of(pile) == want).all()
            assert pile[:, A.PILE_ENDS].sum() == (2 if hi > lo else 0)
        shared, same = reference_pileup(chains, aln, ops, off, bases, offsets)
        assert shared is same and (shared == pq + pdb).all()
        assert (minimizer.pile_depth(shared) == depth_of(shared)).all()


def test_column_sums_of_aligned_chains():
    rng = np.random.default_rng(41)
    for rep in range(30):
        a = "".join(rng.choice(list("ACGT"), int(rng.integers(20, 60))))
        b = list(a)
        for _ in range(4):
            at = int(rng.integers(0, len(b)))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                b[at] = "ACGT"[("ACGT".index(b[at]) + 1) % 4]
            elif kind == 1:
                del b[at]
            else:
                b.insert(at, "ACGT"[int(rng.integers(0, 4))])
        if rep % 5 == 0:
            b = list("GG") + b  # a leading D run
        b, s = "".join(b), rep & 1
        bases, off = batch([a, revcomp(b) if s else b])
        chains = chain_recs([(0, 1, s, 0, len(a), 0, len(b))])
        aln, ops, op_off = reference_cigar(chains, bases, off, band=8)
        pq, pdb = reference_pileup(chains, aln, ops, op_off, bases, off, bases, off)
        tot = sums(ops)
        own = LETTER_CODE[bases]
        assert pq[np.arange(len(a)), own[:len(a)]].sum() == aln[0]["matches"] == tot["="]
        assert pdb[np.arange(len(a), len(bases)), own[len(a):]].sum() == aln[0]["matches"]
        lead_d = int(ops[0]) >> 4 if ops.size and int(ops[0]) & 15 == 2 else 0
        assert pq[:, A.PILE_DEL].sum() == tot["I"] and pq[:, A.PILE_INS_BASES].sum() == tot["D"] - lead_d
        assert pdb[:, A.PILE_DEL].sum() == tot["D"] and pq[:, A.PILE_INS].sum() == sum(1 for v in ops[1 if lead_d else 0:] if v & 15 == 2)


def by_hand(a, b, runs, strand):
    """the two tables (rows of read a, rows of read b) of one whole-read chain with the given runs"""
    bases, off = batch([a, b])
    chains = chain_recs([(0, 1, strand, 0, len(a), 0, len(b))])
    aln = np.zeros(1, ALN)
    aln["flags"] = PATH
    ops = np.array([run_word(k, x) for k, x in runs], np.uint32)
    pile, _ = reference_pileup(chains, aln, ops, np.array([0, len(ops)], np.uint64), bases, off)
    return pile[:len(a)].tolist(), pile[len(a):].tolist()


def test_hand_cases():
    #          A  C  G  T  DEL INS INSB ENDS
    assert by_hand("AA", "A", [(1, "I"), (1, "=")], 0) == ([[0, 0, 0, 0, 1, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0, 1]], [[1, 0, 0, 0, 0, 0, 0, 2]])
    # the same runs the other way round: the gap now has read b's base before it
    assert by_hand("AA", "A", [(1, "="), (1, "I")], 0) == ([[1, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 1, 0, 0, 1]], [[1, 0, 0, 0, 0, 1, 1, 2]])
    # strand 1: B' = A is read b = T backwards; A votes its complement T; an I run at j = 0 < n votes on B' index 0 ...
    assert by_hand("AA", "T", [(1, "I"), (1, "=")], 1) == ([[0, 0, 0, 0, 1, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0, 1]], [[0, 0, 0, 1, 0, 1, 1, 2]])
    # ... and at j = n on nothing
    assert by_hand("AA", "T", [(1, "="), (1, "I")], 1) == ([[1, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 1, 0, 0, 1]], [[0, 0, 0, 1, 0, 0, 0, 2]])
    # a leading D votes no INS on A, a trailing D on A's last base
    assert by_hand("AC", "GAC", [(1, "D"), (2, "=")], 0) == ([[1, 0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 0, 1]],
                                                            [[0, 0, 0, 0, 1, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 1]])
    assert by_hand("AC", "ACG", [(2, "="), (1, "D")], 0)[0] == [[1, 0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1, 1, 1]]
    # strand 1 over three bases: A = ACG against read b = CGT (B' = ACG); A's row i takes B's forward letter complemented
    assert by_hand("ACG", "CGT", [(3, "=")], 1) == ([[1, 0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 1]],
                                                   [[0, 1, 0, 0, 0, 0, 0, 1], [0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 1]])
    # empty segments: no ENDS on the empty side
    assert by_hand("", "ACG", [(3, "D")], 0) == ([], [[0, 0, 0, 0, 1, 0, 0, 1], [0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 1]])
    assert by_hand("ACG", "", [(3, "I")], 0) == ([[0, 0, 0, 0, 1, 0, 0, 1], [0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 1]], [])
    bases, off = batch(["ACG", "ACG"])
    chains = chain_recs([(0, 1, 0, 1, 1, 2, 2)])
    aln = np.zeros(1, ALN)
    aln["flags"] = PATH
    assert not reference_pileup(chains, aln, np.zeros(0, np.uint32), np.zeros(2, np.uint64), bases, off)[0].any()
    # a segment of one base: ENDS is 2; a cut run counts two INS
    assert by_hand("C", "G", [(1, "X")], 0) == ([[0, 0, 1, 0, 0, 0, 0, 2]], [[0, 1, 0, 0, 0, 0, 0, 2]])
    assert by_hand("A", "ACG", [(1, "="), (1, "D"), (1, "D")], 0)[0] == [[1, 0, 0, 0, 0, 2, 2, 2]]
    # a chain without PATH votes nothing
    aln["flags"] = A.ALN_DONE
    assert not reference_pileup(chain_recs([(0, 1, 0, 0, 3, 0, 3)]), aln, np.zeros(0, np.uint32), np.zeros(2, np.uint64), bases, off)[0].any()
    with pytest.raises(NonACGT):
        by_hand("AC", "AN", [(2, "=")], 0)


def test_call_ties_and_min_depth():
    #                 A  C  G  T  DEL INS
    rows = np.array([[2, 2, 0, 0, 0, 0, 0, 0],   # own C among the tied: C, no DIFF
                     [2, 2, 0, 0, 0, 0, 0, 0],   # own G not among them: the smallest, A, DIFF
                     [2, 2, 0, 0, 0, 0, 0, 0],   # own N: A, DIFF
                     [0, 0, 1, 0, 3, 3, 5, 0],   # DEL wins: always DIFF; 2 * 3 > 4: INS
                     [0, 0, 0, 2, 0, 2, 9, 0],   # depth 2 = min_depth - 1: not called
                     [0, 0, 0, 3, 0, 1, 9, 0],   # depth 3: called; 2 * 1 > 3 is false
                     [0, 0, 0, 0, 0, 0, 0, 0],
                     [1, 1, 1, 1, 1, 0, 0, 0]], np.uint32)  # own t (lower case) among five tied
    bases, off = batch(["CGNA", "", "TTAt"])
    call, reads = reference_call(rows, bases, off, 3)
    assert call.tolist() == [1, 0 | 16, 0 | 16, 4 | 8 | 16, 7, 3, 7, 3]
    assert reads.tolist() == [(4, 4, 3, 1, 1, 4, 16), (0, 0, 0, 0, 0, 0, 0), (4, 2, 0, 0, 0, 5, 10)]
    call1, reads1 = reference_call(rows, bases, off, 1)
    assert call1.tolist() == [1, 16, 16, 28, 3 | 8, 3, 7, 3] and reads1["covered"].tolist() == [4, 0, 3] and reads1["n_ins"].tolist() == [1, 0, 1]
    assert reads1["depth_sum"].tolist() == reads["depth_sum"].tolist()


# ---- the symbols and their surroundings -------------------------------------------------------------------------------------------
def test_symbols_and_bindings():
    """fails without the feature: the symbols are missing"""
    L = lib.load()
    for name in ("kmu_chain_pileup", "kmu_pile_call"):
        assert name in lib.SYMBOLS and hasattr(L, name)
    assert len(L.kmu_chain_pileup.argtypes) == 17 and len(L.kmu_pile_call.argtypes) == 9
    assert callable(lib.Context.chain_pileup) and callable(lib.Context.pile_call)
    assert callable(minimizer.pileup_chains) and callable(minimizer.read_pileups) and callable(minimizer.pile_depth)


def test_constants_and_struct_sizes_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()

    def define(name):
        return int(re.search(r"#define %s\s+(\d+)u?\s" % name, txt).group(1))
    names = ["A", "C", "G", "T", "DEL", "INS", "INS_BASES", "ENDS"]
    assert [define("KMU_PILE_" + x) for x in names] == [getattr(A, "PILE_" + x) for x in names] == list(range(8))
    assert define("KMU_PILE_COLS") == A.PILE_COLS == 8 and A.PILE_COLS * 4 == 32
    assert (define("KMU_PILE_Q"), define("KMU_PILE_DB")) == (A.PILE_Q, A.PILE_DB) == (1, 2)
    assert (define("KMU_CALL_NONE"), define("KMU_CALL_INS"), define("KMU_CALL_DIFF")) == (A.CALL_NONE, A.CALL_INS, A.CALL_DIFF) == (7, 8, 16)
    rec = re.search(r"typedef struct \{\s*/\* 32 bytes \*/(.*?)\} kmu_read_pile;", txt[txt.index("} kmu_pile_call_params;"):], re.S).group(1)
    fields = re.findall(r"uint(?:32|64)_t (\w+);", rec)
    assert fields == [n for n, _ in A.ReadPile._fields_] == list(READ_PILE.names)
    assert C.sizeof(A.ReadPile) == READ_PILE.itemsize == 32 and A.ReadPile.depth_sum.offset == READ_PILE.fields["depth_sum"][1] == 24
    assert C.sizeof(A.PileupParams) == 4 and C.sizeof(A.PileCallParams) == 8
    assert "int kmu_chain_pileup(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, const kmu_chain_aln *aln," in txt
    assert "int kmu_pile_call(kmu_ctx *ctx, const uint32_t *pile," in txt
    core = open(os.path.join(ROOT, "kmerutils_amd", "csrc", "kmu_pile_core.h")).read()
    assert int(re.search(r"constexpr uint32_t PILE_TILE = (\d+);", core).group(1)) == 64


def test_refusals_that_need_no_device():
    L = lib.load()
    arr = np.zeros(64, np.uint8)
    a = arr.ctypes.data
    p, pc = A.PileupParams(3), A.PileCallParams(3, 0)
    assert L.kmu_chain_pileup(None, a, 1, a, a, a, 1, a, a, 1, a, a, 1, C.byref(p), A.MEM_HOST, a, a) == A.E_BAD_ARG
    assert L.kmu_chain_pileup(None, None, 1, None, None, None, 0, None, None, 1, None, None, 1, None, A.MEM_HOST, None, None) == A.E_BAD_ARG
    assert L.kmu_pile_call(None, a, a, a, 1, C.byref(pc), A.MEM_HOST, a, a) == A.E_BAD_ARG
    assert L.kmu_pile_call(None, None, None, None, 0, None, 7, None, None) == A.E_BAD_ARG
    assert not arr.any()


# ---- the wrappers on a stub context -----------------------------------------------------------------------------------------------
class _StubContext:
    def chain_pileup(self, chains, aln, ops, op_offsets, bases_q, offsets_q, bases_db=None, offsets_db=None, sides=3, into=None):
        self.seen = (chains, aln, ops, op_offsets, bases_q, offsets_q, bases_db, offsets_db, sides, into)
        return "pile", "pile"

    def pile_call(self, pile, bases, offsets, min_depth=3, want=("call", "reads")):
        self.called = (pile, bases, offsets, min_depth, want)
        return "call", "reads"


def test_wrappers_pass_everything_on(monkeypatch):
    stub = _StubContext()
    assert minimizer.pileup_chains(stub, "ch", "aln", "ops", "off", "bq", "oq") == ("pile", "pile")
    assert stub.seen == ("ch", "aln", "ops", "off", "bq", "oq", None, None, A.PILE_Q | A.PILE_DB, None)
    minimizer.pileup_chains(stub, "ch", "aln", "ops", "off", "bq", "oq", "bdb", "odb", sides=A.PILE_DB, into="t")
    assert stub.seen == ("ch", "aln", "ops", "off", "bq", "oq", "bdb", "odb", A.PILE_DB, "t")
    seen = {}

    def read_cigars(ctx, bases, offsets, k, w, *rest):
        seen["args"] = (ctx, bases, offsets, k, w) + rest
        return "ch", "aln", "ops", "off"
    monkeypatch.setattr(minimizer, "read_cigars", read_cigars)
    assert minimizer.read_pileups(stub, "b", "o", 15, 10, band=32, min_depth=2) == ("ch", "aln", "pile", "call", "reads")
    assert seen["args"] == (stub, "b", "o", 15, 10, A.FHASH_CANON_INVHASH, 0, 5000, 500, 3, 0, 32, 0)
    assert stub.seen == ("ch", "aln", "ops", "off", "b", "o", None, None, A.PILE_Q | A.PILE_DB, None)
    assert stub.called == ("pile", "b", "o", 2, ("call", "reads"))
    table = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [0, 0, 0, 0, 0, 9, 9, 9]], np.uint32)
    assert minimizer.pile_depth(table).tolist() == [15, 0] and minimizer.pile_depth(table.view(np.int32)).tolist() == [15, 0]
