"""-m "not gpu": the host side of chain alignment -- the symbol and its bindings, the constants and the records, refusals that need
no device, minimizer.align_chains / read_alignments on a stub context, minimizer.paf_lines, and `reference_align`: the contract of
kmu_chain_align (include/kmu.h) as plain numpy, which tests/test_gpu_chain_align.py compares the device against.  The reference
sweeps anti-diagonals; it is checked here against a full-matrix brute force over tuples (edits, -matches) with the cells outside
the band infinite, against the unbanded full-matrix DP wherever it sets ALN_EXACT, on a case whose band is too narrow, and on
hand-made cases for the ties."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = np.dtype(A.CHAIN_DTYPE)
ALN = np.dtype(A.CHAIN_ALN_DTYPE)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s.upper()))


def batch(seqs):
    """(bases uint8, offsets uint64) of a list of strings"""
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer("".join(seqs).encode(), np.uint8).copy(), off


def chain_recs(rows):
    """rows of (read_a, read_b, strand, a_start, a_end, b_start, b_end) as A.CHAIN_DTYPE records (score 7, n_seeds 3, n_anchors 4)"""
    out = np.zeros(len(rows), CHAIN)
    for r, (ra, rb, s, a0, a1, b0, b1) in zip(out, rows):
        r["read_a"], r["read_b"], r["strand"], r["a_start"], r["a_end"], r["b_start"], r["b_end"] = ra, rb, s, a0, a1, b0, b1
        r["score"], r["n_seeds"], r["n_anchors"] = 7, 3, 4
    return out


# ---- the reference --------------------------------------------------------------------------------------------------------------
K = 1 << 32    # a key is edits * K - matches: the smaller key is the lexicographic minimum of (edits, -matches), matches < K
INF = 1 << 62


def banded_key(a, b, band):
    """the key of cell (m, n); a, b: uint8 arrays of upper-case letters.  Anti-diagonal t holds the cells (i, t - i); the arrays are
    indexed by i + 1, so that row -1 reads as infinite"""
    m, n = len(a), len(b)
    lo, hi = min(0, n - m) - band, max(0, n - m) + band
    a, b = np.append(a, 1).astype(np.int64), np.append(b, 2).astype(np.int64)  # (a pad each, so that an empty segment can be indexed)
    p2, p1, cur = (np.full(m + 2, INF, np.int64) for _ in range(3))
    for t in range(m + n + 1):
        i0, i1 = max(0, t - n, -((hi - t) // 2)), min(m, t, (t - lo) // 2)  # rows of the anti-diagonal inside matrix and band
        cur.fill(INF)
        if i0 <= i1:
            i = np.arange(i0, i1 + 1, dtype=np.int64)
            j = t - i
            left, up = p1[i0 + 1:i1 + 2] + K, p1[i0:i1 + 1] + K  # from (i, j - 1) and from (i - 1, j)
            dg = p2[i0:i1 + 1] + np.where(a[np.maximum(i - 1, 0)] == b[np.maximum(j - 1, 0)], -1, K)
            v = np.minimum(np.minimum(left, up), dg)
            v = np.where(j == 0, i * K, v)
            cur[i0 + 1:i1 + 2] = np.where(i == 0, j * K, v)
        p2, p1, cur = p1, cur, p2
    return int(p1[m + 1])


def segments(rec, bases_q, offsets_q, bases_db, offsets_db):
    """the two segments of a chain record as upper-case uint8 arrays, B reverse-complemented on strand 1"""
    ba, bb = int(offsets_q[rec["read_a"]]), int(offsets_db[rec["read_b"]])
    a = bases_q[ba + int(rec["a_start"]):ba + int(rec["a_end"])] & 0xDF
    b = bases_db[bb + int(rec["b_start"]):bb + int(rec["b_end"])] & 0xDF
    if rec["strand"]:
        b = np.frombuffer(revcomp(b.tobytes().decode()).encode(), np.uint8)
    return a, b


def reference_align(chains, bases_q, offsets_q, bases_db=None, offsets_db=None, band=64):
    """the records of kmu_chain_align as a structured array of A.CHAIN_ALN_DTYPE, by the text of include/kmu.h (valid input only)"""
    if bases_db is None:
        bases_db, offsets_db = bases_q, offsets_q
    out = np.zeros(len(chains), ALN)
    for rec, o in zip(chains, out):
        a, b = segments(rec, bases_q, offsets_q, bases_db, offsets_db)
        m, n = len(a), len(b)
        n_diags = abs(n - m) + 2 * band + 1
        if n_diags > A.ALIGN_MAX_DIAGS:
            o["edit"], o["matches"], o["n_diags"], o["flags"] = 0xFFFFFFFF, 0, n_diags, 0
            continue
        key = banded_key(a, b, band)
        edit = (key + K - 1) // K
        o["edit"], o["matches"], o["n_diags"] = edit, edit * K - key, n_diags
        o["flags"] = A.ALN_DONE | (A.ALN_EXACT if edit - abs(n - m) <= 2 * band else 0)
    return out


def full_matrix(a, b, band=None):
    """(edits, matches) of cell (m, n) by the full matrix over tuples; band=None: the unbanded problem.  Shares no code with
    banded_key"""
    m, n = len(a), len(b)
    lo, hi = (-m, n) if band is None else (min(0, n - m) - band, max(0, n - m) + band)
    D = [[None] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        for j in range(n + 1):
            if not lo <= j - i <= hi:
                continue
            if i == 0 and j == 0:
                D[0][0] = (0, 0)
                continue
            cand = []
            if i and D[i - 1][j] is not None:
                cand.append((D[i - 1][j][0] + 1, D[i - 1][j][1]))
            if j and D[i][j - 1] is not None:
                cand.append((D[i][j - 1][0] + 1, D[i][j - 1][1]))
            if i and j and D[i - 1][j - 1] is not None:
                e, nm = D[i - 1][j - 1]
                cand.append((e, nm - 1) if a[i - 1] == b[j - 1] else (e + 1, nm))
            D[i][j] = min(cand)
    return D[m][n][0], -D[m][n][1]


def one(a, b, band, strand=0):
    """the reference's record for the strings a (read 0) and b (read 1) taken whole"""
    bases, off = batch([a, b])
    return reference_align(chain_recs([(0, 1, strand, 0, len(a), 0, len(b))]), bases, off, band=band)[0]


def test_reference_equals_the_full_matrix():
    rng = np.random.default_rng(11)
    n_exact = 0
    for rep in range(150):
        alpha = "AC" if rep % 2 else "ACGT"
        m, n, band = int(rng.integers(0, 41)), int(rng.integers(0, 41)), int(rng.integers(0, 9))
        if rep % 10 == 0:
            m = 0
        if rep % 10 == 5:
            n = 0
        a = "".join(rng.choice(list(alpha), m))
        b = "".join(rng.choice(list(alpha), n))
        if rep % 3 == 0 and m and n:  # related strings: b is a with a few edits
            b = a[:n // 2] + "".join(rng.choice(list(alpha), 2)) + a[n // 2 + 1:]
            n = len(b)
        rec = one(a, b, band)
        assert (int(rec["edit"]), int(rec["matches"])) == full_matrix(a, b, band), (a, b, band)
        assert rec["n_diags"] == abs(n - m) + 2 * band + 1 and rec["flags"] & A.ALN_DONE
        if rec["flags"] & A.ALN_EXACT:
            n_exact += 1
            assert (int(rec["edit"]), int(rec["matches"])) == full_matrix(a, b), (a, b, band)
        else:
            assert int(rec["edit"]) - abs(n - m) > 2 * band and int(rec["edit"]) >= full_matrix(a, b)[0]
    assert 20 < n_exact < 150  # both kinds were seen


def narrow_band_case():
    """A = P X Q S and B = P Q Y S with 12 random bases X and Y: m = n, and the unbanded optimum shifts by 12 diagonals across Q"""
    rng = np.random.default_rng(5)
    p, x, q, y, s = ("".join(rng.choice(list("ACGT"), k)) for k in (30, 12, 40, 12, 30))
    return p + x + q + s, p + q + y + s


def test_a_band_too_narrow_is_not_exact():
    a, b = narrow_band_case()
    assert len(a) == len(b)
    narrow, wide, free = one(a, b, 2), one(a, b, 16), full_matrix(a, b)
    assert narrow["flags"] == A.ALN_DONE and wide["flags"] == A.ALN_DONE | A.ALN_EXACT
    assert (int(wide["edit"]), int(wide["matches"])) == free and free[0] <= 24
    assert int(narrow["edit"]) > free[0] and (int(narrow["edit"]), int(narrow["matches"])) == full_matrix(a, b, 2)


# ---- ties by hand -----------------------------------------------------------------------------------------------------------------
# (a, b, band, strand, edit, matches); tests/test_gpu_chain_align.py runs the same on the device
HAND_CASES = [
    ("AAAAA", "AAAAAAAA", 1, 0, 3, 5),                      # homopolymers of two lengths: every placement of the gap ties
    ("AAAAAAAA", "AAAAA", 0, 0, 3, 5),
    ("ACACACAC", "CACACACA", 1, 0, 2, 7),                   # shifted by one: a deletion and an insertion, not eight mismatches
    ("ACACACAC", "CACACACA", 0, 0, 8, 0),                   # ... which is all a band of one diagonal leaves
    ("ACGTACGGTT", "ACGTCAGGTT", 2, 0, 2, 9),               # AC / CA: two mismatches or an insertion and a deletion; the latter matches one more
    ("ACGTTGCAAC", revcomp("ACGTTGCAAC"), 3, 1, 0, 10),     # strand 1 on a reverse complement
    ("ACGTTGCAAC", "GTTGCAACGT".lower(), 3, 1, 0, 10),      # (the same, written out, in lower case)
    ("acgtTGCAac", "ACGTtgcaAC", 0, 0, 0, 10),              # case does not matter
    ("", "ACG", 0, 0, 3, 0),
    ("ACG", "", 2, 0, 3, 0),
    ("", "", 0, 0, 0, 0),
]


@pytest.mark.parametrize("a,b,band,strand,edit,matches", HAND_CASES)
def test_ties_by_hand(a, b, band, strand, edit, matches):
    rec = one(a, b, band, strand)
    assert (int(rec["edit"]), int(rec["matches"])) == (edit, matches)
    assert rec["flags"] & A.ALN_DONE and rec["n_diags"] == abs(len(a) - len(b)) + 2 * band + 1


def test_a_band_too_wide_is_skipped():
    a, b = "A" * 3, "A" * (A.ALIGN_MAX_DIAGS + 3 - 2 * 4)
    rec = one(a, b, 4)
    assert rec.tolist() == (0xFFFFFFFF, 0, A.ALIGN_MAX_DIAGS + 1, 0)
    assert one(a, b[1:], 4)["flags"] == A.ALN_DONE | A.ALN_EXACT


# ---- the symbol and its surroundings ------------------------------------------------------------------------------------------------
def test_symbol_and_bindings():
    """fails without the feature: the symbol is missing"""
    L = lib.load()
    assert "kmu_chain_align" in lib.SYMBOLS and hasattr(L, "kmu_chain_align")
    assert len(L.kmu_chain_align.argtypes) == 12
    assert callable(getattr(lib.Context, "chain_align"))
    assert callable(minimizer.align_chains) and callable(minimizer.read_alignments) and callable(minimizer.paf_lines)


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    assert int(re.search(r"#define KMU_ALIGN_MAX_DIAGS (\d+)", txt).group(1)) == A.ALIGN_MAX_DIAGS
    assert int(re.search(r"#define KMU_ALIGN_CHUNK (\d+)", txt).group(1)) == A.ALIGN_CHUNK
    assert int(re.search(r"#define KMU_ALN_DONE\s+(\d+)u", txt).group(1)) == A.ALN_DONE == 1
    assert int(re.search(r"#define KMU_ALN_EXACT\s+(\d+)u", txt).group(1)) == A.ALN_EXACT == 2
    assert "int kmu_chain_align(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains," in txt
    rec = re.search(r"typedef struct \{\s*/\* 16 bytes \*/(.*?)\} kmu_chain_aln;", txt, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint32_t ([^;]+);", rec) for f in decl.split(",")]
    assert fields == [n for n, _ in A.CHAIN_ALN_DTYPE] == [n for n, _ in A.ChainAln._fields_] == ["edit", "matches", "n_diags", "flags"]
    assert C.sizeof(A.ChainAln) == 16 and ALN.itemsize == 16
    par = re.search(r"typedef struct kmu_align_params \{(.*?)\} kmu_align_params;", txt, re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", par) == [n for n, _ in A.AlignParams._fields_] == ["band", "flags"]
    assert C.sizeof(A.AlignParams) == 8
    # the kernel's chunk is the header's
    core = open(os.path.join(ROOT, "kmerutils_amd", "csrc", "kmu_align_core.h")).read()
    assert int(re.search(r"constexpr uint32_t ALIGN_CHUNK = (\d+);", core).group(1)) == A.ALIGN_CHUNK


def test_refusals_that_need_no_device():
    L = lib.load()
    arr = np.zeros(64, np.uint8)
    p = A.AlignParams(4, 0)
    a = arr.ctypes.data
    # no context: refused before anything is touched, whatever else is there
    assert L.kmu_chain_align(None, a, 1, a, a, 1, a, a, 1, C.byref(p), A.MEM_HOST, a) == A.E_BAD_ARG
    assert L.kmu_chain_align(None, None, 1, None, None, 1, None, None, 1, None, A.MEM_HOST, None) == A.E_BAD_ARG
    assert L.kmu_chain_align(None, a, 0, a, a, 1, a, a, 1, C.byref(p), A.MEM_HOST, a) == A.E_BAD_ARG
    assert not arr.any()


# ---- align_chains and read_alignments on a stub context ---------------------------------------------------------------------------
class _StubContext:
    def chain_align(self, chains, bases_q, offsets_q, bases_db=None, offsets_db=None, band=64):
        self.aligned = (chains, bases_q, offsets_q, bases_db, offsets_db, band)
        return "aln"


def test_align_chains_and_read_alignments_pass_the_batches_on(monkeypatch):
    stub = _StubContext()
    assert minimizer.align_chains(stub, "chains", "bq", "oq") == "aln"
    assert stub.aligned == ("chains", "bq", "oq", None, None, 64)
    minimizer.align_chains(stub, "chains", "bq", "oq", "bdb", "odb", band=9)
    assert stub.aligned == ("chains", "bq", "oq", "bdb", "odb", 9)
    seen = {}

    def read_chains(ctx, bases, offsets, k, w, *rest):
        seen["args"] = (ctx, bases, offsets, k, w) + rest
        return "chains"
    monkeypatch.setattr(minimizer, "read_chains", read_chains)
    assert minimizer.read_alignments(stub, "b", "o", 15, 10, band=32) == ("chains", "aln")
    assert seen["args"] == (stub, "b", "o", 15, 10, A.FHASH_CANON_INVHASH, 0, 5000, 500, 3, 0)
    assert stub.aligned == ("chains", "b", "o", None, None, 32)


# ---- PAF ----------------------------------------------------------------------------------------------------------------------------
def test_paf_lines():
    chains = chain_recs([(0, 2, 0, 10, 110, 5, 100), (1, 0, 1, 0, 50, 20, 75), (2, 1, 0, 0, 40, 0, 1200)])
    chains["score"], chains["n_seeds"] = [310, 45, 60], [9, 3, 4]
    aln = np.array([(7, 93, 134, 3), (2, 52, 134, 1), (0xFFFFFFFF, 0, 1289, 0)], ALN)
    off = np.array([0, 500, 560, 2000], np.uint64)
    names = ["r0", "r1", "r2"]
    lines = minimizer.paf_lines(chains, aln, names, off)
    assert lines == [
        "r0\t500\t10\t110\t+\tr2\t1440\t5\t100\t93\t100\t255\tNM:i:7\ts1:i:310\tcm:i:9",
        "r1\t60\t0\t50\t-\tr0\t500\t20\t75\t52\t54\t255\tNM:i:2\ts1:i:45\tcm:i:3",
        "r2\t1440\t0\t40\t+\tr1\t60\t0\t1200\t0\t1200\t255\ts1:i:60\tcm:i:4",
    ]
    # a database of its own numbers its reads independently
    lines = minimizer.paf_lines(chains[:1], aln[:1], names, off, ["t0", "t1", "t2"], np.array([0, 7, 9, 309], np.uint64))
    assert lines == ["r0\t500\t10\t110\t+\tt2\t300\t5\t100\t93\t100\t255\tNM:i:7\ts1:i:310\tcm:i:9"]
    assert minimizer.paf_lines(chains[:0], aln[:0], names, off) == []
