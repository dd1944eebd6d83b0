"""-m "not gpu": the host side of chain alignment paths -- `reference_cigar`: the contract of kmu_chain_cigar (include/kmu.h) as
plain numpy, which tests/test_gpu_chain_cigar.py compares the device against; the symbol and its bindings, the constants, refusals
that need no device, minimizer.cigar_chains / read_cigars on a stub context, minimizer.cigar_strings and paf_lines(cigar=...).
The reference keeps the banded values of the whole matrix and walks back by the value rule; it is checked here by the four sum
identities, by the equality of its records with reference_align apart from the PATH bit, by replaying its runs over the two
segments, and on hand-made cases for the ties."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import ALN, INF, K, batch, chain_recs, reference_align, revcomp, segments  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTER = {1: "I", 2: "D", 7: "=", 8: "X"}
CODE = {v: k for k, v in LETTER.items()}


# ---- the reference --------------------------------------------------------------------------------------------------------------
def banded_values(a, b, band):
    """V[i + 1, j + 1]: the key of cell (i, j) (test_chain_align_abi.banded_key's keys), INF outside the band; row 0 and column 0
    of V are INF, so that a neighbour outside the matrix reads as infinite"""
    m, n = len(a), len(b)
    lo, hi = min(0, n - m) - band, max(0, n - m) + band
    a1, b1 = np.append(a, 1).astype(np.int64), np.append(b, 2).astype(np.int64)
    V = np.full((m + 2, n + 2), INF, np.int64)
    for t in range(m + n + 1):
        i0, i1 = max(0, t - n, -((hi - t) // 2)), min(m, t, (t - lo) // 2)
        if i0 > i1:
            continue
        i = np.arange(i0, i1 + 1, dtype=np.int64)
        j = t - i
        dg = V[i, j] + np.where(a1[np.maximum(i - 1, 0)] == b1[np.maximum(j - 1, 0)], -1, K)
        v = np.minimum(np.minimum(V[i + 1, j] + K, V[i, j + 1] + K), dg)
        v = np.where(j == 0, i * K, v)
        V[i + 1, j + 1] = np.where(i == 0, j * K, v)
    return V


def walk_back(V, a, b):
    """the path as a string of = X I D in path order, by the rule of include/kmu.h: diagonal, then up, then left"""
    i, j, path = len(a), len(b), []
    V = V.tolist()
    a, b = a.tolist(), b.tolist()
    while i or j:
        if i == 0:
            path.append("D" * j)
            break
        if j == 0:
            path.append("I" * i)
            break
        v, eq = V[i + 1][j + 1], a[i - 1] == b[j - 1]
        if V[i][j] + (-1 if eq else K) == v:
            path.append("=" if eq else "X")
            i, j = i - 1, j - 1
        elif V[i][j + 1] + K == v:
            path.append("I")
            i -= 1
        else:
            assert V[i + 1][j] + K == v
            path.append("D")
            j -= 1
    return "".join(reversed(path))


def runs_of(path, max_run=A.CIGAR_MAX_RUN):
    """len << 4 | code per run; a run above max_run is cut, the remainder first"""
    out = []
    for mt in re.finditer(r"=+|X+|I+|D+", path):
        n, code = mt.end() - mt.start(), CODE[mt.group()[0]]
        if n % max_run:
            out.append((n % max_run) << 4 | code)
        out += [max_run << 4 | code] * (n // max_run)
    return out


def trace_bytes(m, n, band):
    """the bytes of a chain's direction bits (include/kmu.h: ceil(steps C / 8) * 256)"""
    lo = min(0, n - m) - band
    steps = (m + n + (lo & 1)) // 2 + 1
    nd = abs(n - m) + 2 * band + 1
    c = 1 if nd <= 128 else 2 if nd <= 256 else 4 if nd <= 512 else 8
    return (steps * c + 7) // 8 * 256


def reference_cigar(chains, bases_q, offsets_q, bases_db=None, offsets_db=None, band=64, max_trace_bytes=0):
    """(aln, ops, op_offsets) of kmu_chain_cigar by the text of include/kmu.h (valid input only): A.CHAIN_ALN_DTYPE records, uint32
    runs, uint64 offsets"""
    if bases_db is None:
        bases_db, offsets_db = bases_q, offsets_q
    budget = max_trace_bytes or A.CIGAR_TRACE_DEFAULT
    aln, ops, off = np.zeros(len(chains), ALN), [], np.zeros(len(chains) + 1, np.uint64)
    for c, (rec, o) in enumerate(zip(chains, aln)):
        a, b = segments(rec, bases_q, offsets_q, bases_db, offsets_db)
        m, n = len(a), len(b)
        n_diags = abs(n - m) + 2 * band + 1
        if n_diags > A.ALIGN_MAX_DIAGS:
            o["edit"], o["matches"], o["n_diags"], o["flags"] = 0xFFFFFFFF, 0, n_diags, 0
        else:
            V = banded_values(a, b, band)
            key = int(V[m + 1, n + 1])
            edit = (key + K - 1) // K
            o["edit"], o["matches"], o["n_diags"] = edit, edit * K - key, n_diags
            o["flags"] = A.ALN_DONE | (A.ALN_EXACT if edit - abs(n - m) <= 2 * band else 0)
            if trace_bytes(m, n, band) <= budget:
                o["flags"] |= A.ALN_PATH
                ops += runs_of(walk_back(V, a, b))
        off[c + 1] = len(ops)
    return aln, np.array(ops, np.uint32), off


def sums(ops):
    """{letter: bases} of a chain's runs"""
    out = dict.fromkeys("=XID", 0)
    for v in np.asarray(ops).tolist():
        out[LETTER[v & 15]] += v >> 4
    return out


def replay(ops, a, b):
    """walk the runs over the two segments: every = column is equal, every X column differs, and both segments are used up"""
    i = j = 0
    for v in np.asarray(ops).tolist():
        n, op = v >> 4, LETTER[v & 15]
        assert n > 0
        if op in "=X":
            assert ((a[i:i + n] == b[j:j + n]) == (op == "=")).all() and len(a[i:i + n]) == n == len(b[j:j + n])
        i, j = i + (n if op != "D" else 0), j + (n if op != "I" else 0)
    assert (i, j) == (len(a), len(b))


def check_self(chains, bases, off, band, res, bases_db=None, off_db=None):
    """the identities of include/kmu.h on a result (aln, ops, op_offsets)"""
    aln, ops, op_off = res
    plain = reference_align(chains, bases, off, bases_db, off_db, band)
    assert aln.dtype == ALN and ops.dtype == np.uint32 and op_off.dtype == np.uint64 and op_off[0] == 0 and op_off[-1] == ops.shape[0]
    masked = aln.copy()
    masked["flags"] &= ~np.uint32(A.ALN_PATH)
    assert masked.tobytes() == plain.tobytes()
    for c, rec in enumerate(chains):
        mine = ops[int(op_off[c]):int(op_off[c + 1])]
        if not aln[c]["flags"] & A.ALN_PATH:
            assert mine.size == 0
            continue
        assert aln[c]["flags"] & A.ALN_DONE
        a, b = segments(rec, bases, off, bases if bases_db is None else bases_db, off if off_db is None else off_db)
        s = sums(mine)
        assert s["="] == aln[c]["matches"] and s["X"] + s["I"] + s["D"] == aln[c]["edit"]
        assert s["="] + s["X"] + s["I"] == len(a) and s["="] + s["X"] + s["D"] == len(b)
        assert (np.diff(mine & 15) != 0).all() and mine.size <= 2 * int(aln[c]["edit"]) + 1
        replay(mine, a, b)


def one(a, b, band, strand=0):
    """the reference's result for the strings a (read 0) and b (read 1) taken whole, as (record, CIGAR string)"""
    bases, off = batch([a, b, "ACGT"])
    chains = chain_recs([(0, 1, strand, 0, len(a), 0, len(b))])
    res = reference_cigar(chains, bases, off, band=band)
    check_self(chains, bases, off, band, res)
    return res[0][0], minimizer.cigar_strings(res[1], res[2])[0]


def test_reference_against_itself():
    rng = np.random.default_rng(12)
    rows, reads = [], []
    for rep in range(120):
        alpha = "AC" if rep % 2 else "ACGT"
        m, n = int(rng.integers(0, 41)), int(rng.integers(0, 41))
        if rep % 10 == 0:
            m = 0
        if rep % 10 == 5:
            n = 0
        a = "".join(rng.choice(list(alpha), m))
        b = "".join(rng.choice(list(alpha), n))
        if rep % 3 == 0 and m and n:  # related strings
            b = a[:n // 2] + "".join(rng.choice(list(alpha), 2)) + a[n // 2 + 1:]
        s = rep & 1
        reads += [a, revcomp(b) if s else b]
        rows.append((2 * rep, 2 * rep + 1, s, 0, len(a), 0, len(b)))
    bases, off = batch(reads + ["ACGT"])
    chains = chain_recs(rows)
    for band in (0, 1, 2, 5, 8):
        res = reference_cigar(chains, bases, off, band=band)
        check_self(chains, bases, off, band, res)
        assert (res[0]["flags"] & A.ALN_PATH).all()


# ---- ties by hand -----------------------------------------------------------------------------------------------------------------
# (a, b, band, strand, CIGAR along A); tests/test_gpu_chain_cigar.py runs the same on the device
HAND_CIGARS = [
    ("AA", "A", 1, 0, "1I1="),                       # the hand example of include/kmu.h: the diagonal is tried first, from the end
    ("AA", "A", 7, 0, "1I1="),
    ("A", "AA", 1, 0, "1D1="),                       # its mirror
    ("AAAAA", "AAAAAAAA", 1, 0, "3D5="),             # every placement of the gap ties: it goes to the start
    ("AAAAAAAA", "AAAAA", 0, 0, "3I5="),
    ("ACACACAC", "CACACACA", 1, 0, "1D7=1I"),        # 1I7=1D ties; at (8, 8) no diagonal, and up -- v(7, 8) = (1, 7) -- is tried before left
    ("ACACACAC", "CACACACA", 0, 0, "8X"),
    ("ACGTACGGTT", "ACGTCAGGTT", 2, 0, "4=1D1=1I4="),  # AC / CA: 1I1=1D ties; at (6, 6) up -- v(5, 6) = (1, 5) -- is tried before left
    ("AAC", revcomp("AC"), 1, 1, "1I2="),            # strand 1: A against the reverse complement of B
    ("ACGTTGCAAC", "GTTGCAACGT".lower(), 3, 1, "10="),
    ("", "ACG", 0, 0, "3D"),
    ("ACG", "", 2, 0, "3I"),
    ("", "", 0, 0, ""),
]


@pytest.mark.parametrize("a,b,band,strand,cigar", HAND_CIGARS)
def test_ties_by_hand(a, b, band, strand, cigar):
    rec, got = one(a, b, band, strand)
    assert got == cigar and rec["flags"] & A.ALN_PATH


def test_long_runs_are_cut_and_wide_bands_have_no_path():
    assert runs_of("=" * 7 + "X" * 3, 3) == [1 << 4 | 7, 3 << 4 | 7, 3 << 4 | 7, 3 << 4 | 8]
    a, b = "A" * 3, "A" * (A.ALIGN_MAX_DIAGS + 3 - 2 * 4)
    rec, got = one(a, b, 4)
    assert rec.tolist() == (0xFFFFFFFF, 0, A.ALIGN_MAX_DIAGS + 1, 0) and got == ""
    # a chain whose own trace is above the budget keeps its record and loses its path
    bases, off = batch(["ACGTACGTAC", "ACGTTCGTAC"])
    chains = chain_recs([(0, 1, 0, 0, 10, 0, 10)])
    assert trace_bytes(10, 10, 2) == 2 * 256 and trace_bytes(0, 0, 0) == 256 and trace_bytes(7, 7, 200) == 4 * 256
    full, cut = reference_cigar(chains, bases, off, band=2, max_trace_bytes=512), reference_cigar(chains, bases, off, band=2, max_trace_bytes=511)
    assert full[0][0].tolist() == (1, 9, 5, 7) and cut[0][0].tolist() == (1, 9, 5, 3) and cut[1].size == 0 and cut[2].tolist() == [0, 0]


# ---- the symbol and its surroundings ------------------------------------------------------------------------------------------------
def test_symbol_and_bindings():
    """fails without the feature: the symbol is missing"""
    L = lib.load()
    assert "kmu_chain_cigar" in lib.SYMBOLS and hasattr(L, "kmu_chain_cigar")
    assert len(L.kmu_chain_cigar.argtypes) == 16
    assert callable(getattr(lib.Context, "chain_cigar"))
    assert callable(minimizer.cigar_chains) and callable(minimizer.read_cigars) and callable(minimizer.cigar_strings)


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()

    def define(name):
        return int(re.search(r"#define %s\s+(\d+)u" % name, txt).group(1))
    assert define("KMU_ALN_PATH") == A.ALN_PATH == 4
    assert (define("KMU_CIGAR_I"), define("KMU_CIGAR_D"), define("KMU_CIGAR_EQ"), define("KMU_CIGAR_X")) == \
        (A.CIGAR_I, A.CIGAR_D, A.CIGAR_EQ, A.CIGAR_X) == (1, 2, 7, 8)
    assert define("KMU_CIGAR_MAX_RUN") == A.CIGAR_MAX_RUN == 2 ** 28 - 1
    assert define("KMU_CIGAR_TRACE_DEFAULT") == A.CIGAR_TRACE_DEFAULT
    assert "int kmu_chain_cigar(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains," in txt
    par = re.search(r"typedef struct kmu_cigar_params \{(.*?)\} kmu_cigar_params;", txt, re.S).group(1)
    assert re.findall(r"uint(?:32|64)_t (\w+);", par) == [n for n, _ in A.CigarParams._fields_] == ["band", "flags", "max_trace_bytes"]
    assert C.sizeof(A.CigarParams) == 16 and A.CigarParams.max_trace_bytes.offset == 8
    # the kernel's constants are the header's
    core = open(os.path.join(ROOT, "kmerutils_amd", "csrc", "kmu_align_core.h")).read()
    ops = int(re.search(r"constexpr uint32_t ALIGN_DIR_OPS = 0x([0-9A-Fa-f]+)u;", core).group(1), 16)
    assert [(ops >> (4 * d)) & 15 for d in range(4)] == [A.CIGAR_EQ, A.CIGAR_X, A.CIGAR_I, A.CIGAR_D]


def test_refusals_that_need_no_device():
    L = lib.load()
    arr = np.zeros(64, np.uint8)
    p = A.CigarParams(4, 0, 0)
    a, total = arr.ctypes.data, C.c_uint64(99)
    # no context: refused before anything is touched, whatever else is there
    assert L.kmu_chain_cigar(None, a, 1, a, a, 1, a, a, 1, C.byref(p), A.MEM_HOST, a, a, a, 8, C.byref(total)) == A.E_BAD_ARG
    assert L.kmu_chain_cigar(None, None, 1, None, None, 1, None, None, 1, None, A.MEM_HOST, None, None, None, 0, None) == A.E_BAD_ARG
    assert L.kmu_chain_cigar(None, a, 0, a, a, 1, a, a, 1, C.byref(p), A.MEM_HOST, a, a, None, 0, C.byref(total)) == A.E_BAD_ARG
    assert not arr.any() and total.value == 99


# ---- cigar_chains and read_cigars on a stub context -------------------------------------------------------------------------------
class _StubContext:
    def chain_cigar(self, chains, bases_q, offsets_q, bases_db=None, offsets_db=None, band=64, max_trace_bytes=0, aln=None):
        self.seen = (chains, bases_q, offsets_q, bases_db, offsets_db, band, max_trace_bytes, aln)
        return "aln", "ops", "off"


def test_cigar_chains_and_read_cigars_pass_the_batches_on(monkeypatch):
    stub = _StubContext()
    assert minimizer.cigar_chains(stub, "chains", "bq", "oq") == ("aln", "ops", "off")
    assert stub.seen == ("chains", "bq", "oq", None, None, 64, 0, None)
    minimizer.cigar_chains(stub, "chains", "bq", "oq", "bdb", "odb", band=9, max_trace_bytes=77, aln="a")
    assert stub.seen == ("chains", "bq", "oq", "bdb", "odb", 9, 77, "a")
    seen = {}

    def read_chains(ctx, bases, offsets, k, w, *rest):
        seen["args"] = (ctx, bases, offsets, k, w) + rest
        return "chains"
    monkeypatch.setattr(minimizer, "read_chains", read_chains)
    assert minimizer.read_cigars(stub, "b", "o", 15, 10, band=32) == ("chains", "aln", "ops", "off")
    assert seen["args"] == (stub, "b", "o", 15, 10, A.FHASH_CANON_INVHASH, 0, 5000, 500, 3, 0)
    assert stub.seen == ("chains", "b", "o", None, None, 32, 0, None)


# ---- text -------------------------------------------------------------------------------------------------------------------------
def paf_case():
    chains = chain_recs([(0, 2, 0, 10, 110, 5, 100), (1, 0, 1, 0, 50, 20, 75), (2, 1, 0, 0, 40, 0, 1200), (1, 1, 0, 3, 3, 4, 4)])
    chains["score"], chains["n_seeds"] = [310, 45, 60, 1], [9, 3, 4, 1]
    aln = np.array([(7, 93, 134, 7), (2, 52, 134, 5), (0xFFFFFFFF, 0, 1289, 0), (0, 0, 129, 7)], ALN)
    ops = np.array([40 << 4 | 7, 5 << 4 | 1, 2 << 4 | 8, 53 << 4 | 7, 48 << 4 | 7, 2 << 4 | 2, 1 << 4 | 1, 1 << 4 | 8, 3 << 4 | 7], np.uint32)
    return chains, aln, ops, np.array([0, 4, 9, 9, 9], np.uint64), np.array([0, 500, 560, 2000], np.uint64), ["r0", "r1", "r2"]


def test_cigar_strings():
    chains, _, ops, op_off, _, _ = paf_case()
    assert minimizer.cigar_strings(ops, op_off) == ["40=5I2X53=", "48=2D1I1X3=", "", ""]
    assert minimizer.cigar_strings(ops, op_off, extended=False) == ["40M5I55M", "48M2D1I4M", "", ""]
    assert minimizer.cigar_strings(ops, op_off, chains) == ["40=5I2X53=", "3=1X1I2D48=", "", ""]  # strand 1: along the target
    assert minimizer.cigar_strings(ops, op_off, chains, extended=False) == ["40M5I55M", "4M1I2D48M", "", ""]
    assert minimizer.cigar_strings(ops.view(np.int32), op_off.view(np.int64)) == ["40=5I2X53=", "48=2D1I1X3=", "", ""]
    assert minimizer.cigar_strings(ops[:0], op_off[:1]) == []


def test_paf_lines_with_and_without_cigar():
    chains, aln, ops, op_off, off, names = paf_case()
    plain = minimizer.paf_lines(chains, aln, names, off)
    assert plain == [
        "r0\t500\t10\t110\t+\tr2\t1440\t5\t100\t93\t100\t255\tNM:i:7\ts1:i:310\tcm:i:9",
        "r1\t60\t0\t50\t-\tr0\t500\t20\t75\t52\t54\t255\tNM:i:2\ts1:i:45\tcm:i:3",
        "r2\t1440\t0\t40\t+\tr1\t60\t0\t1200\t0\t1200\t255\ts1:i:60\tcm:i:4",
        "r1\t60\t3\t3\t+\tr1\t60\t4\t4\t0\t0\t255\tNM:i:0\ts1:i:1\tcm:i:1",
    ]
    assert minimizer.paf_lines(chains, aln, names, off, cigar=None) == plain
    tagged = minimizer.paf_lines(chains, aln, names, off, cigar=(ops, op_off))
    assert tagged == [plain[0] + "\tcg:Z:40=5I2X53=", plain[1] + "\tcg:Z:3=1X1I2D48=", plain[2], plain[3] + "\tcg:Z:"]
    no_path = aln.copy()
    no_path["flags"] &= ~np.uint32(A.ALN_PATH)
    assert minimizer.paf_lines(chains, no_path, names, off, cigar=(ops, op_off)) == minimizer.paf_lines(chains, no_path, names, off)
    assert minimizer.paf_lines(chains[:0], aln[:0], names, off, cigar=(ops[:0], op_off[:1])) == []
