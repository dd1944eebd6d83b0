"""Test helper: small hostile read batches and the long-read route as a ladder of stages.

`FAMILIES` are deterministic generators of read batches that the friendly end-to-end tests never see: tandem repeats and
homopolymers (one hash many times, `max_occ`, ties in the chaining, chains that leave the band), identical reads, a palindrome,
dovetails and contained reads, unrelated reads, empty and very short reads, lower case, a chimera joined on opposite strands.
`CASES` gives every family the parameter sets it is run with.

A ladder is the route reads -> minimizers -> seed pairs -> chains -> runs -> pileup -> calls -> slots -> inserted letters ->
consensus -> segments -> consensus positions -> trimmed reads, one `Stage` per step.  A stage has two faces that take the same
state (a dict of everything made so far) and return the same named arrays: `ref`, which calls the plain-Python reference of that
step (imported from the tests that own them, never rewritten here), and `dev`, which calls the Context / minimizer entry point.
`reference_ladder` runs the `ref` faces in a row and needs no device; `device_ladder` runs the `dev` faces; `check_ladder` walks
a device ladder and compares every stage, byte for byte, with that stage's reference applied to the DEVICE's own output of the
stages before -- so a failure names the first stage that is wrong and not one that inherited a difference.  Both ladders take one
batch (the self-join) or two (q against db, the reads numbered per batch); every per-read result is then a pair (q side, db side).
"""
import collections
import os
import sys

import numpy as np

from kmerutils_amd import _abi as A
from kmerutils_amd import minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import batch, revcomp  # noqa: E402
from test_chain_cigar_abi import reference_cigar  # noqa: E402
from test_chains_abi import reference_chains  # noqa: E402
from test_consensus_abi import reference_consensus, reference_ins_plan, reference_ins_votes  # noqa: E402
from test_pileup_abi import reference_call, reference_pileup  # noqa: E402
from test_trim_abi import reference_cons_pos, reference_extract, reference_segments  # noqa: E402

K, W = 15, 10
FHASH = A.FHASH_CANON_INVHASH
KMER_TYPE = A.kmer_type_for_k(K)
UINT64_MAX = 2 ** 64 - 1
FLAGS = (("DONE", A.ALN_DONE), ("EXACT", A.ALN_EXACT), ("PATH", A.ALN_PATH))
ALL_FLAGS = A.ALN_DONE | A.ALN_EXACT | A.ALN_PATH


# ---- the families -----------------------------------------------------------------------------------------------------------------
def rand_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), int(n)))


def mutate(rng, s, rate):
    """s with substitutions, insertions and deletions, a third of `rate` each"""
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(str(rng.choice([x for x in "ACGT" if x != c])))
        elif r < 2 * rate / 3:
            out += [str(rng.choice(list("ACGT"))), c]
        elif r >= rate:
            out.append(c)
    return "".join(out)


def friendly():
    """8 copies of a 400-base template at 4 % edits, every second one reverse-complemented: the control"""
    rng = np.random.default_rng(101)
    root = rand_seq(rng, 400)
    reads = [mutate(rng, root, 0.04) for _ in range(8)]
    return [revcomp(s) if r & 1 else s for r, s in enumerate(reads)]


EDGE_LENGTHS = (1, K - 1, K, K + W - 2, K + W - 1, K + W)
# where the friendly reads sit in `edges` (the other reads are the short ones and the empty ones)
EDGES_LONG = (2, 4, 6, 10, 12, 14, 16, 18)


def edges():
    """the friendly reads between reads of 0, 1, k - 1, k, k + w - 2, k + w - 1 and k + w random bases: two empty reads first, two
    last, three in a row in the middle"""
    rng = np.random.default_rng(102)
    f = friendly()
    s = [rand_seq(rng, n) for n in EDGE_LENGTHS]
    reads = ["", "", f[0], s[0], f[1], s[1], f[2], "", "", "", f[3], s[2], f[4], s[3], f[5], s[4], f[6], s[5], f[7], "", ""]
    assert [reads[i] for i in EDGES_LONG] == f
    return reads


def _repeat_family(seed, middles, flank):
    """flank_a + middle + flank_b per middle, the flanks of every read noisy copies (2 %) of the same two sequences"""
    rng = np.random.default_rng(seed)
    fa, fb = rand_seq(rng, flank), rand_seq(rng, flank)
    return [mutate(rng, fa, 0.02) + mid + mutate(rng, fb, 0.02) for mid in middles]


TANDEM_UNIT = "ACGGTCA"
TANDEM_COPIES = (20, 184, 24, 28, 180)


def tandem():
    """flank_a + unit * c + flank_b with a 7-base unit: copy numbers 20, 24, 28 (close) and 180, 184 (far).  Every k-mer inside the
    repeat recurs every 7 bases, so one hash fills the repeat of every read"""
    return _repeat_family(103, [TANDEM_UNIT * c for c in TANDEM_COPIES], 200)


def homopolymer():
    """the same shape with 40 .. 65 A in the middle: poly-A gives a minimizer at every window start, all of one hash"""
    return _repeat_family(104, ["A" * c for c in (40, 65, 48, 57, 52, 61)], 120)


def identical():
    """the same 300 bases five times and their exact reverse complement.  (The seed is one whose sequence has a minimizer at its
    first and at its last k-mer, so that the chains take the reads whole; tests/test_read_ladder_ref.py asserts it.)"""
    s = rand_seq(np.random.default_rng(1074), 300)
    return [s] * 5 + [revcomp(s)]


def palindrome():
    """x + revcomp(x) twice, and a copy at 3 % edits: every seed hits on both strands"""
    rng = np.random.default_rng(106)
    x = rand_seq(rng, 150)
    p = x + revcomp(x)
    return [p, p, mutate(rng, p, 0.03)]


def unrelated():
    """6 random reads of 200 bases: no hit, no chain, no run"""
    rng = np.random.default_rng(107)
    return [rand_seq(rng, 200) for _ in range(6)]


def dovetail():
    """300-base windows of a 900-base sequence every 100 bases at 3 % edits, the fourth reverse-complemented, and one 100-base read
    contained in three of them"""
    rng = np.random.default_rng(108)
    g = rand_seq(rng, 900)
    reads = [mutate(rng, g[b:b + 300], 0.03) for b in range(0, 601, 100)]
    reads[3] = revcomp(reads[3])
    return reads + [mutate(rng, g[400:500], 0.03)]


def two_batches():
    """(q, db) for the route over two batches: q is `dovetail`; db holds four friendly reads and, between them, three fresh windows of
    the dovetail sequence (one reverse-complemented), so read i of q and read i of db are different reads"""
    rng = np.random.default_rng(108)
    g = rand_seq(rng, 900)
    rng = np.random.default_rng(111)
    windows = [mutate(rng, g[50:350], 0.03), revcomp(mutate(rng, g[250:550], 0.03)), mutate(rng, g[450:750], 0.03)]
    f = friendly()
    return dovetail(), [f[0], windows[0], f[1], windows[1], f[2], windows[2], f[3]]


def lower():
    """friendly with every second read all lower case and the others in mixed case"""
    rng = np.random.default_rng(109)
    out = []
    for r, s in enumerate(friendly()):
        out.append(s.lower() if r & 1 else "".join(c.lower() if rng.random() < 0.5 else c for c in s))
    return out


CHIMERA = 10  # the read of chimera_rc that is the chimera


def chimera_rc():
    """five copies of template A, five of template B (400 bases, 3 % edits) and the chimera mutate(A[:200]) + revcomp(mutate(B[200:])):
    its parts join on opposite strands.  Returns the reads; `chimera_join()` is the row of the join.  (Chains end where seeds end:
    the seed is one at which the last k-mer before the join and the first one behind it are minimizers of the chimera and of at
    least three copies of their parent, so that three chains end flush on either side of the join.)"""
    return _chimera()[0]


def chimera_join():
    return _chimera()[1]


def _chimera():
    rng = np.random.default_rng(12120)
    a, b = rand_seq(rng, 400), rand_seq(rng, 400)
    reads = [mutate(rng, a, 0.03) for _ in range(5)] + [mutate(rng, b, 0.03) for _ in range(5)]
    left = mutate(rng, a[:200], 0.03)
    reads.append(left + revcomp(mutate(rng, b[200:], 0.03)))
    assert len(reads) == CHIMERA + 1
    return reads, len(left)


FAMILIES = collections.OrderedDict((f.__name__, f) for f in (friendly, edges, tandem, homopolymer, identical, palindrome, unrelated, dovetail,
                                                             lower, chimera_rc))

# the parameters of a ladder; the defaults are those of minimizer.correct_trim_reads, but for min_depth = 2 and min_len = 30 (the
# families are small: 3 to 8 related reads of a few hundred bases)
Params = collections.namedtuple("Params", "k w max_occ max_gap band_chain min_seeds min_score band max_trace_bytes min_depth max_ins min_span "
                                          "min_len longest")
DEFAULT = Params(K, W, 0, 5000, 500, 3, 0, 64, 0, 2, 16, None, 30, False)

# case name -> (family, parameters).  tandem_flags: the repeat's hash is masked (every read carries it more than 8 times), so the
# flanks chain across the repeat where band_chain lets them -- a close and a far read then differ by more than a thousand bases,
# which at band 4 is more diagonals than a chain may have (no DONE); at band 4 the noisy flanks of two close reads need more than
# 8 edits beyond their length difference (no EXACT) unless the two reads are nearly clean; 24 KiB of trace hold a chain of two
# close reads and not the chain of the two far ones (no PATH).
CASES = collections.OrderedDict([
    ("friendly", ("friendly", DEFAULT)),
    ("edges", ("edges", DEFAULT)),
    ("tandem", ("tandem", DEFAULT._replace(band=4))),
    ("tandem_occ8", ("tandem", DEFAULT._replace(max_occ=8))),
    ("tandem_flags", ("tandem", DEFAULT._replace(max_occ=8, band_chain=2000, band=4, max_trace_bytes=24576))),
    ("homopolymer", ("homopolymer", DEFAULT._replace(band=4))),
    ("identical", ("identical", DEFAULT)),
    ("palindrome", ("palindrome", DEFAULT)),
    ("unrelated", ("unrelated", DEFAULT)),
    ("dovetail", ("dovetail", DEFAULT)),
    ("lower", ("lower", DEFAULT)),
    ("chimera_rc", ("chimera_rc", DEFAULT._replace(min_depth=3, min_len=50))),
    ("chimera_rc_depth_only", ("chimera_rc", DEFAULT._replace(min_depth=3, min_span=0, min_len=50))),
])


def case_batch(name):
    """(bases, offsets, params) of a case"""
    family, params = CASES[name]
    return batch(FAMILIES[family]()) + (params,)


# ---- the stages -------------------------------------------------------------------------------------------------------------------
def reference_pairs(q, db, own, max_occ):
    """the seed join as minimizer.seed_pairs documents it: uint32 [n, 2] pairs (entry of q, entry of db) of equal hashes, ordered by
    the entry of q, then the entry of db.  A hash equal to UINT64_MAX seeds nothing; with max_occ > 0 neither does a hash that more
    than max_occ entries of db carry; in the self-join (own) a minimizer never pairs with one of its own read"""
    by_hash = {}
    for e, h in enumerate(np.asarray(db.hashes).tolist()):
        by_hash.setdefault(h, []).append(e)
    read_q, read_db = np.asarray(q.read).tolist(), np.asarray(db.read).tolist()
    out = []
    for e, h in enumerate(np.asarray(q.hashes).tolist()):
        bucket = by_hash.get(h, ())
        if h == UINT64_MAX or (max_occ and len(bucket) > max_occ):
            continue
        out += [(e, e2) for e2 in bucket if not own or read_db[e2] != read_q[e]]
    return np.array(out, np.uint32).reshape(-1, 2)


def _sides(s):
    """[(bases, offsets)] of the batches of a state: one in the self-join, q and db otherwise"""
    return [(s["bases"], s["offsets"])] + ([] if s["own"] else [(s["bases_db"], s["offsets_db"])])


def _db(s):
    return (None, None) if s["own"] else (s["bases_db"], s["offsets_db"])


def _per_side(s, f):
    """f(side index, bases, offsets) for every batch, the results transposed: a tuple per result name, an entry per side"""
    return tuple(zip(*[f(i, b, o) for i, (b, o) in enumerate(_sides(s))]))


def _rows(segs, offsets):
    """the first rows and the end rows of segments in their batch, as one uint64 array (all firsts, then all ends)"""
    beg = np.asarray(offsets).astype(np.uint64)[segs["read"]]
    return np.concatenate([beg + segs["start"].astype(np.uint64), beg + segs["end"].astype(np.uint64)])


def _mini(x):
    """a Minimizers record of host arrays from the five arrays of read_minimizers / `expected`"""
    return minimizer.Minimizers(*[np.asarray(v) for v in x[:5]], K, W, FHASH)


class Stage:
    """name: what a failure is reported under; outputs: the names it adds to the state; ref(s, p, oracle) and dev(s, p, ctx) return
    them as a tuple"""
    def __init__(self, name, outputs, ref, dev):
        self.name, self.outputs, self.ref, self.dev = name, outputs.split(), ref, dev


def _ref_minimizers(s, p, oracle):
    from test_gpu_minimizers import expected
    # the oracle hashes a batch of at least one byte
    return (tuple(_mini(expected(oracle, b if b.size else np.zeros(1, np.uint8), o, KMER_TYPE, p.k, FHASH, p.w)) for b, o in _sides(s)),)


def _dev_minimizers(s, p, ctx):
    return (tuple(minimizer.read_minimizers(ctx, b, o, p.k, p.w) for b, o in _sides(s)),)


def _ref_pairs(s, p, oracle):
    return (reference_pairs(s["mini"][0], s["mini"][-1], s["own"], p.max_occ),)


def _dev_pairs(s, p, ctx):
    return (minimizer.seed_pairs(ctx, s["mini"][0], None if s["own"] else s["mini"][1], p.max_occ),)


def _ref_chains(s, p, oracle):
    return (reference_chains(s["pairs"], s["mini"][0], None if s["own"] else s["mini"][1], p.k, p.max_gap, p.band_chain, p.min_seeds, p.min_score,
                             upper=s["own"]),)


def _dev_chains(s, p, ctx):
    return (ctx.seed_chains(s["pairs"], s["mini"][0], None if s["own"] else s["mini"][1], span=p.k, max_gap=p.max_gap, band=p.band_chain,
                            min_seeds=p.min_seeds, min_score=p.min_score, upper=s["own"]),)


def _ref_cigar(s, p, oracle):
    return reference_cigar(s["chains"], s["bases"], s["offsets"], *_db(s), band=p.band, max_trace_bytes=p.max_trace_bytes)


def _dev_cigar(s, p, ctx):
    return ctx.chain_cigar(s["chains"], s["bases"], s["offsets"], *_db(s), band=p.band, max_trace_bytes=p.max_trace_bytes)


def _ref_pileup(s, p, oracle):
    pile = reference_pileup(s["chains"], s["aln"], s["ops"], s["op_off"], s["bases"], s["offsets"], *_db(s))
    return (pile[:1] if s["own"] else pile,)


def _dev_pileup(s, p, ctx):
    pile = ctx.chain_pileup(s["chains"], s["aln"], s["ops"], s["op_off"], s["bases"], s["offsets"], *_db(s))
    return (pile[:1] if s["own"] else pile,)


def _ref_call(s, p, oracle):
    return _per_side(s, lambda i, b, o: reference_call(s["pile"][i], b, o, p.min_depth))


def _dev_call(s, p, ctx):
    return _per_side(s, lambda i, b, o: ctx.pile_call(s["pile"][i], b, o, min_depth=p.min_depth))


def _ref_plan(s, p, oracle):
    return _per_side(s, lambda i, b, o: reference_ins_plan(s["pile"][i], s["call"][i], p.max_ins))


def _dev_plan(s, p, ctx):
    return _per_side(s, lambda i, b, o: ctx.pile_ins_plan(s["pile"][i], s["call"][i], max_ins=p.max_ins))


def _ref_ins(s, p, oracle):
    ins_db = () if s["own"] else (s["ins_len"][1],)
    ins = reference_ins_votes(s["chains"], s["aln"], s["ops"], s["op_off"], s["bases"], s["offsets"], s["ins_len"][0], *_db(s), *ins_db)
    return (ins[:1] if s["own"] else ins,)


def _dev_ins(s, p, ctx):
    plan_db = () if s["own"] else (s["ins_len"][1], s["n_slots"][1])
    ins = ctx.chain_pile_ins(s["chains"], s["aln"], s["ops"], s["op_off"], s["bases"], s["offsets"], s["ins_len"][0], s["n_slots"][0], *_db(s), *plan_db)
    return (ins[:1] if s["own"] else ins,)


def _ref_consensus(s, p, oracle):
    return _per_side(s, lambda i, b, o: reference_consensus(s["pile"][i], s["call"][i], s["ins_len"][i], s["ins"][i], b, o))


def _dev_consensus(s, p, ctx):
    return _per_side(s, lambda i, b, o: ctx.pile_consensus(s["pile"][i], s["call"][i], s["ins_len"][i], s["n_slots"][i], s["ins"][i], b, o))


def _ref_segments(s, p, oracle):
    span = p.min_depth if p.min_span is None else p.min_span
    return _per_side(s, lambda i, b, o: reference_segments(s["pile"][i], o, p.min_depth, span, p.min_len, p.longest))


def _dev_segments(s, p, ctx):
    return _per_side(s, lambda i, b, o: ctx.pile_segments(s["pile"][i], o, min_depth=p.min_depth, min_span=p.min_span, min_len=p.min_len,
                                                           longest=p.longest))


def _ref_pos(s, p, oracle):
    return _per_side(s, lambda i, b, o: (reference_cons_pos(s["pile"][i], s["call"][i], s["ins_len"][i], s["ins"][i], b, o, _rows(s["segs"][i], o)),))


def _dev_pos(s, p, ctx):
    return _per_side(s, lambda i, b, o: (ctx.pile_consensus_pos(s["pile"][i], s["call"][i], s["ins_len"][i], s["n_slots"][i], s["ins"][i], b, o,
                                                                _rows(s["segs"][i], o)),))


def _ranges(s, i):
    n = len(s["segs"][i])
    return s["cons"][i], s["pos"][i][:n], s["pos"][i][n:]


def _ref_extract(s, p, oracle):
    return _per_side(s, lambda i, b, o: reference_extract(*_ranges(s, i)))


def _dev_extract(s, p, ctx):
    return _per_side(s, lambda i, b, o: ctx.extract_ranges(*_ranges(s, i)))


STAGES = (
    Stage("read_minimizers", "mini", _ref_minimizers, _dev_minimizers),
    Stage("seed_pairs", "pairs", _ref_pairs, _dev_pairs),
    Stage("seed_chains", "chains", _ref_chains, _dev_chains),
    Stage("chain_cigar", "aln ops op_off", _ref_cigar, _dev_cigar),
    Stage("chain_pileup", "pile", _ref_pileup, _dev_pileup),
    Stage("pile_call", "call reads", _ref_call, _dev_call),
    Stage("pile_ins_plan", "ins_len n_slots", _ref_plan, _dev_plan),
    Stage("chain_pile_ins", "ins", _ref_ins, _dev_ins),
    Stage("pile_consensus", "cons cons_off", _ref_consensus, _dev_consensus),
    Stage("pile_segments", "segs seg_off trims", _ref_segments, _dev_segments),
    Stage("pile_consensus_pos", "pos", _ref_pos, _dev_pos),
    Stage("extract_ranges", "out out_off", _ref_extract, _dev_extract),
)

# what both ladders return: the inputs, then every stage's outputs in order.  mini .. op_off belong to the chains; pile .. out_off
# are tuples with one entry per batch (one in the self-join; q, db otherwise)
Ladder = collections.namedtuple("Ladder", "own bases offsets bases_db offsets_db " + " ".join(" ".join(st.outputs) for st in STAGES))


def _start(bases, offsets, bases_db, offsets_db):
    return dict(own=bases_db is None, bases=bases, offsets=offsets, bases_db=bases_db, offsets_db=offsets_db)


def reference_ladder(oracle, bases, offsets, params=DEFAULT, bases_db=None, offsets_db=None):
    """every intermediate result of the route, from the references alone (oracle: the `oracle` fixture, for the k-mer hashes)"""
    s = _start(bases, offsets, bases_db, offsets_db)
    for st in STAGES:
        s.update(zip(st.outputs, st.ref(s, params, oracle)))
    return Ladder(**s)


def device_ladder(ctx, bases, offsets, params=DEFAULT, bases_db=None, offsets_db=None):
    """the same results through the Context / minimizer calls, on host arrays"""
    s = _start(bases, offsets, bases_db, offsets_db)
    for st in STAGES:
        s.update(zip(st.outputs, st.dev(s, params, ctx)))
    return Ladder(**s)


def reference_stage(lad, name, params, oracle=None):
    """{output: value} of one stage's reference on the earlier results of `lad`"""
    st = STAGES[[x.name for x in STAGES].index(name)]
    return dict(zip(st.outputs, st.ref(lad._asdict(), params, oracle)))


def reference_tail(lad, params, first="pile_segments", oracle=None):
    """a ladder whose stages from `first` on are the references' under other parameters, on the earlier results of `lad`"""
    s = lad._asdict()
    names = [st.name for st in STAGES]
    for st in STAGES[names.index(first):]:
        s.update(zip(st.outputs, st.ref(s, params, oracle)))
    return Ladder(**s)


# ---- comparing ----------------------------------------------------------------------------------------------------------------------
def flat(x):
    """the leaves of a stage output: a Minimizers record is its five arrays, a tuple per side its entries, an int itself"""
    if isinstance(x, minimizer.Minimizers):
        return [x.hashes, x.pos, x.read, x.strand, x.offsets]
    if isinstance(x, tuple):
        return [leaf for v in x for leaf in flat(v)]
    return [x]


def first_difference(got, want):
    """None if two stage outputs hold the same bytes, otherwise a text that names the first record that differs"""
    g, w = flat(got), flat(want)
    if len(g) != len(w):
        return "%d arrays, want %d" % (len(g), len(w))
    for k, (a, b) in enumerate(zip(g, w)):
        if isinstance(b, (int, np.integer)):
            if int(a) != int(b):
                return "value %d: got %d, want %d" % (k, a, b)
            continue
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype != b.dtype or a.shape != b.shape:
            return "array %d: got %s %s, want %s %s" % (k, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            rec = a.reshape(a.shape[0], -1) if a.dtype.names is None else a
            ref = b.reshape(b.shape[0], -1) if b.dtype.names is None else b
            bad = [i for i in range(a.shape[0]) if rec[i].tobytes() != ref[i].tobytes()]
            return "array %d, record %d of %d that differ (of %d): got %s, want %s" % (k, bad[0], len(bad), a.shape[0], rec[bad[0]], ref[bad[0]])
    return None


def check_ladder(got, oracle, params, what):
    """every stage of a device ladder against its reference on the device's own output of the stages before; stops at the first
    stage that differs and names it, the case and the record"""
    s = got._asdict()
    for st in STAGES:
        want = st.ref(s, params, oracle)
        for name, w in zip(st.outputs, want):
            diff = first_difference(s[name], w)
            assert diff is None, "%s: stage %s, output %s: %s" % (what, st.name, name, diff)


def swapped_chains(chains):
    """chain records with the sides exchanged, in the order of the exchanged read pair: what a call with q and db swapped reports
    where the two calls choose the same chains"""
    out = chains.copy()
    for a, b in (("read_a", "read_b"), ("a_start", "b_start"), ("a_end", "b_end")):
        out[a], out[b] = chains[b], chains[a]
    return out[np.lexsort((out["read_b"], out["read_a"]))]


def check_swapped(lad, swapped):
    """two ladders over two batches, the second with q and db exchanged.  What include/kmu.h makes symmetric is asserted: the same
    chains with the sides exchanged (on these batches no tie of the winner rule is broken by the (x, y) order), the same alignment
    records (edit and matches are unique values), and per row the same depth and the same ENDS.  The letter columns are NOT
    symmetric: the path prefers `I` to `D` among equal values, so where a gap can sit in two places the two calls place it
    differently and a partner's letter lands one row apart."""
    order = np.lexsort((swapped.chains["read_a"], swapped.chains["read_b"]))
    assert swapped_chains(swapped.chains).tobytes() == lad.chains.tobytes(), "chains"
    assert swapped.aln[order].tobytes() == lad.aln.tobytes(), "aln"
    for i in range(2):
        mine, theirs = lad.pile[i].astype(np.int64), swapped.pile[1 - i].astype(np.int64)
        assert (mine[:, :A.PILE_INS].sum(axis=1) == theirs[:, :A.PILE_INS].sum(axis=1)).all(), "depth of side %d" % i
        assert (mine[:, A.PILE_ENDS] == theirs[:, A.PILE_ENDS]).all(), "ENDS of side %d" % i


def flag_counts(aln):
    """{"chains": n, "no DONE": .., "no EXACT": .., "no PATH": .., "all": ..} of alignment records"""
    flags = np.asarray(aln["flags"]).astype(np.int64)
    out = {"chains": int(flags.size), "all": int(((flags & ALL_FLAGS) == ALL_FLAGS).sum())}
    for name, bit in FLAGS:
        out["no " + name] = int(((flags & bit) == 0).sum())
    return out


def has_every_flag_state(aln):
    """a chain without DONE, one that is DONE without EXACT, one that is DONE without PATH and one with all three"""
    flags = np.asarray(aln["flags"]).astype(np.int64)
    done = (flags & A.ALN_DONE) != 0
    return bool((~done).any() and (done & ((flags & A.ALN_EXACT) == 0)).any() and (done & ((flags & A.ALN_PATH) == 0)).any()
                and ((flags & ALL_FLAGS) == ALL_FLAGS).any())
