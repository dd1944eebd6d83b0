"""Unitig consensus on the device (minimizer.polish_unitigs, read_contigs) on the planted genomes of tests/test_unitig_map_abi.py:
error-free reads pin the coordinate arithmetic of every branch against the real alignment -- every record aligns with 0 edits and
nothing changes --, noisy reads must come out closer to the template than the draft, and the composition equals its stages called
by hand on the reference's map records, byte for byte, on host arrays and on resident tensors."""
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_string_graph_abi import CHAIN, params  # noqa: E402
from test_unitigs_abi import STEP, UNITIG  # noqa: E402
from test_unitig_map_abi import edit_distance, planted_genome, reference_unitig_chains  # noqa: E402
from test_gpu_unitig_map import dev, host  # noqa: E402

pytestmark = pytest.mark.gpu
NOISY_SEED = 11
ALN = np.dtype(A.CHAIN_ALN_DTYPE)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def layout(g):
    return g["unitigs"], g["path"], g["place"]


def draft(ctx, g):
    return ctx.sg_unitig_seqs(g["unitigs"], g["path"], g["bases"], g["offsets"])


def stages(ctx, records, seq, seq_off, bases, off, band=64, min_depth=2, max_ins=16):
    """the stages of polish_unitigs called one by one: (cons, cons_off, tables, aln)"""
    aln, ops, op_off = ctx.chain_cigar(records, seq, seq_off, bases, off, band=band)
    pile, _ = ctx.chain_pileup(records, aln, ops, op_off, seq, seq_off, bases, off, sides=A.PILE_Q)
    call, _ = ctx.pile_call(pile, seq, seq_off, min_depth=min_depth)
    ins_len, n_slots = ctx.pile_ins_plan(pile, call, max_ins=max_ins)
    ins, _ = ctx.chain_pile_ins(records, aln, ops, op_off, seq, seq_off, ins_len, n_slots, bases, off, sides=A.PILE_Q)
    cons, cons_off = ctx.pile_consensus(pile, call, ins_len, n_slots, ins, seq, seq_off)
    return cons, cons_off, (pile, call, ins_len, n_slots, ins), aln


def translated(ctx, tables, seq, seq_off, cons_off, unitig, coord):
    """coordinates of unitig `unitig` in the polished batch"""
    rows = np.asarray(seq_off).astype(np.int64)[unitig] + np.asarray(coord).astype(np.int64)
    pos = ctx.pile_consensus_pos(*tables, seq, seq_off, rows.astype(np.uint64))
    return pos.astype(np.int64) - np.asarray(cons_off).astype(np.int64)[unitig]


@pytest.fixture(scope="module")
def noisy():
    return planted_genome(NOISY_SEED, rate=0.05, ends=8)


@pytest.mark.parametrize("circular", [False, True])
def test_error_free_reads_change_nothing(ctx, circular):
    g = planted_genome(5, circular)
    seq, seq_off = draft(ctx, g)
    assert seq.tobytes() == g["template"].tobytes()
    cons, cons_off, new_path, summaries, records, aln = minimizer.polish_unitigs(ctx, *layout(g), seq, seq_off, g["bases"], g["offsets"],
                                                                                 g["chains"], g["classes"])
    want, stats = reference_unitig_chains(*layout(g), g["chains"], g["classes"], g["offsets"])
    assert records.tobytes() == want.tobytes() and stats["n_contained"] > 80 and len(summaries) == 1
    assert len(aln) == len(records) and not aln["edit"].any() and (aln["flags"] & A.ALN_PATH).all()
    assert (aln["matches"] == records["a_end"] - records["a_start"]).all()
    assert cons.tobytes() == seq.tobytes() and cons_off.tolist() == seq_off.tolist()
    assert new_path.dtype == STEP and new_path.tobytes() == g["path"].tobytes()
    if circular:  # the first reads of the circle are mapped by their tails only
        assert int(records["a_start"][0]) == 0 and int(records["a_end"][0]) == 150 and int(records["b_start"][0]) == 450


def test_noisy_reads_come_out_closer_to_the_template(ctx, noisy):
    """Measured on one MI355X with NOISY_SEED = 11: the draft is 159 edits from the 3 000 bases of the template, the polished unitig 1
    (DESIGN.md 3.25)."""
    g = noisy
    seq, seq_off = draft(ctx, g)
    got = minimizer.polish_unitigs(ctx, *layout(g), seq, seq_off, g["bases"], g["offsets"], g["chains"], g["classes"])
    d_draft, d_polished = edit_distance(seq, g["template"]), edit_distance(got[0], g["template"])
    print("edit distance to the template: draft %d, polished %d (template %d bases)" % (d_draft, d_polished, len(g["template"])))
    assert d_polished < d_draft
    # the same stages by hand on the reference's records
    want, _ = reference_unitig_chains(*layout(g), g["chains"], g["classes"], g["offsets"])
    cons, cons_off, tables, aln = stages(ctx, want, seq, seq_off, g["bases"], g["offsets"])
    assert got[0].tobytes() == cons.tobytes() and got[1].tobytes() == cons_off.tobytes()
    assert got[4].tobytes() == want.tobytes() and got[5].tobytes() == aln.tobytes()
    ends = translated(ctx, tables, seq, seq_off, cons_off, np.zeros(len(g["path"]), np.int64), g["path"]["end"])
    assert got[2]["end"].tolist() == ends.tolist() and got[2]["read"].tolist() == g["path"]["read"].tolist()
    assert int(ends[-1]) == len(cons) and (np.diff(ends) >= 0).all()


def test_resident_tensors_give_the_same_bytes(ctx, noisy):
    g = noisy
    seq, seq_off = draft(ctx, g)
    want = minimizer.polish_unitigs(ctx, *layout(g), seq, seq_off, g["bases"], g["offsets"], g["chains"], g["classes"], rounds=2)
    got = minimizer.polish_unitigs(ctx, dev(g["unitigs"], 8), dev(g["path"], 4), dev(g["place"], 4), dev(seq), dev(seq_off), dev(g["bases"]),
                                   dev(g["offsets"]), dev(g["chains"], 10), dev(g["classes"]), rounds=2)
    assert all(x.is_cuda for x in got)
    for x, w, dtype in zip(got, want, (np.uint8, np.uint64, STEP, np.dtype(A.READ_PILE_DTYPE), CHAIN, ALN)):
        assert host(x, dtype).tobytes() == w.tobytes(), dtype


def test_two_rounds_are_two_rounds_by_hand(ctx, noisy):
    g = noisy
    seq, seq_off = draft(ctx, g)
    records, _ = ctx.sg_unitig_chains(*layout(g), g["chains"], g["classes"], g["offsets"])
    cons1, off1, tables, _ = stages(ctx, records, seq, seq_off, g["bases"], g["offsets"])
    second = records.copy()
    for name in ("a_start", "a_end"):
        second[name] = translated(ctx, tables, seq, seq_off, off1, records["read_a"].astype(np.int64), records[name])
    ends1 = translated(ctx, tables, seq, seq_off, off1, np.zeros(len(g["path"]), np.int64), g["path"]["end"])
    cons2, off2, tables2, aln2 = stages(ctx, second, cons1, off1, g["bases"], g["offsets"])
    ends2 = translated(ctx, tables2, cons1, off1, off2, np.zeros(len(ends1), np.int64), ends1)
    got = minimizer.polish_unitigs(ctx, *layout(g), seq, seq_off, g["bases"], g["offsets"], g["chains"], g["classes"], rounds=2)
    assert got[0].tobytes() == cons2.tobytes() and got[1].tobytes() == off2.tobytes() and got[2]["end"].tolist() == ends2.tolist()
    assert got[4].tobytes() == second.tobytes() and got[5].tobytes() == aln2.tobytes()


def test_gfa_lines_of_the_polished_unitigs(ctx, noisy):
    g = noisy
    seq, seq_off = draft(ctx, g)
    cons, cons_off, new_path, _, _, _ = minimizer.polish_unitigs(ctx, *layout(g), seq, seq_off, g["bases"], g["offsets"], g["chains"], g["classes"])
    unitigs = minimizer.polished_unitigs(g["unitigs"], cons_off)
    assert unitigs.dtype == UNITIG and int(unitigs["len"][0]) == len(cons) and g["unitigs"]["len"][0] == len(seq)
    names = ["r%d" % r for r in range(len(g["offsets"]) - 1)]
    lines = minimizer.unitig_gfa_lines(unitigs, new_path, cons, cons_off, names)
    assert len(lines) == 1 + g["n_layout"] and lines[0] == "S\tutg000000l\t%s\tLN:i:%d" % (cons.tobytes().decode(), len(cons))
    cols = lines[-1].split("\t")
    assert cols[0] == "a" and int(cols[2]) + int(cols[5]) == len(cons) and all(int(x.split("\t")[5]) >= 0 for x in lines[1:])


def test_read_contigs_on_error_free_reads(ctx):
    """from the reads alone: the graph, the layout and the draft are those of read_unitigs, and polishing changes no byte"""
    g = planted_genome(5, cont_step=96)
    kw = dict(params(min_overlap=100, fuzz=10))
    unitigs, path, place, seq, seq_off = minimizer.read_unitigs(ctx, g["bases"], g["offsets"], 15, 5, **kw)
    assert len(unitigs) == 1 and seq.tobytes() == g["template"].tobytes() and int((place["unitig"] == A.SG_NONE).sum()) > 20
    got = minimizer.read_contigs(ctx, g["bases"], g["offsets"], 15, 5, **kw)
    for x, w in zip(got[:5], (unitigs, path, place, seq, seq_off)):
        assert x.dtype == w.dtype and x.tobytes() == w.tobytes()
    assert len(got[5]) == 1
