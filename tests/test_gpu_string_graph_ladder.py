"""The string graph as one more stage of the long-read ladder (tests/read_families.py, unchanged): behind chain_align, on the
families whose overlaps mean something to a graph -- dovetail, identical, chimera_rc and unrelated -- the device against
reference_graph applied to the device's own chain and alignment records, byte for byte, on host arrays and on resident tensors."""
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import read_families as F  # noqa: E402
from test_gpu_string_graph import same, to_device, to_host  # noqa: E402
from test_string_graph_abi import params, reference_graph  # noqa: E402

pytestmark = pytest.mark.gpu
# the reads have a few hundred bases at 3 % edits: overlaps from 50 bases on, at least 80 % identity
GRAPH = params(min_overlap=50, min_identity_permille=800, fuzz=10)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def records_of(ctx, name):
    """the device's own chains and alignment records of a case: the first three stages of the ladder, then chain_align"""
    bases, offsets, p = F.case_batch(name)
    s = dict(own=True, bases=bases, offsets=offsets, bases_db=None, offsets_db=None)
    for st in F.STAGES[:3]:
        s.update(zip(st.outputs, st.dev(s, p, ctx)))
    chains = s["chains"]
    return chains, ctx.chain_align(chains, bases, offsets, band=p.band), offsets


@pytest.mark.parametrize("name", ["dovetail", "identical", "chimera_rc", "unrelated"])
def test_graph_stage(ctx, name):
    chains, aln, offsets = records_of(ctx, name)
    for with_aln in (aln, None):
        want = reference_graph(chains, with_aln, offsets, **GRAPH)
        same(ctx.sg_graph(chains, with_aln, offsets, **GRAPH), want, name + " host")
        same(to_host(*ctx.sg_graph(*to_device(chains, with_aln, offsets), **GRAPH)), want, name + " device")
    arcs, arc_off, classes, reads = want
    if name == "unrelated":
        assert len(chains) == 0 and len(arcs) == 0 and not reads.view(np.uint32).any() and not arc_off.any()
    if name == "identical":  # the chains take the reads whole: every pair ties, the read of the larger number is contained
        assert len(chains) == 15 and set(classes.tolist()) == {A.SG_B_CONTAINED} and reads["flags"].tolist() == [0, 1, 1, 1, 1, 1] and len(arcs) == 0
    if name == "dovetail":
        assert A.SG_DOVETAIL in classes.tolist()
