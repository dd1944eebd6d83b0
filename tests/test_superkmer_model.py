"""The tests' model of the super-k-mer record (superkmer_model.py) against the oracle's reader of records, and its count of the
fewest records a sender can emit on owner sequences written out by hand.  No GPU."""
import numpy as np
import pytest

import superkmer_model as M


@pytest.mark.parametrize("L", [1, 2, 15, 16])
@pytest.mark.parametrize("k", [17, 23, 24, 28, 29, 31])
def test_packed_record_expands_to_its_canonical_kmers(oracle, k, L):
    rng = np.random.default_rng(1000 * k + L)
    for trial in range(8):
        # the last trials end on T and on A: bits right up to the length field, and a tail that is all zeros
        bases = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L + k - 1)])
        if trial >= 6:
            bases = bases[:-3] + (b"TTT" if trial == 6 else b"AAA")
        rec = M.pack_record(bases, k)
        assert all(0 <= w < 1 << 32 for w in rec) and (rec[2] & 15) == L - 1
        got, clean = oracle.superkmer_expand(np.array([rec], np.uint32), k)
        assert clean and np.array_equal(got, M.canon_kmers(bases, k)), (k, L, bases)
    # both strands of a sequence hold the same canonical k-mers, in reverse order
    rc = bases[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    assert np.array_equal(M.canon_kmers(rc, k), M.canon_kmers(bases, k)[::-1])
    # lower case letters are the same bases
    assert M.pack_record(bases.lower(), k) == rec


def test_packed_record_layout_by_hand():
    # k = 17, one k-mer "C" + 16 x "A": C = 01 in bits 31..30 of word 0, nothing else, length field 0
    assert M.pack_record(b"C" + b"A" * 16, 17) == (0x40000000, 0, 0)
    # 46 bases of T at k = 31: 92 bits set, the length field holds 15
    assert M.pack_record(b"T" * 46, 31) == (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    # 17 bases at k = 17 end in bits 31..30 of word 1
    assert M.pack_record(b"A" * 16 + b"G", 17) == (0, 0x80000000, 0)


def test_ideal_records_on_hand_written_owner_sequences():
    # one read: a run of 33 for owner 2 (3 records), then a run of 16 for owner 0 (1) that ends with the read
    own = [2] * 33 + [0] * 16
    assert M.ideal_records(own, [49], 3).tolist() == [1, 0, 3]
    # two reads whose k-mers share an owner: the run ends at the read end, 17 + 1 k-mers are 2 + 1 records, not ceil(18 / 16) = 2;
    # a read without k-mers between them changes nothing
    assert M.ideal_records([1] * 18, [17, 0, 1], 2).tolist() == [0, 3]
    # alternating owners: one record per k-mer
    assert M.ideal_records([0, 1] * 20, [40], 2).tolist() == [20, 20]
    # no k-mers at all, with and without reads
    assert M.ideal_records([], [], 4).tolist() == [0, 0, 0, 0] and M.ideal_records([], [0, 0, 0], 1).tolist() == [0]
    # a run of exactly 16 and one of 17, owners that never occur
    assert M.ideal_records([5] * 16 + [4] * 17, [16, 17], 8).tolist() == [0, 0, 0, 0, 2, 1, 0, 0]
