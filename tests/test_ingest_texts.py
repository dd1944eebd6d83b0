"""The texts of tests/ingest_texts.py under the two CPU references, the oracle's ingest and the plain readers: they agree on every text,
and every text has the properties that make the GPU tests of tests/test_gpu_ingest_edges.py mean something.  A text that fails here is
a bug of its builder, not a finding about the library.  No GPU."""
import numpy as np
import pytest

import ingest_texts as T
import read_stats_model as M


def both_references(oracle, text, fmt):
    """the oracle's (bases, offsets, info, record_index) of a text, after the plain reader gave the same"""
    wb, wo, winfo, widx = getattr(oracle, "ingest_" + fmt)(text)
    pb, po, pinfo, pidx = T.plain_ingest(text, fmt)
    assert pinfo == winfo
    assert np.array_equal(pb, wb) and np.array_equal(po, wo) and np.array_equal(pidx, widx)
    xb, xo, xinfo, xidx = oracle.ingest_fastx(text)  # the format by the first byte
    assert xinfo == winfo and np.array_equal(xb, wb) and np.array_equal(xo, wo) and np.array_equal(xidx, widx)
    if fmt == "fastq":
        model = M.ingest_fastq_qual(text)
        assert model is not None and np.array_equal(model[0], wb) and np.array_equal(model[2], wo) and np.array_equal(model[3], widx)
        assert model[1].size == wb.size
    return wb, wo, winfo, widx


@pytest.mark.parametrize("line", T.FASTQ_LINES)
def test_placed_fastq(oracle, line):
    texts = T.placed_texts("fastq", line)
    assert len(texts) == 17 * 2 * 2
    for P, nl, fin, text in texts:
        assert text[P] == 0x0A and text.endswith(b"\n") == fin and (nl == b"\r\n") == (text[P - 1] == 0x0D)
        _, _, info, idx = both_references(oracle, text, "fastq")
        assert (info["n_records"], info["n_kept"]) == (6, 4) and idx.tolist() == [0, 2, 3, 5], (P, nl, fin)


@pytest.mark.parametrize("what", T.FASTA_LINES)
def test_placed_fasta(oracle, what):
    texts = T.placed_texts("fasta", what)
    assert len(texts) == 17 * 2 * 2
    for P, nl, fin, text in texts:
        assert text[P] == 0x0A and text.endswith(b"\n") == fin and (nl == b"\r\n") == (text[P - 1] == 0x0D)
        _, off, info, idx = both_references(oracle, text, "fasta")
        assert (info["n_records"], info["n_kept"]) == (6, 4) and idx.tolist() == [0, 2, 3, 5], (P, nl, fin)
        assert np.diff(off.astype(np.int64)).tolist() == [12, 26, 0, 49]  # record 3 is a header alone
        assert b"\n>r3 a header alone" + nl + b">r4" in text  # two header lines next to each other


def test_the_positions_are_the_chunk_step_and_region_edges():
    assert all(P % 16 in (15, 0) for P in T.POSITIONS if P != 16385)
    for border in (144, 1024, T.REGION):  # the last and first byte of a step and of a region, and one chunk past each
        assert {border - 1, border, border + 15, border + 16} <= set(T.POSITIONS)
    assert {2 * T.REGION - 1, 2 * T.REGION, 3 * T.REGION - 1, 3 * T.REGION} <= set(T.POSITIONS)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_end_at(oracle, fmt):
    for n_bytes in T.END_SIZES:
        for nl in T.LINE_ENDS:
            for fin in (True, False):
                text = T.end_at(n_bytes, fmt, fin, nl)
                assert len(text) == n_bytes and text.endswith(b"\n") == fin
                _, _, info, _ = both_references(oracle, text, fmt)
                assert (info["n_records"], info["n_kept"]) == (5, 4)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_many_records(oracle, fmt):
    for n in T.RECORD_COUNTS:
        text = T.many_records(n, fmt)
        _, _, info, _ = both_references(oracle, text, fmt)
        if fmt == "fastq":
            assert info["n_records"] == n
        else:
            assert text.count(b"\n") == n and text.endswith(b"\n")  # n lines
        if n >= 1023:
            assert 0.05 * info["n_records"] <= info["nb_bad_reads"] <= 0.30 * info["n_records"], (n, info)
            assert info["n_records"] > n // 5


def test_special_texts(oracle):
    texts = T.special_texts()
    got = {name: both_references(oracle, text, fmt) for name, (fmt, text) in texts.items()}
    _, off, info, _ = got["fasta_empty_lines"]
    text = texts["fasta_empty_lines"][1]
    assert off.tolist() == [0, 4, 8] and not text.endswith(b"\n")
    assert any(text[r * T.REGION:(r + 1) * T.REGION] == b"\n" * T.REGION for r in range(1, 2)) and text.count(b"\r\n" * 16) >= 500
    for name in ("fastq_long_line", "fasta_long_line"):
        text = texts[name][1]
        assert text.index(b"\n") == T.REGION - 2 and got[name][1].tolist() == [0, 3 * T.REGION + 5, 3 * T.REGION + 9]
    for name in ("fastq_odd_bytes", "fasta_odd_bytes"):
        text, info = texts[name][1], got[name][2]
        assert all(bytes([b]) in text for b in T.ODD_BYTES) and all(b not in (0x0A, 0x0D) for b in T.ODD_BYTES)
        assert sorted(b ^ 0x0A for b in T.NEAR_NEWLINE) == [1 << i for i in range(8)]
        assert info["n_records"] == 13 and info["nb_bad_reads"] == 7 and info["nb_bad_bases"] == 5 + 16 + 1 + (16 if name == "fasta_odd_bytes" else 0)
    for name in ("fastq_all_empty", "fasta_all_empty", "fasta_header_alone"):
        _, off, info, _ = got[name]
        assert info["n_kept"] == info["n_records"] == off.size - 1 and not off.any() and info["n_bases"] == 0
    for name in ("fastq_all_dropped", "fasta_all_dropped"):
        _, off, info, _ = got[name]
        assert info["n_kept"] == 0 and info["n_records"] == 2 and off.tolist() == [0]
    assert got["fasta_cr_one_record"][0].tobytes() == b"ACGT" and got["fasta_cr_one_record"][2]["n_kept"] == 1
    assert got["fasta_cr_two_records"][0].tobytes() == b"ACGTGGTT" and got["fasta_cr_two_records"][1].tolist() == [0, 4, 8]
    assert got["fasta_cr_empty_last_line"][0].tobytes() == b"ACGT" and got["fasta_cr_header_last"][1].tolist() == [0, 4, 4]
    assert got["fastq_cr"][0].tobytes() == b"ACGTACGGTT" and M.ingest_fastq_qual(texts["fastq_cr"][1])[1].tobytes() == b"IIII%%7777"
    assert got["fastq_cr_empty_record"][1].tolist() == [0, 0]
    assert set(T.trailing_cr_texts()) <= set(texts) and all(t.endswith(b"\r") for _, t in T.trailing_cr_texts().values())
