"""FASTQ / FASTA texts whose line ends fall on the edges of the ingest's walk (kmu_ingest.hip): a lane's 16-byte chunk, a wave's step
of 1 024 bytes, a region of 16 384 bytes, and the loop and tile edges of the scans (1 024, 8 192, 32 768 values).  Deterministic
builders on seeded numpy generators, and the plain readers that serve as the second reference: a helper for the tests, not a test."""
import numpy as np

import read_stats_model as M

REGION = 16384
# the last and first byte of a lane's chunk, of a wave's step and of a region, and one chunk past each
POSITIONS = (143, 144, 159, 160, 1023, 1024, 1039, 1040, 16383, 16384, 16385, 16399, 16400, 32767, 32768, 49151, 49152)
LINE_ENDS = (b"\n", b"\r\n")
FASTQ_LINES = (0, 1, 2, 3)  # header, sequence, separator, quality
FASTA_LINES = ("hdr", "seq", "empty", "lastseq")
END_SIZES = (16368, 16383, 16384, 16385, 32768)  # a full last region, one that holds one byte, a tail chunk of 0, 1 and 15 bytes
RECORD_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 8191, 8192, 8193, 32767, 32768, 32769, 40960, 40961)
# '\n' with one bit flipped (the classifier of newline_mask16 must not take them for a line end), and the two constant bytes
NEAR_NEWLINE = bytes([0x0B, 0x08, 0x0E, 0x02, 0x1A, 0x2A, 0x4A, 0x8A])
ODD_BYTES = bytes([0x00, 0xFF]) + NEAR_NEWLINE
INFO_NAMES = ("n_records", "n_kept", "kept_bases", "n_bases", "nb_bad_bases", "nb_bad_reads")

_ACGT = np.frombuffer(b"ACGTacgt", np.uint8)


def _seq(rng, length, with_n=False):
    s = rng.choice(_ACGT, length)
    if with_n:
        s[int(rng.integers(0, length))] = ord("N")
    return s.tobytes()


def _qual(rng, length, first=None):
    q = rng.integers(0x21, 0x7F, length).astype(np.uint8)
    if first is not None and length:
        q[0] = first
    return q.tobytes()


# ---- a line end at a given byte -----------------------------------------------------------------------------------------------
def place_fastq(P, line, nl, final_newline):
    """six records, records 1 and 4 with one N each; the '\\n' that ends line `line` of record 2 is byte P of the text (the padded
    header of record 2 puts it there), with nl == "\\r\\n" the '\\r' is byte P - 1"""
    rng = np.random.default_rng([P, line, len(nl), int(final_newline)])
    lens = (12, 11, 17, 1, 33, 16)
    recs = []
    for i, length in enumerate(lens):
        # a quality line may open with '@' or '+'
        recs.append([b"@r%d" % i, _seq(rng, length, with_n=i in (1, 4)), b"+" + (b"r%d tail" % i if i % 2 else b""),
                     _qual(rng, length, first=(ord("@"), None, ord("+"))[i % 3])])
    before = sum(len(x) + len(nl) for r in recs[:2] for x in r) + sum(len(x) + len(nl) for x in recs[2][:line + 1])
    pad = P + 1 - before
    assert pad >= 0, "position %d lies before the line" % P
    recs[2][0] += b" " + b"x" * (pad - 1) if pad else b""
    text = nl.join(x for r in recs for x in r) + (nl if final_newline else b"")
    assert text[P:P + 1] == b"\n" and (nl == b"\n" or text[P - 1:P] == b"\r")
    assert text[:P].count(b"\n") == 8 + line
    return text


def place_fasta(P, what, nl, final_newline):
    """six records: record 2 has a header, a sequence line, an empty line and a last sequence line, and the '\\n' that ends its line
    `what` is byte P; records 1 and 4 hold an N; record 3 is a header alone, so its header and that of record 4 are neighbours"""
    rng = np.random.default_rng([P, FASTA_LINES.index(what), len(nl), int(final_newline)])
    recs = [[b">r0 first", _seq(rng, 12)],
            [b">r1", _seq(rng, 11, with_n=True)],
            [b">r2", _seq(rng, 17), b"", _seq(rng, 9)],
            [b">r3 a header alone"],
            [b">r4 some>thing", _seq(rng, 20), _seq(rng, 20, with_n=True), _seq(rng, 3)],
            [b">r5", _seq(rng, 33), _seq(rng, 16)]]
    upto = FASTA_LINES.index(what) + 1
    before = sum(len(x) + len(nl) for r in recs[:2] for x in r) + sum(len(x) + len(nl) for x in recs[2][:upto])
    pad = P + 1 - before
    assert pad >= 0, "position %d lies before the line" % P
    recs[2][0] += b" " + b"x" * (pad - 1) if pad else b""
    text = nl.join(x for r in recs for x in r) + (nl if final_newline else b"")
    assert text[P:P + 1] == b"\n" and (nl == b"\n" or text[P - 1:P] == b"\r")
    assert text[:P].count(b"\n") == 4 + upto - 1
    return text


def placed_texts(fmt, line):
    """(P, nl, final_newline, text) of every placed text of one line kind"""
    build = place_fastq if fmt == "fastq" else place_fasta
    return [(P, nl, fin, build(P, line, nl, fin)) for P in POSITIONS for nl in LINE_ENDS for fin in (True, False)]


# ---- a text of a given length -------------------------------------------------------------------------------------------------
def end_at(n_bytes, fmt, final_newline, nl):
    """a text of exactly n_bytes: five records, record 3 with an N; the sequence of the last record takes up the slack (FASTQ: with
    its quality line, and one byte of its header where the slack is odd)"""
    rng = np.random.default_rng([n_bytes, fmt == "fastq", int(final_newline), len(nl)])
    end = nl if final_newline else b""
    if fmt == "fastq":
        head = b"".join(b"@e%d" % i + nl + _seq(rng, n, with_n=i == 3) + nl + b"+" + nl + _qual(rng, n) + nl
                        for i, n in enumerate((40, 1, 300, 25)))
        slack = n_bytes - len(head) - len(b"@e4+") - 3 * len(nl) - len(end)
        assert slack >= 2
        length = slack // 2
        text = head + b"@e4" + b"x" * (slack % 2) + nl + _seq(rng, length) + nl + b"+" + nl + _qual(rng, length) + end
    else:
        head = b"".join(b">e%d" % i + nl + _seq(rng, n, with_n=i == 3) + nl for i, n in enumerate((40, 1, 300, 25)))
        head += b">e4" + nl + _seq(rng, 60) + nl + _seq(rng, 60) + nl
        slack = n_bytes - len(head) - len(end)
        assert slack >= 1
        text = head + _seq(rng, slack) + end
    assert len(text) == n_bytes
    return text


# ---- record and line counts on the scans' edges -------------------------------------------------------------------------------
def many_records(n, fmt):
    """FASTQ: n records with 0 .. 3 bases, an N in about 30 % of those with two or more.  FASTA: n lines, each a header, one base
    or empty, an N in place of about one base in ten.  Irregular lengths and drops, so that a wrong scan offset shows"""
    rng = np.random.default_rng([n, fmt == "fastq"])
    if fmt == "fastq":
        lens = rng.integers(0, 4, n)
        drop = np.flatnonzero((lens >= 2) & (rng.random(n) < 0.3))
        bases = rng.choice(_ACGT, (n, 3))
        bases[drop, rng.integers(0, 3, drop.size) % lens[drop]] = ord("N")
        rows = bases.tobytes()
        return b"".join(b"@\n" + rows[3 * i:3 * i + length] + b"\n+\n" + b"III"[:length] + b"\n" for i, length in enumerate(lens.tolist()))
    kind = rng.choice(3, n, p=[0.3, 0.5, 0.2])  # header, one base, empty
    kind[0] = 0
    base = rng.choice(np.frombuffer(b"ACGTN", np.uint8), n, p=[0.225, 0.225, 0.225, 0.225, 0.1])
    return b"".join((b">", bytes([b]), b"")[k] + b"\n" for k, b in zip(kind.tolist(), base.tolist()))


# ---- special texts ------------------------------------------------------------------------------------------------------------
def _odd_fastq():
    odd = ODD_BYTES
    recs = [b"@h" + odd + b"\nACGTACGTACGTACGTAC\n+" + odd + b"\n" + (odd * 2)[:18] + b"\n"]
    for i, b in enumerate(odd):  # one odd byte after another in header, separator and quality line; the near-newlines in a sequence too
        seq = b"ACGTACG" + (bytes([b]) if i % 2 else b"T") + b"ACGTACGTAC"
        recs.append(b"@" + bytes([b]) * (i + 1) + b"\n" + seq + b"\n+" + bytes([b]) + b"\n" + bytes([b]) * len(seq) + b"\n")
    recs.append(b"@x\n" + bytes([0x8A]) * 16 + b"\n+\n" + bytes([0x0B]) * 16 + b"\n")
    recs.append(b"@y\n" + bytes([0x0B]) + b"ACGT\n+\n" + bytes([0x8A]) + b"IIII\n")
    return b"".join(recs)


def _odd_fasta():
    odd = ODD_BYTES
    recs = [b">h" + odd + b"\nACGTACGTACGTACGTAC\nGGT\n"]
    for i, b in enumerate(odd):
        recs.append(b">" + bytes([b]) * (i + 1) + b"\nACGTACG" + (bytes([b]) if i % 2 else b"T") + b"\nACGTACGTAC\n")
    recs.append(b">x\n" + bytes([0x8A]) * 16 + b"\n" + bytes([0x0B]) * 16 + b"\n")
    recs.append(b">y\nAC\n" + bytes([0x0B]) + b"\nGT\n")
    return b"".join(recs)


def _long_line(fmt):
    rng = np.random.default_rng(77)
    seq = _seq(rng, 3 * REGION + 5)
    first = b"@" if fmt == "fastq" else b">"
    text = first + b"h" * (REGION - 3) + b"\n"
    assert len(text) % REGION == REGION - 1  # the first base is the last byte of region 0
    if fmt == "fastq":
        return text + seq + b"\n+\n" + _qual(rng, len(seq)) + b"\n@s\nACGT\n+\nIIII\n"
    return text + seq + b"\n>s\nACGT\n"


def special_texts():
    """name -> (format, text)"""
    t = {}
    # regions whose newline count is the largest there is: every chunk mask 0xFFFF; then "\r\n" pairs, and no final newline
    # (the first record fills region 0, so that region 1 is newlines from end to end)
    t["fasta_empty_lines"] = ("fasta", b">a" + b" " * (REGION - 8) + b"\nACGT\n" + b"\n" * 20000 + b">b\r\nAC\r\n" + b"\r\n" * 9000 + b"GT")
    t["fastq_long_line"] = ("fastq", _long_line("fastq"))
    t["fasta_long_line"] = ("fasta", _long_line("fasta"))
    t["fastq_odd_bytes"] = ("fastq", _odd_fastq())
    t["fasta_odd_bytes"] = ("fasta", _odd_fasta())
    t["fastq_all_empty"] = ("fastq", b"@a\n\n+\n\n" * 3)
    t["fasta_all_empty"] = ("fasta", b">a\n>b\n")
    t["fasta_header_alone"] = ("fasta", b">a")
    t["fastq_all_dropped"] = ("fastq", b"@a\nNN\n+\nII\n@b\nACNT\n+\nIIII\n")
    t["fasta_all_dropped"] = ("fasta", b">a\nNN\n>b\nAC\nNT\n")
    t.update(trailing_cr_texts())
    return t


def trailing_cr_texts():
    """a '\\r' ends the text, no '\\n' after it: it belongs to the line end, not to the line"""
    return {
        "fasta_cr_one_record": ("fasta", b">r\r\nACGT\r"),
        "fasta_cr_two_records": ("fasta", b">r\r\nACGT\r\n>s\r\nGG\r\nTT\r"),
        "fasta_cr_empty_last_line": ("fasta", b">r\r\nACGT\r\n\r"),
        "fasta_cr_header_last": ("fasta", b">r\r\nACGT\r\n>s\r"),
        "fastq_cr": ("fastq", b"@a\r\nACGTAC\r\n+\r\nIIII%%\r\n@b\r\nGGTT\r\n+\r\n7777\r"),
        "fastq_cr_empty_record": ("fastq", b"@a\r\n\r\n+\r\n\r"),
    }


# ---- the plain readers --------------------------------------------------------------------------------------------------------
def read_fasta(text):
    """the sequences of a FASTA text: split on "\\n", one trailing "\\r" stripped per line, a line that starts with '>' opens a record"""
    lines = bytes(text).split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    records = []
    for line in lines:
        if line.startswith(b">"):
            records.append([])
        else:
            records[-1].append(line[:-1] if line.endswith(b"\r") else line)
    return [b"".join(r) for r in records]


def read_fastq(text):
    return [s for s, _ in M.parse_fastq(text)]


def plain_ingest(text, fmt):
    """(bases, offsets, info dict, record_index) as the oracle's ingest returns them, from the plain readers"""
    seqs = read_fastq(text) if fmt == "fastq" else read_fasta(text)
    bad = [int((M.BASE_CLASS[np.frombuffer(s, np.uint8)] == 4).sum()) for s in seqs]
    kept = [i for i, b in enumerate(bad) if b == 0]
    bases = np.frombuffer(b"".join(seqs[i] for i in kept), np.uint8)
    offsets = np.cumsum([0] + [len(seqs[i]) for i in kept]).astype(np.uint64)
    info = dict(n_records=len(seqs), n_kept=len(kept), kept_bases=int(offsets[-1]), n_bases=sum(len(s) for s in seqs),
                nb_bad_bases=sum(bad), nb_bad_reads=sum(1 for b in bad if b))
    return bases, offsets, info, np.array(kept, np.uint32)
