"""`parsefastq --stats`, both tools: bases.histo, readlen.histo and quality.histo are byte for byte what kmerutils_amd/statutils.py
writes from the numpy model's tables; without the option none of them appears and the dump is the same file; on fewer than 100
reads readlen.histo is not written and the tool still ends with 0, as the reference discards that error (parsefastq.rs:200)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import read_stats_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
HISTOS = ("bases.histo", "readlen.histo", "quality.histo")


def fastq_text(n_reads, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n_reads):
        length = int(rng.integers(40, 2500))
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), length, p=[.35, .15, .2, .3])
        if i % 13 == 6:
            seq[int(rng.integers(0, length))] = ord("N")
        qual = rng.integers(0x21, 0x4B, length).astype(np.uint8)
        end = b"\r\n" if i % 9 == 2 else b"\n"
        recs.append(b"@r%d" % i + end + seq.tobytes() + end + b"+" + end + qual.tobytes() + end)
    return b"".join(recs)


def model_files(text, outdir):
    """the three files from the model's tables through statutils.py's dumps; None for a file that is not written"""
    from kmerutils_amd import statutils
    bases, quals, off, _ = M.ingest_fastq_qual(text)
    _, pct_hist, len_hist, info = M.read_stats(bases, off)
    d = statutils.ReadBaseDistribution(pct_hist, len_hist, info["n_reads"], info["histo_out"], info["n_other"], 1_000_000, 3)
    d.ascii_dump_acgt_distribution(str(outdir / "bases.histo"))
    d.ascii_dump_readlen_distribution(str(outdir / "readlen.histo"))
    _, hist = M.read_qual_stats(quals, off)
    (outdir / "quality.histo").write_text("".join("%d\t%d\n" % (c, hist[c]) for c in range(8)))
    return {name: (outdir / name).read_bytes() if (outdir / name).exists() else None for name in HISTOS}


def run_tools(fq, outdir, stats):
    """both tools into directories of their own; {tool: {file name: bytes}}"""
    from kmerutils_amd import build, parsefastq
    exe = [p for p in build.build_host() if p.endswith("parsefastq")][0]
    out = {}
    for tool in ("py", "cpp"):
        d = outdir / ("%s_%s" % (tool, "stats" if stats else "plain"))
        d.mkdir()
        extra = ["--stats"] if stats else []
        if tool == "py":
            assert parsefastq.main(["-f", str(fq), "-s", "21", "--outdir", str(d)] + extra) == 0
        else:
            r = subprocess.run([exe, "-f", str(fq), "kmer", "--count", "-s", "21", "--outdir", str(d)] + extra, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert ("nb read outside max size for histogram 0" in r.stderr) == stats
        out[tool] = {name: (d / name).read_bytes() for name in sorted(os.listdir(d))}
    return out


def test_stats_files_of_both_tools(tmp_path):
    text = fastq_text(300, 0x57A7)
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(text)
    model_dir = tmp_path / "model"
    model_dir.mkdir()
    want = model_files(text, model_dir)
    assert all(want[name] for name in HISTOS) and want["bases.histo"].count(b"\n") == 101 and want["quality.histo"].count(b"\n") == 8
    with_stats, plain = run_tools(fq, tmp_path, True), run_tools(fq, tmp_path, False)
    for tool in ("py", "cpp"):
        assert sorted(with_stats[tool]) == sorted(HISTOS + ("reads.fastq.multi_kmer.bin",)), tool
        for name in HISTOS:
            assert with_stats[tool][name] == want[name], (tool, name)
        assert sorted(plain[tool]) == ["reads.fastq.multi_kmer.bin"], tool  # none of the three files without the option
        assert plain[tool]["reads.fastq.multi_kmer.bin"] == with_stats[tool]["reads.fastq.multi_kmer.bin"], tool


def test_fewer_than_100_reads_write_no_readlen_histo(tmp_path):
    from kmerutils_amd import build
    text = fastq_text(50, 0x57A8)
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(text)
    model_dir = tmp_path / "model"
    model_dir.mkdir()
    want = model_files(text, model_dir)
    assert want["readlen.histo"] is None and want["bases.histo"] and want["quality.histo"]
    got = run_tools(fq, tmp_path, True)
    for tool in ("py", "cpp"):
        assert "readlen.histo" not in got[tool] and got[tool]["bases.histo"] == want["bases.histo"], tool
        assert got[tool]["quality.histo"] == want["quality.histo"], tool
    # the statistics alone: the C++ tool needs no k-mer task for them, the Python tool (which has no task word) takes --no-count
    from kmerutils_amd import parsefastq
    py_alone = tmp_path / "py_alone"
    py_alone.mkdir()
    assert parsefastq.main(["-f", str(fq), "--stats", "--no-count", "--outdir", str(py_alone)]) == 0
    assert sorted(os.listdir(py_alone)) == ["bases.histo", "quality.histo"] and (py_alone / "bases.histo").read_bytes() == want["bases.histo"]
    with pytest.raises(SystemExit):
        parsefastq.main(["-f", str(fq), "--no-count", "--outdir", str(py_alone)])
    alone = tmp_path / "alone"
    alone.mkdir()
    exe = [p for p in build.build_host() if p.endswith("parsefastq")][0]
    r = subprocess.run([exe, "-f", str(fq), "--stats", "--outdir", str(alone)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and sorted(os.listdir(alone)) == ["bases.histo", "quality.histo"], r.stderr[-2000:]
    assert (alone / "bases.histo").read_bytes() == want["bases.histo"]
