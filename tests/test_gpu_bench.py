"""bench.py end to end at a small size (2 000 reads of the headline workload), each run a child process: a plain line only
times its steps, --full adds the per-kernel timers and the oracle checks, and --dump-outputs writes the same files whatever the
number of steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reads", "2000"] + list(args),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_line_full_line_and_dumped_outputs(tmp_path):
    a = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    assert a["steps"] == 3 and a["warmup"] == 1 and a["full"] is False and a["ms_per_step"] > 0 and a["value"] > 0
    for key in ("kernels", "roofline", "alu", "gpu_work", "checks", "cpu_baseline", "host_to_host", "configs"):
        assert a[key] is None, key
    b = _bench("--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "b"))
    assert b["steps"] == 1
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["count_sample.npy", "count_totals.npy", "signatures_hi32.npy", "signatures_lo32.npy"]
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64e6
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float64 and np.array_equal(x, y), n
    sig = np.load(tmp_path / "a" / "signatures_hi32.npy")
    assert sig.shape == (2000, 200) and sig.max() > 0
    tot = np.load(tmp_path / "a" / "count_totals.npy")
    kmers = a["config"]["kmers_per_gpu"]  # the occurrences held are the k-mers that went in, unless a count saturated
    assert 0 < tot[0] <= tot[2] and (tot[2] == kmers if tot[3] == 0 else tot[2] <= kmers)
    f = _bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-configs")
    assert f["full"] is True and f["kernels"] and f["roofline"] and f["host_to_host"]
    c = f["checks"]
    assert c["parity_rows_ok"] and c["parity_counts_ok"] and c["count_conservation_ok"] and c["host_leg_equals_device_leg"]
