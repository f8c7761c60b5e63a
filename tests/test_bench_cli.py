"""bench.py's command line: a plain run prints the headline line only, --full adds the checks and the
per-kernel figures, --dump-outputs writes what the last timed step computed."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "cpu_baseline", "fullsize_parity", "guard_counts", "mismatches", "ratio")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_dump_sample_is_fixed_sorted_and_within_budget():
    import bench
    row = 1200 + 1024 + 8
    a, b = bench.dump_sample(10_000_000, row), bench.dump_sample(10_000_000, row)
    assert np.array_equal(a, b) and a.dtype == np.int64
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 10_000_000
    assert 4 * row * len(a) <= bench.DUMP_BUDGET_BYTES < 64 * 10 ** 6
    assert np.array_equal(bench.dump_sample(100, row), np.arange(100))


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs == "" and args.steps == 2


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    d = str(tmp_path / "out")
    res = _bench("--n", "4096", "--steps", "2", "--warmup", "1", "--dump-outputs", d)
    assert all(k in res for k in HEADLINE) and not any(k in res for k in FULL_ONLY), sorted(res)
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["unit"] == "GiB/s" and res["dtype"] == "u8"
    a = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sorted(a) == ["compress_rc", "compressed", "compressed_len", "decompress_rc", "decompressed",
                         "decompressed_len", "sample_index", "totals"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    assert np.array_equal(a["sample_index"], np.arange(4096))
    assert not a["compress_rc"].any() and not a["decompress_rc"].any()
    assert np.all(a["decompressed_len"] == 1024) and a["decompressed"].shape == (4096, 1024)
    assert list(a["totals"]) == [a["compressed_len"].sum(dtype=np.float64), 0.0, 4096 * 1024.0, 0.0]
    for k in (0, 1, 2047, 4095):
        n = int(a["compressed_len"][k])
        assert not a["compressed"][k, n:].any()
        assert gzip.decompress(a["compressed"][k, :n].astype(np.uint8).tobytes()) == \
            a["decompressed"][k].astype(np.uint8).tobytes()


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_kernel_figures():
    res = _bench("--n", "4096", "--steps", "1", "--warmup", "1", "--full", "--cpu-sample", "2000")
    assert all(k in res for k in HEADLINE + FULL_ONLY), sorted(res)
    assert res["mismatches"] == 0 and res["verified_values"] == 4096
    assert res["fullsize_parity"]["match"] is True and res["fullsize_parity"]["members"] == 4096
    assert res["roofline"]["kernel_ms_per_step"] and res["cpu_baseline"]["value"] > 0
