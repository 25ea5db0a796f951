"""CPU tests of bench.py's host-side pieces: the --dump-outputs writer (names, dtype, the size cap and its seeded sample) and
the refusal of step / repetition counts that would time nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _rows(n, seed=1):
    rng = np.random.default_rng(seed)
    return {"wrench": rng.standard_normal((n, 6)), "sdot": rng.standard_normal((n, 6)),
            "counts": rng.integers(0, 1000, (n, 4)).astype(np.int32)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_writes_every_row_below_the_limit(tmp_path):
    rows = _rows(100)
    ids = np.arange(100) * 3
    r = bench.dump_outputs(str(tmp_path), ids, rows)
    assert r["files"] == ["counts.npy", "item_ids.npy", "sdot.npy", "wrench.npy"] and not r["sampled"]
    got = _load(str(tmp_path))
    assert sorted(got) == ["counts", "item_ids", "sdot", "wrench"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["item_ids"], ids)
    for k, v in rows.items():
        assert np.array_equal(got[k], v), k          # the int32 counts are exact in float64


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    n = 5000
    rows = _rows(n)
    row_bytes = 8 * (1 + 6 + 6 + 4)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 4096 + 1000 * row_bytes)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ra = bench.dump_outputs(a, np.arange(n), rows)
    rb = bench.dump_outputs(b, np.arange(n), rows)
    assert ra["sampled"] and ra["items_written"] == 1000 and ra["items_computed"] == n
    ga, gb = _load(a), _load(b)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= bench.DUMP_LIMIT_BYTES
    ids = ga["item_ids"].astype(np.int64)
    assert np.all(np.diff(ids) > 0)                   # a subset, in item order
    assert np.array_equal(ga["item_ids"], gb["item_ids"])      # the same sample every time
    for k, v in rows.items():
        assert np.array_equal(ga[k], v[ids]), k


@pytest.mark.parametrize("args", [["--steps", "0"], ["--reps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_counts_that_time_nothing(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "at least" in p.stderr, p.stderr
