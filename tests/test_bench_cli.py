"""bench.py command line: --dump-outputs writes what the timed path returned,
a plain run skips the --full legs, --steps sets the timed step count."""

import json
import os
import subprocess
import sys

import numpy as np
import pandas
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Result:
    def __init__(self, pdf):
        self._pdf = pdf

    def to_pandas(self):
        return self._pdf


def test_dump_outputs_small_and_sampled(tmp_path, monkeypatch):
    """Under the cap every group is written; over it, the same seeded row
    sample of every array, identical from call to call."""
    n = 1000
    pdf = pandas.DataFrame(
        {"v": np.arange(n) * 0.5},
        index=pandas.Index(np.arange(n, dtype=np.int64) * 3, name="k"))
    bench.dump_outputs(_Result(pdf), str(tmp_path / "all"))
    k = np.load(tmp_path / "all" / "index_k.npy")
    v = np.load(tmp_path / "all" / "v.npy")
    assert k.dtype == v.dtype == np.float64
    np.testing.assert_array_equal(k, pdf.index.to_numpy())
    np.testing.assert_array_equal(v, pdf["v"].to_numpy())

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 8 * 100)
    for d in ("a", "b"):
        bench.dump_outputs(_Result(pdf), str(tmp_path / d))
    ka = np.load(tmp_path / "a" / "index_k.npy")
    va = np.load(tmp_path / "a" / "v.npy")
    assert ka.shape == va.shape == (100,)
    assert ka.nbytes + va.nbytes <= bench.DUMP_MAX_BYTES
    assert (np.diff(ka) > 0).all()                 # a subset, in result order
    np.testing.assert_array_equal(va, ka / 3 * 0.5)  # same rows in each array
    np.testing.assert_array_equal(ka, np.load(tmp_path / "b" / "index_k.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_last_step(gpu_ready, tmp_path):
    """A plain run at a small odd size: the result line, and the dumped
    arrays against the oracle regeneration of the seeded device draws."""
    rows, keys, steps = 200_003, 1000, 3
    out = tmp_path / "dump"
    p = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", str(steps), "--warmup", "1", "--rows", str(rows),
         "--keys", str(keys), "--dump-outputs", str(out)],
        capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "verify ok" not in p.stderr            # the parity gate is --full
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["cpu_baseline"] is None
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(rows / (line["ms_per_step"] / 1e3))
    # per-kernel launch counts cover the timed steps only
    kern = line["roofline"]["kernel_ms"]
    assert all(c % steps == 0 for c, _ in kern.values()), kern

    exp_keys, exp_sums = bench.expected_tables(rows, keys, 0, [rows],
                                               "uniform")
    k = np.load(out / "index_k.npy")
    v = np.load(out / "v.npy")
    assert k.dtype == v.dtype == np.float64
    np.testing.assert_array_equal(k, exp_keys)
    np.testing.assert_allclose(v, exp_sums, rtol=1e-12, atol=1e-9)
