"""GPU tier: the order-preserving compaction (hf_filter_plan / hf_filter_apply /
hf_filter_iota) element-wise against boolean indexing, at the sizes and masks
where the tile counts, the one-block tile scan and the ballot rank go wrong.
Everything here is exact: f64 columns are compared on their int64 bit view, so
NaN payloads and -0.0 count."""

import numpy as np
import pytest

from modin_amd.core import lib
from tests import scan_refs as sr
from tests.scan_refs import TILE

pytestmark = pytest.mark.gpu

ITER = 1024 * TILE

# as the scan sizes: a thread's 16 rows, a 256-row chunk of the scatter loop,
# a tile, 3 tiles and a tail, and the first count with a second iteration of
# k_compact_scan's 1024-tile loop
SIZES = [1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
         3 * TILE + 5, ITER + 4097]


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _rows(n, rows):
    m = np.zeros(n, dtype=np.int64)
    m[rows] = 1
    return m


def _masks(rng, n):
    i = np.arange(n)
    # n_kept == 0: apply and iota return empty columns of the right dtype
    yield "none", np.zeros(n, dtype=np.int64)
    # n_kept == n: every tile count is full, output equals input
    yield "all", np.ones(n, dtype=np.int64)
    # the first output slot comes from the first row alone
    yield "row 0", _rows(n, [0])
    # the last row of the tail tile, every tile base before it is 0
    yield "row n-1", _rows(n, [n - 1])
    # lane 0 of every wave: rank 0 under an empty below-mask
    yield "lane 0", (i % 64 == 0).astype(np.int64)
    # lane 63 of every wave: the lane == 63 branch of the ballot-rank mask
    yield "lane 63", (i % 64 == 63).astype(np.int64)
    # the last thread of every 256-row chunk: wave_base over three waves
    yield "thread 255", (i % 256 == 255).astype(np.int64)
    # the first / the last row of every tile: the tile base alone places it
    yield "tile first", (i % TILE == 0).astype(np.int64)
    yield "tile last", (i % TILE == TILE - 1).astype(np.int64)
    yield "half", (rng.random(n) < 0.5).astype(np.int64)
    # most tiles keep nothing at all
    yield "sparse", (rng.random(n) < 0.001).astype(np.int64)
    # any nonzero value counts as kept, not only 1
    yield "sevens", (rng.random(n) < 0.5).astype(np.int64) * 7


def _f64_with_payloads(rng, n):
    """Random doubles with -0.0, +-inf and NaNs of assorted sign and
    payload among them: only a bit-view comparison tells them apart."""
    x = rng.normal(0.0, 1.0, n)
    special = np.array([0x8000000000000000, 0x7FF8000000000000,
                        0xFFF8000000000001, 0x7FF0000000000001,
                        0x7FFFFFFFFFFFFFFF, 0x7FF0000000000000,
                        0xFFF0000000000000], dtype=np.uint64).view(np.float64)
    at = rng.random(n) < 0.2
    x[at] = rng.choice(special, int(at.sum()))
    return x


@pytest.mark.parametrize("n", SIZES)
def test_filter_vs_boolean_indexing(n):
    rng = np.random.default_rng(n)
    xf = _f64_with_payloads(rng, n)
    xi = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n,
                      endpoint=True)
    cf, ci = lib.put(xf), lib.put(xi)
    for what, mask in _masks(rng, n):
        what = (what, n)
        plan = lib.filter_plan(lib.put(mask))
        assert plan.n_kept == int(np.count_nonzero(mask)), what
        gf = lib.filter_apply(plan, cf)
        gi = lib.filter_apply(plan, ci)
        assert gf.np_dtype == np.float64 and gi.np_dtype == np.int64, what
        assert gf.length == gi.length == plan.n_kept, what
        gf, gi = lib.get(gf), lib.get(gi)
        assert gf.dtype == np.float64 and gi.dtype == np.int64, what
        assert np.array_equal(gf.view(np.int64),
                              sr.ref_filter(mask, xf).view(np.int64)), what
        assert np.array_equal(gi, sr.ref_filter(mask, xi)), what
        # base 0, and a base that does not fit 32 bits
        for base in (0, 2**40 + 3):
            it = lib.filter_iota(plan, base)
            assert it.np_dtype == np.int64 and it.length == plan.n_kept, what
            assert np.array_equal(lib.get(it),
                                  sr.ref_filter_iota(mask, base)), what


def test_length_mismatch_is_rejected():
    plan = lib.filter_plan(lib.put(np.ones(10, dtype=np.int64)))
    for col in (np.arange(9.0), np.arange(11, dtype=np.int64)):
        with pytest.raises(lib.HfError, match=r"rc=2"):
            lib.filter_apply(plan, lib.put(col))
