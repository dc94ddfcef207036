"""GPU tier: the radix groupby plan with a tile-major payload.  The record and
the replay write each 12288-row tile's bucket-sorted staging verbatim at
tile * TILE, and P2 fetches a bucket's run out of each tile through the plan's
bucket-major run table and its (bucket, tile range) work items.

Every case first asserts through hf_groupby_radix_rl which geometry it runs,
then checks both routes against oracle.groupby_agg:
  * groupby_accum + groupby_compact — touch bytes and the atomic merge;
  * groupby_reduce — the arming call, then mapped calls through the partial
    table flush and k_gb_combine.
Each route gets one recording call and at least two replayed calls with fresh
values.  Contract: keys, presence and counts exact; f64 values rtol=1e-12,
atol=1e-9; integer-valued data exactly equal.

Sizes are the smallest at which this layout can go wrong: the tile is 12288
rows, buckets hold 16384 / 8192 / 4096 slots, a work item is cut below 2^21
rows, a P2 wave takes up to 64 tiles at a time and reads runs of up to 8 rows
one per lane.  HF_GB_NT_STORE (read once per process, hence the child process
at the end) switches the flavour of the replay's stores.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from modin_amd.core import lib

pytestmark = pytest.mark.gpu

TILE = 12288
RTOL, ATOL = 1e-12, 1e-9
AGG_NAME = {lib.AGG_SUM: "sum", lib.AGG_MIN: "min", lib.AGG_MAX: "max"}
SPAN14 = 2**18 + 1
SPAN14_EDGE = -(-SPAN14 // 16384) * 16384
# name -> (span, want_counts, log2 of the bucket width it must run at)
GEOMS = {
    "rl14": (SPAN14, False, 14),
    "rl14_edge": (SPAN14_EDGE, False, 14),
    "rl13": (8193, False, 13),
    "rl13_wide": (3 * 8192 + 5, False, 13),
    "rl12_counts": (3 * 4096 + 1, True, 12),
}
DEFAULT_NT_STORE = "1"   # the library's flavour when the variable is unset
ROW_COUNTS = [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 2]


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _geometry(name):
    """The geometry this test means to run, asserted before it runs."""
    span, wc, rl = GEOMS[name]
    assert lib.groupby_radix_rl(span, wc) == rl, (name, span, wc)
    return span, wc, 1 << rl


def _keys(rng, n, span, bucket):
    """Uniform keys over [0, span) with the range ends and the slots on both
    sides of the first bucket edge pinned (as far as n allows)."""
    k = rng.integers(0, span, n).astype(np.int64)
    for at, slot in list(zip((n - 1, 0, n - 2, 1),
                             (span - 1, 0, bucket - 1, bucket)))[:n]:
        k[at] = slot
    return k


def _ints(rng, n):
    """Integer-valued f64 data: every partial sum is exact in any order."""
    return rng.integers(-1000, 1000, n).astype(np.float64)


def _two_call(key_col, vals, agg_op, span, wc):
    nv = len(vals)
    val_cols = [lib.put(v) for v in vals]
    sums = lib.alloc_raw(8 * max(nv, 1) * span)
    rowcnt = lib.alloc_raw(8 * span)
    counts = lib.alloc_raw(8 * nv * span) if wc and nv else 0
    try:
        lib.fill_f64(sums, lib.AGG_IDENTITY[agg_op], max(nv, 1) * span)
        lib.memset_raw(rowcnt, 0, 8 * span)
        if counts:
            lib.memset_raw(counts, 0, 8 * nv * span)
        lib.groupby_accum(key_col, val_cols, agg_op, 0, span, sums, rowcnt,
                          counts)
        k, s, c, n = lib.groupby_compact(sums, rowcnt, counts, nv, 0, span)
        assert k.length == n
        return (lib.get(k), [lib.get(x) for x in s],
                [lib.get(x) for x in c] if counts else None)
    finally:
        lib.free_raw(sums)
        lib.free_raw(rowcnt)
        if counts:
            lib.free_raw(counts)


def _reduce(key_col, vals, agg_op, span, wc):
    val_cols = [lib.put(v) for v in vals]
    k, s, c, n = lib.groupby_reduce(key_col, val_cols, agg_op, wc, 0, span)
    assert k.length == n
    return (lib.get(k), [lib.get(x) for x in s],
            [lib.get(x) for x in c] if wc else None)


def _expected(keys, vals, agg_op):
    named = {str(i): v for i, v in enumerate(vals)}
    ok, oexp = oracle.groupby_agg(keys, named, AGG_NAME[agg_op])
    _, ocnt = oracle.groupby_agg(keys, named, "count")
    return ok, oexp, ocnt


def _check(keys, vals, agg_op, got, wc=False, exact=False):
    """Keys exact; values against the oracle on the groups that hold a non-NaN
    value; a group without one keeps the aggregate's identity."""
    ok, oexp, ocnt = _expected(keys, vals, agg_op)
    np.testing.assert_array_equal(got[0], ok)
    assert len(got[1]) == len(vals)
    for i in range(len(vals)):
        live = ocnt[str(i)] > 0
        g, e = got[1][i], oexp[str(i)]
        if exact:
            np.testing.assert_array_equal(g[live], e[live])
        else:
            np.testing.assert_allclose(g[live], e[live], rtol=RTOL, atol=ATOL)
        assert (g[~live] == lib.AGG_IDENTITY[agg_op]).all()
        if wc:
            np.testing.assert_array_equal(got[2][i], ocnt[str(i)])


def _both_routes(keys, geom, make_vals, agg_op=lib.AGG_SUM, calls=3,
                 exact=False):
    """Each route on a key column of its own: one recording (arming) call, then
    replayed (mapped) calls, every call with fresh values."""
    span, wc, _ = _geometry(geom)
    for route in (_two_call, _reduce):
        key_col = lib.put(keys)
        for _ in range(calls):
            vals = make_vals()
            _check(keys, vals, agg_op, route(key_col, vals, agg_op, span, wc),
                   wc, exact)


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_and_geometries(n, geom):
    """The odd last row (a row of the last tile), a partial last tile, and
    every geometry; at rl14_edge the last bucket is full."""
    span, _, bucket = _geometry(geom)
    rng = np.random.default_rng(1000 * n + span)
    keys = _keys(rng, n, span, bucket)
    _both_routes(keys, geom, lambda: [_ints(rng, n)], exact=True)


@pytest.mark.parametrize("geom", ["rl14", "rl13_wide", "rl12_counts"])
def test_sorted_keys(geom):
    """Ascending keys: one or two runs per tile, most descriptors empty, and
    an item's few tiles shared out among the waves."""
    span, _, bucket = _geometry(geom)
    rng = np.random.default_rng(2000 + span)
    n = 3 * TILE + 2
    keys = np.sort(_keys(rng, n, span, bucket))
    _both_routes(keys, geom, lambda: [_ints(rng, n)], exact=True)
    _both_routes(keys, geom, lambda: [rng.standard_normal(n)])


@pytest.mark.parametrize("geom", ["rl14", "rl13_wide"])
def test_bucket_only_in_the_odd_last_row(geom):
    span, _, bucket = _geometry(geom)
    rng = np.random.default_rng(3000 + span)
    n = 2 * TILE + 1
    keys = rng.integers(0, bucket, n).astype(np.int64)
    keys[n - 1] = span - 1                     # the last bucket's only row
    keys[0] = 0
    assert (keys >= bucket).sum() == 1
    _both_routes(keys, geom, lambda: [_ints(rng, n)], exact=True)


@pytest.mark.parametrize("geom", ["rl14", "rl13_wide", "rl12_counts"])
def test_one_row_and_three_rows_per_tile(geom):
    """Bucket 1 has exactly one row in every tile and bucket 2 exactly three,
    behind an odd number of bucket-0 rows: odd starts and odd lengths, read a
    lane per run."""
    span, _, bucket = _geometry(geom)
    rng = np.random.default_rng(4000 + span)
    ntiles = 5
    n = ntiles * TILE - 7                      # odd, partial last tile
    keys = rng.integers(0, bucket, n).astype(np.int64)
    for t in range(ntiles):
        at = t * TILE + 2 + rng.choice(TILE - 9, 4, replace=False)
        keys[at[0]] = bucket + 9
        keys[at[1:]] = 2 * bucket + rng.integers(0, 50, 3)
    keys[0] = 0
    keys[1] = span - 1
    _both_routes(keys, geom, lambda: [_ints(rng, n)], exact=True)
    _both_routes(keys, geom, lambda: [rng.standard_normal(n)])


@pytest.mark.parametrize("geom", ["rl14_edge", "rl13_wide"])
def test_one_key_holds_most_rows(geom):
    """90 % of the rows on one key: a head run that fills most of each tile
    beside runs of a row or two, and the register run-accumulator."""
    span, _, bucket = _geometry(geom)
    rng = np.random.default_rng(5000 + span)
    n = 3 * TILE + 1
    keys = _keys(rng, n, span, bucket)
    head = rng.random(n) < 0.9
    head[[0, 1, n - 2, n - 1]] = False         # keep the pinned edge keys
    keys[head] = bucket + 77
    _both_routes(keys, geom, lambda: [_ints(rng, n)], exact=True)
    _both_routes(keys, geom, lambda: [rng.standard_normal(n)])


def test_bucket_above_the_item_cut():
    """Bucket 0 holds more than 2^21 rows, so its items are cut between tiles
    and the atomic merge and k_gb_combine fold more than one table."""
    span, _, bucket = _geometry("rl14")
    rng = np.random.default_rng(6000)
    n = 2**21 + 2 * TILE + 1
    keys = rng.integers(0, bucket, n).astype(np.int64)
    far = rng.choice(n - 2, 40, replace=False) + 1
    keys[far] = rng.integers(bucket, span, 40)
    keys[0], keys[n - 1] = 0, span - 1
    assert (keys < bucket).sum() > 2**21
    _both_routes(keys, "rl14", lambda: [_ints(rng, n)], exact=True)


def test_bucket_of_exactly_2_21_rows():
    span, _, bucket = _geometry("rl14")
    rng = np.random.default_rng(6001)
    n = 2**21 + 5
    keys = rng.integers(bucket, 2 * bucket, n).astype(np.int64)
    keys[[0, 7, TILE, n - 2, n - 1]] = [0, 3 * bucket, 5, span - 1, 1]
    assert ((keys >= bucket) & (keys < 2 * bucket)).sum() == 2**21
    _both_routes(keys, "rl14", lambda: [_ints(rng, n)], exact=True)


@pytest.mark.parametrize("agg_op", [lib.AGG_SUM, lib.AGG_MIN, lib.AGG_MAX])
@pytest.mark.parametrize("geom", ["rl14", "rl12_counts"])
def test_nans_min_max_counts(agg_op, geom):
    """30 % NaNs and a group whose values are all NaN: it stays present, keeps
    the identity and counts zero."""
    span, wc, bucket = _geometry(geom)
    rng = np.random.default_rng(7000 + agg_op + span)
    n = 2 * TILE + 1
    keys = _keys(rng, n, span, bucket)
    lone = bucket + 5
    keys[7] = keys[TILE + 7] = lone

    def vals():
        v = rng.standard_normal(n)
        v[rng.random(n) < 0.3] = np.nan
        v[keys == lone] = np.nan
        return [v]

    _both_routes(keys, geom, vals, agg_op)


@pytest.mark.parametrize("geom", ["rl14_edge", "rl12_counts"])
def test_two_value_columns_and_keys_only(geom):
    span, wc, bucket = _geometry(geom)
    rng = np.random.default_rng(8000 + span)
    n = 2 * TILE + 1
    keys = _keys(rng, n, span, bucket)
    for first in ((2, 0, 1, 2), (0, 0, 2)):    # also keys-only as the record
        for route in (_two_call, _reduce):
            key_col = lib.put(keys)
            for nv in first:
                vals = [rng.standard_normal(n) for _ in range(nv)]
                _check(keys, vals, lib.AGG_SUM,
                       route(key_col, vals, lib.AGG_SUM, span, wc), wc)


@pytest.mark.parametrize("geom", ["rl14_edge", "rl13_wide"])
def test_out_of_range_keys_raise_on_every_call(geom):
    span, wc, bucket = _geometry(geom)
    rng = np.random.default_rng(9000 + span)
    n = TILE + 1
    keys = _keys(rng, n, span, bucket)
    short = span - 3                           # same geometry, 3 slots too few
    assert lib.groupby_radix_rl(short, wc) == GEOMS[geom][2]
    for route in (_two_call, _reduce):
        key_col = lib.put(keys)
        for _ in range(3):
            with pytest.raises(lib.HfError, match="outside"):
                route(key_col, [_ints(rng, n)], lib.AGG_SUM, short, wc)
        for _ in range(3):
            v = _ints(rng, n)
            _check(keys, [v], lib.AGG_SUM,
                   route(key_col, [v], lib.AGG_SUM, span, wc), wc, exact=True)


def test_range_change_rerecords():
    """(key_min, n_slots) changes on one key column: each change re-records
    the plan, its run table and its items."""
    rng = np.random.default_rng(10000)
    n = 2 * TILE + 1
    keys = _keys(rng, n, 8193, 8192)
    for route in (_two_call, _reduce):
        key_col = lib.put(keys)
        for span in (8193, 8193, 3 * 8192 + 5, 3 * 8192 + 5, SPAN14, SPAN14,
                     8193, 8193):
            v = _ints(rng, n)
            _check(keys, [v], lib.AGG_SUM,
                   route(key_col, [v], lib.AGG_SUM, span, False), exact=True)


def test_records_once_and_cuts_items_on_the_device():
    _geometry("rl14")
    rng = np.random.default_rng(11000)
    n = 2 * TILE + 1
    keys = _keys(rng, n, SPAN14, 16384)
    key_col = lib.put(keys)
    names = ["gb_plan_record", "gb_plan_items", "gb_scatter", "gb_keys32"]
    lib.profiling(True)
    lib.kernel_stats_reset()
    try:
        for _ in range(3):
            v = _ints(rng, n)
            _check(keys, [v], lib.AGG_SUM,
                   _two_call(key_col, [v], lib.AGG_SUM, SPAN14, False),
                   exact=True)
        got = {m: lib.kernel_stats(m)[0] for m in names}
    finally:
        lib.profiling(False)
    # the item pass runs with the record only: count, then fill
    assert got == {"gb_plan_record": 1, "gb_plan_items": 2, "gb_scatter": 2,
                   "gb_keys32": 0}


def test_other_store_flavour_child_process():
    """A subset of the cases above with the replay's store flavour switched
    (HF_GB_NT_STORE is read once per process, hence the fresh child)."""
    here = os.environ.get("HF_GB_NT_STORE", DEFAULT_NT_STORE)
    env = dict(os.environ, HF_GB_NT_STORE="0" if here == "1" else "1")
    res = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
         "-k", "row_counts or one_row_and_three or most_rows",
         os.path.abspath(__file__)],
        env=env, capture_output=True, text=True, timeout=600)
    tail = res.stdout[-3000:] + res.stderr[-1000:]
    assert res.returncode == 0, tail
    assert " passed" in res.stdout and "failed" not in res.stdout, tail
