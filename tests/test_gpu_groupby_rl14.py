"""GPU tier: the radix groupby at 16384-slot buckets (RL = 14), the geometry
sum/min/max calls without counts take on key ranges above 2^18 slots.

Every case first asserts through hf_groupby_radix_rl which geometry it runs,
then checks both routes against oracle.groupby_agg:
  * groupby_accum + groupby_compact — the first call records the plan with the
    touch-byte P2 variant and the atomic merge, later calls replay it;
  * groupby_reduce — the arming call, then mapped calls through the partial
    table flush and k_gb_combine at RANGE = 16384.
Contract: keys and presence exact; f64 values rtol=1e-12, atol=1e-9, and
integer-valued sums exactly equal.  Calls with counts stay on 4096-slot
buckets and are only used here to force a geometry change.

Sizes are the smallest at which this geometry can go wrong: 2^18 + 1 slots is
the narrowest range that selects it, the plan tile is 12288 rows, a bucket
holds 16384 slots, a work item 2^21 rows.  With HF_GB_RL=13 (read once per
process, hence the child process at the end) the same cases run on 8192-slot
buckets.
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
BUCKET = 16384
RTOL, ATOL = 1e-12, 1e-9
SPAN_MIN = 2**18 + 1                      # narrowest range that selects 14
SPAN_EDGE = -(-SPAN_MIN // BUCKET) * BUCKET   # ... rounded up to a bucket edge
WANT_RL = 13 if os.environ.get("HF_GB_RL") == "13" else 14
AGG_NAME = {lib.AGG_SUM: "sum", lib.AGG_MIN: "min", lib.AGG_MAX: "max"}


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _geometry(span, want_counts=False):
    """The geometry this test means to run, asserted before it runs."""
    rl = lib.groupby_radix_rl(span, want_counts)
    assert rl == (12 if want_counts else WANT_RL), (span, want_counts, rl)


def _keys(rng, n, span):
    """Uniform keys over [0, span) with the range ends and the slots on both
    sides of the first bucket edge pinned (as far as n allows)."""
    k = rng.integers(0, span, n).astype(np.int64)
    for at, slot in list(zip((n - 1, 0, n - 2, 1),
                             (span - 1, 0, BUCKET - 1, BUCKET)))[:n]:
        k[at] = slot
    return k


def _ints(rng, n):
    """Integer-valued f64 data: every partial sum is exact in any order."""
    return rng.integers(-1000, 1000, n).astype(np.float64)


def _two_call(key_col, vals, agg_op, span):
    """groupby_accum + groupby_compact on caller-owned tables, no counts."""
    nv = len(vals)
    val_cols = [lib.put(v) for v in vals]
    sums = lib.alloc_raw(8 * max(nv, 1) * span)
    rowcnt = lib.alloc_raw(8 * span)
    try:
        lib.fill_f64(sums, lib.AGG_IDENTITY[agg_op], max(nv, 1) * span)
        lib.memset_raw(rowcnt, 0, 8 * span)
        lib.groupby_accum(key_col, val_cols, agg_op, 0, span, sums, rowcnt, 0)
        k, s, _, n = lib.groupby_compact(sums, rowcnt, 0, nv, 0, span)
        assert k.length == n
        return lib.get(k), [lib.get(x) for x in s]
    finally:
        lib.free_raw(sums)
        lib.free_raw(rowcnt)


def _reduce(key_col, vals, agg_op, span, want_counts=False):
    val_cols = [lib.put(v) for v in vals]
    k, s, c, n = lib.groupby_reduce(key_col, val_cols, agg_op, want_counts, 0,
                                    span)
    assert k.length == n
    if want_counts:
        return lib.get(k), [lib.get(x) for x in s], [lib.get(x) for x in c]
    return lib.get(k), [lib.get(x) for x in s]


def _check(keys, vals, agg_op, got, exact=False):
    """Keys exact; values against the oracle on the groups that hold a non-NaN
    value; a group without one keeps the aggregate's identity (no counts are
    requested, so nothing marks it)."""
    named = {str(i): v for i, v in enumerate(vals)}
    ok, oexp = oracle.groupby_agg(keys, named, AGG_NAME[agg_op])
    _, ocnt = oracle.groupby_agg(keys, named, "count")
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


def _both_routes(keys, span, make_vals, agg_op=lib.AGG_SUM, calls=3,
                 exact=False):
    """Each route on a key column of its own: one recording (arming) call, then
    replayed (mapped) calls, every call with fresh values."""
    _geometry(span)
    for route in (_two_call, _reduce):
        key_col = lib.put(keys)
        for _ in range(calls):
            vals = make_vals()
            _check(keys, vals, agg_op, route(key_col, vals, agg_op, span),
                   exact)


@pytest.mark.parametrize("span", [SPAN_MIN, SPAN_EDGE - 1, SPAN_EDGE,
                                  SPAN_EDGE + 1])
def test_spans_and_bucket_edge_keys(span):
    """17 buckets; at SPAN_EDGE the last one is full and the last slot's low
    key is 0x3FFF, at SPAN_EDGE + 1 an 18th bucket holds a single slot.  Keys
    sit at slots 16383 and 16384 and at the last slot."""
    rng = np.random.default_rng(span)
    n = 2 * TILE + 1
    keys = _keys(rng, n, span)
    assert {BUCKET - 1, BUCKET, span - 1, 0} <= set(keys.tolist())
    _both_routes(keys, span, lambda: [_ints(rng, n)], exact=True)


def test_narrower_range_keeps_8192_slot_buckets():
    assert lib.groupby_radix_rl(SPAN_MIN - 1, False) == 13
    assert lib.groupby_radix_rl(SPAN_MIN, True) == 12


@pytest.mark.parametrize("n", [1, 2, TILE - 2, TILE, TILE + 1, 3 * TILE + 1])
def test_row_counts(n):
    """Odd tail row and tile edges: recorded once, replayed twice."""
    rng = np.random.default_rng(100 + n)
    keys = _keys(rng, n, SPAN_MIN)
    _both_routes(keys, SPAN_MIN, lambda: [_ints(rng, n)], exact=True)


@pytest.mark.parametrize("agg_op", [lib.AGG_SUM, lib.AGG_MIN, lib.AGG_MAX])
def test_aggregates(agg_op):
    rng = np.random.default_rng(200 + agg_op)
    n = 2 * TILE + 1
    keys = _keys(rng, n, SPAN_EDGE + 1)
    _both_routes(keys, SPAN_EDGE + 1, lambda: [rng.standard_normal(n)], agg_op)


def test_split_bucket():
    """2^21 + 3 rows in bucket 0 (one more at the last slot): the bucket is
    cut into two work items, the second 3 rows long with an odd tail, so the
    atomic merge and the combine both fold two tables."""
    rng = np.random.default_rng(300)
    n = 2**21 + 4
    keys = rng.integers(0, BUCKET, n).astype(np.int64)
    keys[0], keys[1], keys[n - 1] = 0, BUCKET - 1, SPAN_MIN - 1
    assert (keys < BUCKET).sum() == 2**21 + 3
    _both_routes(keys, SPAN_MIN, lambda: [_ints(rng, n)], calls=2, exact=True)


def test_two_value_columns_and_keys_only():
    rng = np.random.default_rng(400)
    n, span = 2 * TILE + 1, SPAN_EDGE
    keys = _keys(rng, n, span)
    _geometry(span)
    for route in (_two_call, _reduce):
        key_col = lib.put(keys)
        for nv in (2, 0, 1, 2, 0):
            vals = [rng.standard_normal(n) for _ in range(nv)]
            _check(keys, vals, lib.AGG_SUM,
                   route(key_col, vals, lib.AGG_SUM, span))
    # keys-only as the recording call
    for route in (_two_call, _reduce):
        key_col = lib.put(keys)
        for nv in (0, 0, 2):
            vals = [_ints(rng, n) for _ in range(nv)]
            _check(keys, vals, lib.AGG_SUM,
                   route(key_col, vals, lib.AGG_SUM, span), exact=True)


@pytest.mark.parametrize("agg_op", [lib.AGG_SUM, lib.AGG_MIN, lib.AGG_MAX])
def test_nans_and_all_nan_group(agg_op):
    """30 % NaNs, and a group (in the second bucket) whose values are all NaN:
    it stays present and keeps the identity — 0.0 for a sum."""
    rng = np.random.default_rng(500 + agg_op)
    n, span = 2 * TILE + 1, SPAN_MIN
    keys = _keys(rng, n, span)
    lone = BUCKET + 5
    keys[7] = keys[TILE + 7] = lone

    def vals():
        v = rng.standard_normal(n)
        v[rng.random(n) < 0.3] = np.nan
        v[keys == lone] = np.nan
        return [v]

    _both_routes(keys, span, vals, agg_op)
    got = _reduce(lib.put(keys), vals(), agg_op, span)
    at = int(np.searchsorted(got[0], lone))
    assert got[0][at] == lone
    assert got[1][0][at] == lib.AGG_IDENTITY[agg_op]


def test_one_slot_holds_most_rows():
    """90 % of the rows in one slot of the third bucket: one long write run
    per tile, and the register run-accumulator in P2."""
    rng = np.random.default_rng(600)
    n, span = 3 * TILE + 1, SPAN_EDGE + 1
    keys = _keys(rng, n, span)
    head = rng.random(n) < 0.9
    head[[0, 1, n - 2, n - 1]] = False      # keep the pinned edge keys
    keys[head] = 2 * BUCKET + 77
    _both_routes(keys, span, lambda: [_ints(rng, n)], exact=True)
    _both_routes(keys, span, lambda: [rng.standard_normal(n)])


def test_geometry_change_on_one_key_column():
    """sum (16384-slot buckets), then a call with counts (4096), then sum
    again: layout and plan re-record each time and results stay right."""
    rng = np.random.default_rng(700)
    n, span = 2 * TILE + 1, SPAN_MIN
    keys = _keys(rng, n, span)
    key_col = lib.put(keys)
    for wc in (False, False, True, True, False, False):
        _geometry(span, wc)
        v = _ints(rng, n)
        got = _reduce(key_col, [v], lib.AGG_SUM, span, wc)
        _check(keys, [v], lib.AGG_SUM, got, exact=True)
        if wc:
            _, ocnt = oracle.groupby_agg(keys, {"v": v}, "count")
            np.testing.assert_array_equal(got[2][0], ocnt["v"])
    # the same through the frame API: sum, mean, sum on one frame
    import modin_amd.pandas as mpd
    v = _ints(rng, n)
    df = mpd.DataFrame({"k": keys, "v": v})
    for agg in ("sum", "mean", "sum", "sum"):
        ok, oexp = oracle.groupby_agg(keys, {"v": v}, agg)
        out = getattr(df.groupby("k"), agg)().to_pandas()
        np.testing.assert_array_equal(out.index.to_numpy(), ok)
        np.testing.assert_allclose(out["v"].to_numpy(), oexp["v"], rtol=RTOL,
                                   atol=ATOL)


def test_out_of_range_key_raises_on_every_call():
    """50 slots too few, still above the 2^18 bound: the recording call and
    every replay raise, and no group map is armed."""
    rng = np.random.default_rng(800)
    n, span = TILE + 1, SPAN_EDGE
    keys = _keys(rng, n, span)
    _geometry(span - 50)
    for route in (_two_call, _reduce):
        key_col = lib.put(keys)
        for _ in range(3):
            with pytest.raises(lib.HfError, match="outside"):
                route(key_col, [_ints(rng, n)], lib.AGG_SUM, span - 50)
        # the raise cleared the error word; the full range works, twice
        for _ in range(2):
            v = _ints(rng, n)
            _check(keys, [v], lib.AGG_SUM,
                   route(key_col, [v], lib.AGG_SUM, span), exact=True)


def test_forced_8192_slot_buckets_child_process():
    """The cases above with HF_GB_RL=13 (read once per process, hence the fresh
    child, which leaves this test out), where the query answers 13 for the
    same ranges."""
    env = dict(os.environ, HF_GB_RL="13")
    probe = subprocess.run(
        [sys.executable, "-c",
         "from modin_amd.core import lib; "
         f"print(lib.groupby_radix_rl({SPAN_MIN}, False))"],
        env=env, capture_output=True, text=True, timeout=120,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert probe.stdout.strip() == "13", probe.stdout + probe.stderr
    res = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
         "-k", "not child_process", os.path.abspath(__file__)],
        env=env, capture_output=True, text=True, timeout=600)
    tail = res.stdout[-3000:] + res.stderr[-1000:]
    assert res.returncode == 0, tail
    assert " passed" in res.stdout and "failed" not in res.stdout, tail
