"""GPU tier: the single-call groupby (hf_groupby_reduce) and the group map it
caches on the key column next to the scatter plan.

The first call on a key column takes the accumulate + compact path and arms
the map; later calls replay the plan, flush per-work-item partial tables and
fold them straight into the output (no dense tables, no compaction).  Every
case calls the same frame (or key column) three times and checks each result
against oracle.groupby_agg.  Contract: keys and counts exact; f64 values
rtol=1e-12, atol=1e-9.

Sizes are the smallest at which tiling, tails and bucket edges can go wrong:
the plan tile is 12288 rows, a sum-only bucket holds 8192 keys (4096 when
counts are requested), a work item holds 2^21 rows, and the radix path starts
above 8192 slots.
"""

import gc
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
PLAN_ON = os.environ.get("HF_GB_PLAN", "1")[:1] != "0"


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _keys(rng, n, span, kmin=0):
    """Uniform keys over [kmin, kmin+span), both range ends pinned."""
    k = rng.integers(kmin, kmin + span, n).astype(np.int64)
    k[0], k[n - 1] = kmin, kmin + span - 1
    return k


def _frame_check(keys, cols, agg, calls=3, df=None):
    """The same frame `calls` times through DataFrame.groupby(...).<agg>()."""
    import modin_amd.pandas as mpd
    if df is None:
        df = mpd.DataFrame({"k": keys, **cols})
    ok, oexp = oracle.groupby_agg(keys, cols, agg)
    for _ in range(calls):
        out = getattr(df.groupby("k"), agg)().to_pandas()
        np.testing.assert_array_equal(out.index.to_numpy(), ok)
        for name in cols:
            got = out[name].to_numpy()
            if agg == "count":
                np.testing.assert_array_equal(got, oexp[name])
            else:
                np.testing.assert_allclose(got, oexp[name], rtol=RTOL,
                                           atol=ATOL)
    return df


def _reduce(key_col, vals, agg_op, want_counts, kmin, n_slots):
    val_cols = [lib.put(v) for v in vals]
    k, s, c, n = lib.groupby_reduce(key_col, val_cols, agg_op, want_counts,
                                    kmin, n_slots)
    assert k.length == n
    return (lib.get(k), [lib.get(x) for x in s],
            [lib.get(x) for x in c] if want_counts else None)


def _two_call(key_col, vals, agg_op, want_counts, kmin, n_slots):
    """The accumulate + compact pair on caller-owned tables."""
    nv = len(vals)
    val_cols = [lib.put(v) for v in vals]
    sums = lib.alloc_raw(8 * max(nv, 1) * n_slots)
    rowcnt = lib.alloc_raw(8 * n_slots)
    counts = lib.alloc_raw(8 * nv * n_slots) if want_counts else 0
    try:
        lib.fill_f64(sums, lib.AGG_IDENTITY[agg_op], max(nv, 1) * n_slots)
        lib.memset_raw(rowcnt, 0, 8 * n_slots)
        if counts:
            lib.memset_raw(counts, 0, 8 * nv * n_slots)
        lib.groupby_accum(key_col, val_cols, agg_op, kmin, n_slots, sums,
                          rowcnt, counts)
        k, s, c, _ = lib.groupby_compact(sums, rowcnt, counts, nv, kmin,
                                         n_slots)
        return (lib.get(k), [lib.get(x) for x in s],
                [lib.get(x) for x in c] if counts else None)
    finally:
        lib.free_raw(sums)
        lib.free_raw(rowcnt)
        if counts:
            lib.free_raw(counts)


def _lib_check(keys, vals, got, want_counts):
    gk, gs, gcn = got
    named = {str(i): v for i, v in enumerate(vals)}
    ok, osums = oracle.groupby_agg(keys, named, "sum")
    _, ocnts = oracle.groupby_agg(keys, named, "count")
    np.testing.assert_array_equal(gk, ok)
    for i in range(len(vals)):
        np.testing.assert_allclose(gs[i], osums[str(i)], rtol=RTOL, atol=ATOL)
        if want_counts:
            np.testing.assert_array_equal(gcn[i], ocnts[str(i)])


@pytest.mark.parametrize("agg", ["sum", "mean", "min", "max"])
@pytest.mark.parametrize("n", [5, TILE, 2 * TILE + 1])
def test_row_counts_and_aggs(n, agg):
    """8193 slots: two 8192-key buckets for sum (the second holds one slot),
    three 4096-key buckets when counts are wanted (mean, min, max)."""
    rng = np.random.default_rng(1000 + n)
    keys = _keys(rng, n, 8193, kmin=-17)
    _frame_check(keys, {"a": rng.standard_normal(n)}, agg)


@pytest.mark.parametrize("agg", ["sum", "mean"])
def test_two_work_items_in_one_bucket(agg):
    """2^21 + 3 rows, all but one in [0, 8192): bucket 0 is cut into two work
    items, the second 2 rows long, so the combine folds two partial tables."""
    rng = np.random.default_rng(11)
    n = 2**21 + 3
    keys = rng.integers(0, 4096 if agg == "mean" else 8192, n).astype(np.int64)
    keys[0], keys[n - 1] = 0, 8192
    if agg == "mean":  # 4096-key buckets: keep the last row alone in bucket 2
        assert ((keys >= 4096) & (keys < 8192)).sum() == 0
    _frame_check(keys, {"a": rng.standard_normal(n)}, agg)


@pytest.mark.parametrize("agg", ["sum", "mean"])
def test_ten_work_items_in_one_bucket(agg):
    """The combine folds a bucket's partial tables eight at a time and then
    one by one: 9 * 2^21 + 5 rows in bucket 0 make nine full work items and a
    4-row one, so both loops run (with the counts tables for mean)."""
    rng = np.random.default_rng(21)
    n = 9 * 2**21 + 5
    keys = rng.integers(0, 4096 if agg == "mean" else 8192, n).astype(np.int64)
    keys[0], keys[n - 1] = 0, 8192
    v = rng.standard_normal(n)
    v[::1000] = np.nan
    _frame_check(keys, {"a": v}, agg)


@pytest.mark.parametrize("agg", ["sum", "count", "max"])
def test_sparse_keys_leave_absent_slots(agg):
    rng = np.random.default_rng(12)
    n = 2 * TILE + 1
    keys = (rng.integers(0, 20000 // 3, n) * 3).astype(np.int64) + 100
    keys[0], keys[n - 1] = 100, 100 + 3 * (20000 // 3 - 1)
    assert np.unique(keys).size < keys.max() - keys.min() + 1
    _frame_check(keys, {"a": rng.standard_normal(n)}, agg)


@pytest.mark.parametrize("agg_op", [lib.AGG_SUM, lib.AGG_MIN, lib.AGG_MAX])
def test_nan_values_and_all_nan_group(agg_op):
    """A group whose values are all NaN stays present: sum 0.0 and count 0;
    its min/max slot carries what the two-call path leaves there."""
    rng = np.random.default_rng(13)
    n, span = 2 * TILE + 1, 3 * 4096 + 1
    keys = _keys(rng, n, span)
    keys[5] = keys[TILE + 5] = 4097
    v = rng.standard_normal(n)
    v[rng.random(n) < 0.1] = np.nan
    v[keys == 4097] = np.nan
    ref = _two_call(lib.put(keys), [v], agg_op, True, 0, span)
    how = {lib.AGG_SUM: "sum", lib.AGG_MIN: "min", lib.AGG_MAX: "max"}[agg_op]
    ok, oexp = oracle.groupby_agg(keys, {"v": v}, how)
    _, ocnt = oracle.groupby_agg(keys, {"v": v}, "count")
    at = int(np.searchsorted(ok, 4097))
    key_col = lib.put(keys)
    for _ in range(3):
        gk, gs, gcn = _reduce(key_col, [v], agg_op, True, 0, span)
        np.testing.assert_array_equal(gk, ok)
        np.testing.assert_array_equal(gcn[0], ocnt["v"])
        live = gcn[0] > 0
        np.testing.assert_allclose(gs[0][live], oexp["v"][live], rtol=RTOL,
                                   atol=ATOL)
        assert gk[at] == 4097 and gcn[0][at] == 0
        assert gs[0][at] == ref[1][0][at]
        if agg_op == lib.AGG_SUM:
            assert gs[0][at] == 0.0


def test_three_value_columns_then_new_values():
    rng = np.random.default_rng(14)
    n = 2 * TILE + 1
    keys = _keys(rng, n, 3 * 8192 + 5, kmin=1000)
    cols = {c: rng.standard_normal(n) for c in "abcw"}
    cols["b"][rng.random(n) < 0.05] = np.nan
    import modin_amd.pandas as mpd
    df = mpd.DataFrame({"k": keys, **cols})
    abc = {c: cols[c] for c in "abc"}
    _frame_check(keys, abc, "sum", df=df[["k", "a", "b", "c"]])
    # the same device key column under another value column
    _frame_check(keys, {"w": cols["w"]}, "sum", calls=2, df=df[["k", "w"]])


def test_new_values_on_one_key_column_lib_level():
    """Fresh value columns on every call, 1 then 3 then 0 then 2 of them."""
    rng = np.random.default_rng(15)
    n, span, kmin = 2 * TILE + 1, 8193, -5
    keys = _keys(rng, n, span, kmin)
    key_col = lib.put(keys)
    for nv, wc in [(1, False), (3, False), (0, False), (2, False), (2, True),
                   (2, True)]:
        vals = [rng.standard_normal(n) for _ in range(nv)]
        _lib_check(keys, vals, _reduce(key_col, vals, lib.AGG_SUM, wc, kmin,
                                       span), wc)


def _stats(names):
    return {m: lib.kernel_stats(m)[0] for m in names}


@pytest.mark.parametrize("nvals", [1, 3])
def test_steady_state_launches(nvals):
    names = ["gb_compact_count", "gb_compact_scan", "gb_scatter",
             "gb_bucket_agg", "gb_compact_scatter", "gb_plan_record"]
    rng = np.random.default_rng(16)
    n, span = 2 * TILE + 1, 3 * 8192 + 5
    keys = _keys(rng, n, span)
    key_col = lib.put(keys)
    vals = [rng.standard_normal(n) for _ in range(nvals)]
    lib.profiling(True)
    lib.kernel_stats_reset()
    try:
        _lib_check(keys, vals, _reduce(key_col, vals, lib.AGG_SUM, False, 0,
                                       span), False)
        s0 = _stats(names)
        _lib_check(keys, vals, _reduce(key_col, vals, lib.AGG_SUM, False, 0,
                                       span), False)
        s1 = _stats(names)
    finally:
        lib.profiling(False)
    d = {m: s1[m] - s0[m] for m in names}
    if PLAN_ON:
        assert s0["gb_plan_record"] == 1 and s0["gb_compact_count"] == 1
        assert d == {"gb_compact_count": 0, "gb_compact_scan": 0,
                     "gb_scatter": nvals, "gb_bucket_agg": nvals,
                     "gb_compact_scatter": nvals, "gb_plan_record": 0}
    else:  # HF_GB_PLAN=0: no plan, no map — the compaction runs every call
        assert d["gb_compact_count"] == 1 and d["gb_compact_scatter"] == 1
        assert d["gb_plan_record"] == 0


def test_wider_range_then_original_rerecords():
    rng = np.random.default_rng(17)
    n, span, kmin = 2 * TILE + 1, 8192 + 100, 50
    keys = _keys(rng, n, span, kmin)
    key_col = lib.put(keys)
    v = rng.standard_normal(n)
    geoms = [(kmin, span)] * 2 + [(kmin - 7, span + 9000)] * 2 + \
        [(kmin, span)] * 2
    for km, ns in geoms:
        _lib_check(keys, [v], _reduce(key_col, [v], lib.AGG_SUM, False, km,
                                      ns), False)


def test_too_few_slots_raises_on_every_call():
    rng = np.random.default_rng(18)
    n, span = TILE + 1, 8192 + 300
    keys = _keys(rng, n, span)
    key_col = lib.put(keys)
    v = rng.random(n)
    for _ in range(3):
        with pytest.raises(lib.HfError, match="outside"):
            _reduce(key_col, [v], lib.AGG_SUM, False, 0, span - 50)
    # the raise cleared the error word, and no map was left behind
    for _ in range(2):
        _lib_check(keys, [v], _reduce(key_col, [v], lib.AGG_SUM, False, 0,
                                      span), False)


def test_device_blocks_balance():
    rng = np.random.default_rng(19)
    n, span = 2 * TILE + 1, 8193
    keys = _keys(rng, n, span)
    gc.collect()
    base = lib.dev_live()
    key_col = lib.put(keys)
    for wc in (False, False, True, True, False):
        v = rng.standard_normal(n)
        got = _reduce(key_col, [v], lib.AGG_SUM, wc, 0, span)
        _lib_check(keys, [v], got, wc)
    assert lib.dev_live() > base
    del key_col, got
    gc.collect()
    assert lib.dev_live() == base
    _frame_check(keys, {"a": rng.standard_normal(n)}, "mean")
    gc.collect()
    assert lib.dev_live() == base


def test_disabled_plan_child_process():
    """Two of the cases above on the plan-less path (HF_GB_PLAN=0 is read once
    per process, hence the fresh child): equal results, and the compaction
    runs on every call."""
    env = dict(os.environ, HF_GB_PLAN="0")
    res = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
         "-k", "steady_state_launches or sparse_keys",
         os.path.abspath(__file__)],
        env=env, capture_output=True, text=True, timeout=300)
    tail = res.stdout[-3000:] + res.stderr[-1000:]
    assert res.returncode == 0, tail
    assert " passed" in res.stdout and "failed" not in res.stdout, tail
