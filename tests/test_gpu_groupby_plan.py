"""GPU tier: the radix groupby's cached scatter plan (record once per key
column, replay as a pure value permutation).

Everything goes through lib.groupby_accum / lib.groupby_compact on one key
column that is reused across rounds, against oracle.groupby_agg.  Contract:
keys, presence and counts exact; f64 sums rtol=1e-12, atol=1e-9.

Sizes are the smallest at which tiling, tails and bucket edges can go wrong:
the plan tile is 12288 rows, a sum-only bucket holds 8192 keys (4096 when
counts are requested), and the radix path starts above 8192 slots.
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
PLAN_ON = os.environ.get("HF_GB_PLAN", "1")[:1] != "0"


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _round(key_col, vals, kmin, n_slots, want_counts=False):
    """One accumulate+compact round on an existing device key column."""
    nv = len(vals)
    val_cols = [lib.put(v) for v in vals]
    sums = lib.alloc_raw(8 * max(nv, 1) * n_slots)
    rowcnt = lib.alloc_raw(8 * n_slots)
    counts = lib.alloc_raw(8 * nv * n_slots) if want_counts and nv else 0
    try:
        lib.memset_raw(sums, 0, 8 * max(nv, 1) * n_slots)
        lib.memset_raw(rowcnt, 0, 8 * n_slots)
        if counts:
            lib.memset_raw(counts, 0, 8 * nv * n_slots)
        lib.groupby_accum(key_col, val_cols, lib.AGG_SUM, kmin, n_slots, sums,
                          rowcnt, counts)
        kout, sout, cout, _ = lib.groupby_compact(sums, rowcnt, counts, nv,
                                                  kmin, n_slots)
        return (lib.get(kout), [lib.get(s) for s in sout],
                [lib.get(c) for c in cout] if counts else None)
    finally:
        lib.free_raw(sums)
        lib.free_raw(rowcnt)
        if counts:
            lib.free_raw(counts)


def _check(keys, vals, got, want_counts=False):
    gk, gs, gc = got
    named = {str(i): v for i, v in enumerate(vals)}
    ok, _ = oracle.groupby_agg(keys, {}, "sum")
    np.testing.assert_array_equal(gk, ok)
    _, osums = oracle.groupby_agg(keys, named, "sum")
    _, ocnts = oracle.groupby_agg(keys, named, "count")
    for i in range(len(vals)):
        np.testing.assert_allclose(gs[i], osums[str(i)], rtol=RTOL, atol=ATOL)
        if want_counts:
            np.testing.assert_array_equal(gc[i], ocnts[str(i)])


def _keys(rng, n, span, kmin):
    """Uniform keys over [kmin, kmin+span) with both range ends pinned where
    there is room (n >= 2), so n_slots == span exactly."""
    k = rng.integers(kmin, kmin + span, n).astype(np.int64)
    if n >= 2:
        k[0], k[n - 1] = kmin, kmin + span - 1
    return k


def _rounds(keys, kmin, span, nvals_seq, rng, counts_seq=None, nan_frac=0.0):
    """Successive rounds on ONE device key column (first records the plan,
    the rest replay it), each with fresh value columns, each checked."""
    key_col = lib.put(keys)
    for r, nv in enumerate(nvals_seq):
        wc = bool(counts_seq[r]) if counts_seq else False
        vals = [rng.standard_normal(keys.size) for _ in range(nv)]
        for v in vals:
            v[rng.random(v.size) < nan_frac] = np.nan
        _check(keys, vals, _round(key_col, vals, kmin, span, wc), wc)


@pytest.mark.parametrize("n", [1, 2, TILE - 2, TILE, TILE + 1, 3 * TILE + 1])
def test_row_counts(n):
    rng = np.random.default_rng(100 + n)
    span, kmin = 8193, -17
    keys = _keys(rng, n, span, kmin)
    _rounds(keys, kmin, span, [1, 1, 2], rng)


@pytest.mark.parametrize("span,counts", [(8193, False), (3 * 8192 + 5, False),
                                         (3 * 4096 + 1, True)])
def test_key_spans(span, counts):
    rng = np.random.default_rng(span)
    kmin = 1000
    keys = _keys(rng, 3 * TILE + 1, span, kmin)
    _rounds(keys, kmin, span, [1, 1, 1], rng, counts_seq=[counts] * 3)


def test_repeated_calls_record_once_then_replay():
    rng = np.random.default_rng(7)
    span, kmin = 3 * 8192 + 5, 0
    keys = _keys(rng, 3 * TILE + 1, span, kmin)
    lib.profiling(True)
    lib.kernel_stats_reset()
    try:
        _rounds(keys, kmin, span, [1, 1, 1], rng)
        rec, _ = lib.kernel_stats("gb_plan_record")
        scat, _ = lib.kernel_stats("gb_scatter")
        k32, _ = lib.kernel_stats("gb_keys32")
    finally:
        lib.profiling(False)
    if PLAN_ON:
        assert (rec, scat, k32) == (1, 2, 0)
    else:  # HF_GB_PLAN=0: the plan-less path, scattering on every round
        assert (rec, scat, k32) == (0, 3, 1)


def test_plan_invalidation_sum_counts_sum():
    rng = np.random.default_rng(8)
    span, kmin = 3 * 8192 + 5, -4000
    keys = _keys(rng, 3 * TILE + 1, span, kmin)
    # counts switch the bucket width (8192 -> 4096 keys), so each change
    # re-records; the last round must not see the first round's plan
    _rounds(keys, kmin, span, [1, 1, 1], rng, counts_seq=[0, 1, 0])


def test_nslots_change_inside_one_bucket_count():
    """Same key_min and bucket count, different n_slots: the rows between the
    two bounds are out of range for the narrow call only, so the cached
    histogram and plan of one must not serve the other."""
    rng = np.random.default_rng(9)
    kmin, wide, narrow = 0, 8192 + 100, 8192 + 50
    keys = _keys(rng, TILE + 1, wide, kmin)
    key_col = lib.put(keys)
    v = rng.random(keys.size)
    _check(keys, [v], _round(key_col, [v], kmin, wide))
    with pytest.raises(lib.HfError, match="outside"):
        _round(key_col, [v], kmin, narrow)
    _check(keys, [v], _round(key_col, [v], kmin, wide))


@pytest.mark.parametrize("nvals", [0, 1, 2, 3])
def test_value_column_counts(nvals):
    rng = np.random.default_rng(20 + nvals)
    span, kmin = 8193, 5
    keys = _keys(rng, TILE + 1, span, kmin)
    _rounds(keys, kmin, span, [nvals, nvals], rng)
    # and a plan recorded by a keys-only call serves value columns later
    _rounds(keys, kmin, span, [0, nvals, 0], rng)


def test_nan_values_and_all_nan_group():
    rng = np.random.default_rng(30)
    span, kmin = 3 * 4096 + 1, 0
    keys = _keys(rng, 3 * TILE + 1, span, kmin)
    keys[5] = keys[TILE + 5] = kmin + 4097
    key_col = lib.put(keys)
    for _ in range(2):
        v = rng.standard_normal(keys.size)
        v[rng.random(v.size) < 0.1] = np.nan
        v[keys == kmin + 4097] = np.nan
        gk, gs, gc = got = _round(key_col, [v], kmin, span, True)
        _check(keys, [v], got, True)
        at = int(np.searchsorted(gk, kmin + 4097))
        assert gk[at] == kmin + 4097 and gs[0][at] == 0.0 and gc[0][at] == 0


@pytest.mark.parametrize("dist", ["one_key", "last_bucket", "zipf_head"])
def test_key_distributions(dist):
    rng = np.random.default_rng(40)
    n, span, kmin = 3 * TILE + 1, 3 * 8192 + 5, 0
    if dist == "one_key":
        keys = np.full(n, kmin + 9000, dtype=np.int64)
    elif dist == "last_bucket":
        keys = rng.integers(kmin + 3 * 8192, kmin + span, n).astype(np.int64)
    else:
        # zipf-like: bucket 0 takes ~95 % of every tile, the rest spread
        head = rng.zipf(1.2, n) % 8192
        keys = np.where(rng.random(n) < 0.95, head,
                        rng.integers(8192, span, n)).astype(np.int64) + kmin
        for t in range(0, n - TILE + 1, TILE):
            assert (keys[t:t + TILE] - kmin < 8192).mean() > 0.9
    _rounds(keys, kmin, span, [1, 1, 2], rng, nan_frac=0.05)


def test_bucket_split_into_two_work_items_with_odd_tail():
    """One bucket above AGG_CHUNK (2^21 rows per aggregate work item) is split
    into two items; its odd row count leaves the second item an odd tail.
    Bucket 0 takes every row but 101 drawn ones and the pinned last row, which
    land in the last bucket.  Keys stay below 4096, so bucket 0 is the same
    with counts (4096-key buckets) as without (8192)."""
    agg_chunk = 2**21
    rng = np.random.default_rng(70)
    n, span, kmin = 2**21 + 2**20 + 3, 8192 + 300, -5
    keys = rng.integers(kmin, kmin + 4096, n).astype(np.int64)
    keys[rng.choice(np.arange(1, n - 1), 101, replace=False)] = \
        rng.integers(kmin + 8192, kmin + span, 101)
    keys[0], keys[n - 1] = kmin, kmin + span - 1  # pinned ends: n_slots == span
    in_b0 = int((keys - kmin < 4096).sum())
    assert in_b0 == n - 102 and in_b0 % 2 == 1 and in_b0 > agg_chunk
    _rounds(keys, kmin, span, [1, 2], rng, counts_seq=[0, 1], nan_frac=0.05)


def test_out_of_range_key_raises_on_record_and_on_replay():
    rng = np.random.default_rng(50)
    span, kmin = 8192 + 300, 0
    keys = _keys(rng, TILE + 1, span, kmin)
    keys[TILE // 2] = kmin + span + 7
    key_col = lib.put(keys)
    v = rng.random(keys.size)
    for _ in range(3):  # recording call, then two replayed calls
        with pytest.raises(lib.HfError, match="outside"):
            _round(key_col, [v], kmin, span)
    with pytest.raises(lib.HfError, match="outside"):
        _round(key_col, [], kmin, span)  # keys-only on the recorded plan
    # the error word is cleared by the raise: a clean column passes after it
    good = _keys(rng, TILE + 1, span, kmin)
    _check(good, [v], _round(lib.put(good), [v], kmin, span))


def test_allocator_reuse_gets_no_stale_plan():
    rng = np.random.default_rng(60)
    n, span, kmin = 3 * TILE + 1, 8193, 0
    keys = _keys(rng, n, span, kmin)
    key_col = lib.put(keys)
    v = rng.random(n)
    _check(keys, [v], _round(key_col, [v], kmin, span))
    _check(keys, [v], _round(key_col, [v], kmin, span))
    del key_col  # frees the column and its plan into the allocator's cache
    keys2 = _keys(rng, n, span, kmin)
    key_col2 = lib.put(keys2)  # same length: the allocator hands memory back
    _check(keys2, [v], _round(key_col2, [v], kmin, span))
    _check(keys2, [v], _round(key_col2, [v], kmin, span))


def test_disabled_plan_child_process():
    """The same cases on the plan-less path (HF_GB_PLAN=0 is read once per
    process, hence the fresh child, which runs every case but this one)."""
    env = dict(os.environ, HF_GB_PLAN="0")
    res = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
         "-k", "not disabled_plan_child", os.path.abspath(__file__)],
        env=env, capture_output=True, text=True, timeout=300)
    tail = res.stdout[-3000:] + res.stderr[-1000:]
    assert res.returncode == 0, tail
    assert " passed" in res.stdout and "failed" not in res.stdout, tail
