"""GPU tier: loop edges of the two streaming groupby kernels that keep several
row pairs in flight per lane — the radix path's bucket aggregate (P2,
k_gb_bucket_agg) and the dense path (k_gb_dense, n_slots <= 8192).

Both kernels run 512 threads, two rows per lane per load, and issue U
block-strides of loads before they consume the first; whatever is left goes
one stride at a time, and an odd last row on its own.  One trip of the
unrolled body therefore covers B = 1024 * U rows of a P2 work item (or of a
one-block dense grid).  The row counts below sit on both sides of B, of a
further stride and of several trips for U = 2, 4 and 8 alike, so the cases do
not depend on the depth the build uses.

Contract: keys and counts exact; f64 values rtol=1e-12, atol=1e-9.  Values
are small integers stored as f64, so sums, minima and maxima are exact in any
order and are compared for equality with oracle.groupby_agg — a row dropped
or fed twice at a loop boundary cannot hide in a tolerance.  Every frame (or
key column) is called three times: the first call arms the group map through
the accumulate + compact route, the later ones run the partial-table flush.
"""

import numpy as np
import pytest

import oracle
from modin_amd.core import lib

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-9
BODIES = (2048, 4096, 8192)          # rows per body trip for U = 2, 4, 8
P2_ROWS = [1, 2, 3] + [r for b in BODIES
                       for r in (b - 1, b, b + 1, b + 2, b + 1024 + 3,
                                 3 * b + 5)]
DENSE_ROWS = [1, 2, 3] + [r for b in BODIES for r in (b - 1, b, b + 1)] + \
    [2 * 65536 + 1]                  # the last one runs a grid of 3 blocks
EXACT = ("sum", "min", "max", "count")


@pytest.fixture(autouse=True)
def _ready(gpu_ready):
    yield


def _int_values(rng, n, nan):
    """Integers in [-1000, 1000) as f64 (|v| < 2^20), ~10 % NaN on request."""
    v = rng.integers(-1000, 1000, n).astype(np.float64)
    if nan:
        v[rng.random(n) < 0.1] = np.nan
    return v


def _bucket0_keys(rng, rows, agg, skew=False):
    """`rows` rows in bucket 0 and one row at key 8192: 8193 slots, so the
    radix route, with bucket 0 a single work item of `rows` rows.  Mean, min
    and max take 4096-key buckets, so their keys stay in [0, 4096)."""
    span = 8192 if agg == "sum" else 4096
    keys = rng.integers(0, span, rows + 1).astype(np.int64)
    if skew:  # 90 % of the rows on one slot
        keys[rng.random(rows + 1) < 0.9] = 77
    keys[0], keys[rows] = 0, 8192
    return keys


def _frame_check(keys, cols, agg, calls=3):
    import modin_amd.pandas as mpd
    df = mpd.DataFrame({"k": keys, **cols})
    ok, oexp = oracle.groupby_agg(keys, cols, agg)
    for _ in range(calls):
        out = getattr(df.groupby("k"), agg)().to_pandas()
        np.testing.assert_array_equal(out.index.to_numpy(), ok)
        for name in cols:
            got = out[name].to_numpy()
            if agg in EXACT:
                np.testing.assert_array_equal(got, oexp[name])
            else:
                np.testing.assert_allclose(got, oexp[name], rtol=RTOL,
                                           atol=ATOL)


# --------------------------------------------------------------------------
# P2: k_gb_bucket_agg
# --------------------------------------------------------------------------

@pytest.mark.parametrize("nan", [False, True], ids=["dense", "nan"])
@pytest.mark.parametrize("agg", ["sum", "mean", "min", "max"])
@pytest.mark.parametrize("rows", P2_ROWS)
def test_p2_body_edges(rows, agg, nan):
    rng = np.random.default_rng(7000 + rows)
    keys = _bucket0_keys(rng, rows, agg)
    _frame_check(keys, {"a": _int_values(rng, rows + 1, nan)}, agg)


@pytest.mark.parametrize("agg", ["sum", "mean", "max"])
@pytest.mark.parametrize("rows", [4096 + 1024 + 3, 3 * 8192 + 5])
def test_p2_skewed_head_slot(rows, agg):
    """Run-accumulation in registers follows a lane's row order: with 90 % of
    the rows on one slot nearly every feed extends a run."""
    rng = np.random.default_rng(7100 + rows)
    keys = _bucket0_keys(rng, rows, agg, skew=True)
    _frame_check(keys, {"a": _int_values(rng, rows + 1, True)}, agg)


def _keys_only(key_col, n_slots):
    """hf_groupby_accum with no value column, then the compaction."""
    rowcnt = lib.alloc_raw(8 * n_slots)
    sums = lib.alloc_raw(8 * n_slots)
    try:
        lib.memset_raw(rowcnt, 0, 8 * n_slots)
        lib.fill_f64(sums, 0.0, n_slots)
        lib.groupby_accum(key_col, [], lib.AGG_SUM, 0, n_slots, sums, rowcnt,
                          0)
        k, _, _, n = lib.groupby_compact(sums, rowcnt, 0, 0, 0, n_slots)
        assert k.length == n
        return lib.get(k)
    finally:
        lib.free_raw(rowcnt)
        lib.free_raw(sums)


@pytest.mark.parametrize("rows", P2_ROWS)
def test_p2_keys_only(rows):
    """The ushort2-only stream: presence marks and nothing else.  Keys step
    by 3, so a mark on a wrong slot shows as an extra group."""
    rng = np.random.default_rng(7200 + rows)
    keys = (rng.integers(0, 8192 // 3, rows + 1) * 3).astype(np.int64)
    keys[0], keys[rows] = 0, 8192
    key_col = lib.put(keys)
    want = np.unique(keys)
    for _ in range(3):
        np.testing.assert_array_equal(_keys_only(key_col, 8193), want)


@pytest.mark.parametrize("agg", ["sum", "mean"])
def test_p2_second_work_item_edges(agg):
    """2^21 + 8192 + 1 rows in bucket 0: the second work item starts at row
    2^21 of the bucket and has 8193 rows — whole body trips and an odd last
    row — and the combine folds it with the first item's table."""
    rng = np.random.default_rng(7300)
    rows = 2**21 + 8192 + 1
    keys = _bucket0_keys(rng, rows, agg)
    _frame_check(keys, {"a": _int_values(rng, rows + 1, True)}, agg)


# --------------------------------------------------------------------------
# dense: k_gb_dense
# --------------------------------------------------------------------------

HOW = {"sum": (lib.AGG_SUM, False), "mean": (lib.AGG_SUM, True),
       "min": (lib.AGG_MIN, True)}


def _dense_reduce(key_col, v, how, kmin, n_slots):
    agg_op, wc = HOW[how]
    k, s, c, n = lib.groupby_reduce(key_col, [lib.put(v)], agg_op, wc, kmin,
                                    n_slots)
    assert k.length == n
    return lib.get(k), lib.get(s[0]), lib.get(c[0]) if wc else None


def _dense_check(keys, v, how, kmin, n_slots, calls=3):
    named = {"v": v}
    ok, oval = oracle.groupby_agg(keys, named, "min" if how == "min" else "sum")
    _, ocnt = oracle.groupby_agg(keys, named, "count")
    key_col = lib.put(keys)
    for _ in range(calls):
        gk, gs, gc = _dense_reduce(key_col, v, how, kmin, n_slots)
        np.testing.assert_array_equal(gk, ok)
        if gc is None:
            np.testing.assert_array_equal(gs, oval["v"])
        else:
            np.testing.assert_array_equal(gc, ocnt["v"])
            live = gc > 0  # an all-NaN group keeps the identity in its slot
            np.testing.assert_array_equal(gs[live], oval["v"][live])


@pytest.mark.parametrize("nan", [False, True], ids=["dense", "nan"])
@pytest.mark.parametrize("how", ["sum", "mean", "min"])
@pytest.mark.parametrize("n_slots", [1, 4096, 8192])
@pytest.mark.parametrize("n", DENSE_ROWS)
def test_dense_body_edges(n, n_slots, how, nan):
    rng = np.random.default_rng(8000 + n + n_slots)
    keys = rng.integers(0, n_slots, n).astype(np.int64)
    _dense_check(keys, _int_values(rng, n, nan), how, 0, n_slots)


@pytest.mark.parametrize("kmin", [-17, 10**12])
@pytest.mark.parametrize("n", [3, 8193, 2 * 65536 + 1])
def test_dense_nonzero_key_min(n, kmin):
    rng = np.random.default_rng(8100 + n)
    keys = rng.integers(kmin, kmin + 4096, n).astype(np.int64)
    _dense_check(keys, _int_values(rng, n, True), "mean", kmin, 4096)


# 8192 rows are whole body trips for every depth; the 515 pairs after them
# are less than one stride past a trip boundary, so they run one stride at a
# time; the last of the odd row count is the single-row tail.
OOR_N = 8192 + 2 * 515 + 1
OOR_AT = {"body": 5, "remainder": OOR_N - 3, "tail": OOR_N - 1}


@pytest.mark.parametrize("bad", [4096, -1], ids=["above", "below"])
@pytest.mark.parametrize("where", sorted(OOR_AT))
def test_dense_out_of_range_key_raises(where, bad):
    rng = np.random.default_rng(8200)
    keys = rng.integers(0, 4096, OOR_N).astype(np.int64)
    good = keys.copy()
    keys[OOR_AT[where]] = bad
    v = _int_values(rng, OOR_N, False)
    key_col = lib.put(keys)
    for _ in range(3):
        with pytest.raises(lib.HfError, match="outside"):
            _dense_reduce(key_col, v, "sum", 0, 4096)
    # the raise cleared the error word: the same rows without the bad key
    _dense_check(good, v, "sum", 0, 4096, calls=1)
